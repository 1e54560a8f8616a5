// nerf_view.hip -- the view around the NeRF stage's training render (include/dwg_nerf_view.h, boundary B20).
//
//   k_view_rays              one thread per pixel: the ray of view_math.h's view_ray from the camera in device memory, stored, and the
//                            slab test of raymarch_common.h's near_far_ray on the stored values (the bits of k_near_far on these rays)
//   k_view_compose_forward   one thread per pixel: reads its [C] row of image_fg, weights_sum and the background, writes the C planes;
//                            with a sparsity loss, the three fp64 terms are summed over the workgroup into its own slot
//   k_view_sparsity_finish   one workgroup adds the slots in index order -> the three totals (kept for the backward) and the loss
//   k_view_compose_backward  one thread per pixel: d image_fg, d weights_sum, d image_bg
//
// All three are streaming kernels: a few floats per pixel each way, no reuse, nothing staged.  Rows of [N, C] are read by one lane
// each (C = 4: one 16-byte load; C = 3: three dword loads that the wave's 64 lanes cover without gaps); the planes are written with
// consecutive lanes on consecutive addresses, N = H * W being linear so an odd W changes nothing.  Sums are fp64 in a fixed order
// (wave butterfly, waves in order, slots in order): no atomics, two runs give the same bits.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_nerf_view.h"
#include "raymarch_common.h"
#include "view_math.h"

namespace {

constexpr int NT = 256;                              // threads per workgroup, one per pixel
constexpr int NW = NT / DWG_WAVE;
constexpr int FT = 1024;                             // threads of the finishing workgroup

__global__ __launch_bounds__(NT) void k_view_rays(const float* __restrict__ c2w, const float* __restrict__ intrinsics,
                                                  const float* __restrict__ aabb, uint32_t W, uint32_t N, float min_near,
                                                  float* __restrict__ rays_o, float* __restrict__ rays_d, float* __restrict__ nears,
                                                  float* __restrict__ fars) {
    const uint32_t n = blockIdx.x * NT + threadIdx.x;
    if (n >= N) return;
    const uint32_t row = n / W, col = n - row * W;
    float d[3];
    view_ray(c2w, intrinsics, row, col, d);
    const float o[3] = {c2w[3], c2w[7], c2w[11]};
    rays_o[3 * (size_t)n] = o[0]; rays_o[3 * (size_t)n + 1] = o[1]; rays_o[3 * (size_t)n + 2] = o[2];
    rays_d[3 * (size_t)n] = d[0]; rays_d[3 * (size_t)n + 1] = d[1]; rays_d[3 * (size_t)n + 2] = d[2];
    const Ray r = load_ray(o, d);
    float near, far;
    near_far_ray(r, aabb, min_near, near, far);
    nears[n] = near;
    fars[n] = far;
}

// Sum over the workgroup in a fixed order: butterfly inside each wave, then the waves in order.  Every thread gets the total.
template <int WAVES>
__device__ __forceinline__ double block_sum(double v, double* s_red, int tid) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    __syncthreads();                                   // s_red may still be read from the previous call
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    double t = s_red[0];
    for (int w = 1; w < WAVES; w++) t += s_red[w];
    return t;
}

template <int C>
__device__ __forceinline__ void load_row(const float* __restrict__ p, size_t n, float* v) {
    if (C == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + 4 * n);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) v[c] = p[(size_t)C * n + c];
    }
}

template <int C>
__device__ __forceinline__ void store_row(float* __restrict__ p, size_t n, const float* v) {
    if (C == 4) *reinterpret_cast<float4*>(p + 4 * n) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int c = 0; c < C; c++) p[(size_t)C * n + c] = v[c];
    }
}

template <int C>
__global__ __launch_bounds__(NT) void k_view_compose_forward(uint32_t N, uint32_t channels_out, const float* __restrict__ image_fg,
                                                             const float* __restrict__ weights_sum, const float* __restrict__ bg,
                                                             uint32_t bg_mode, float* __restrict__ image, double* __restrict__ partial) {
    __shared__ double s_red[NW];
    const int tid = threadIdx.x;
    const uint32_t n = blockIdx.x * NT + tid;
    const bool inside = n < N;
    float ws = 0.f;
    if (inside) ws = weights_sum[n];
    if (inside && image) {                           // image == NULL: the sparsity loss alone
        float fg[C], b[C] = {};
        load_row<C>(image_fg, n, fg);
        if (bg_mode == DWG_VIEW_BG_IMAGE) load_row<C>(bg, n, b);
        else if (bg_mode == DWG_VIEW_BG_CONSTANT) {
#pragma unroll
            for (int c = 0; c < C; c++) b[c] = bg[c];
        }
#pragma unroll
        for (int c = 0; c < C; c++)
            if ((uint32_t)c < channels_out) image[(size_t)c * N + n] = bg_mode == DWG_VIEW_BG_NONE ? fg[c] : view_mix(fg[c], ws, b[c]);
    }
    if (!partial) return;                            // uniform over the launch
    double t[3] = {0.0, 0.0, 0.0};
    if (inside) sparsity_terms(ws, t);
    for (int k = 0; k < 3; k++) {
        const double s = block_sum<NW>(t[k], s_red, tid);
        if (tid == 0) partial[3 * (size_t)blockIdx.x + k] = s;
    }
}

// One workgroup.  partial [slots, 3] -> totals [3] (right behind the slots) and the loss.
__global__ __launch_bounds__(FT) void k_view_sparsity_finish(uint32_t slots, double n, double lambda_opacity, double lambda_entropy,
                                                             double lambda_emptiness, double mult, double* __restrict__ partial,
                                                             float* __restrict__ loss) {
    __shared__ double s_red[FT / DWG_WAVE];
    const int tid = threadIdx.x;
    double sums[3];
    for (int k = 0; k < 3; k++) {
        double a = 0.0;
        for (uint32_t i = tid; i < slots; i += FT) a += partial[3 * (size_t)i + k];
        sums[k] = block_sum<FT / DWG_WAVE>(a, s_red, tid);
    }
    if (tid == 0) {
        double* totals = partial + 3 * (size_t)slots;
        totals[0] = sums[0]; totals[1] = sums[1]; totals[2] = sums[2];
        loss[0] = (float)sparsity_loss(sums, n, lambda_opacity, lambda_entropy, lambda_emptiness, mult);
    }
}

template <int C>
__global__ __launch_bounds__(NT) void k_view_compose_backward(uint32_t N, uint32_t channels_out, const float* __restrict__ d_image,
                                                              const float* __restrict__ d_sparsity, const float* __restrict__ weights_sum,
                                                              const float* __restrict__ bg, uint32_t bg_mode, uint32_t detach_ws,
                                                              double lambda_opacity, double lambda_entropy, double lambda_emptiness,
                                                              double mult, const double* __restrict__ totals, float* __restrict__ d_image_fg,
                                                              float* __restrict__ d_weights_sum, float* __restrict__ d_image_bg) {
#pragma clang fp contract(off)
    const uint32_t n = blockIdx.x * NT + threadIdx.x;
    if (n >= N) return;
    float d[C];
#pragma unroll
    for (int c = 0; c < C; c++) d[c] = (d_image && (uint32_t)c < channels_out) ? d_image[(size_t)c * N + n] : 0.f;
    if (d_image_fg) store_row<C>(d_image_fg, n, d);
    const float ws = weights_sum[n];
    double g = 0.0;
    if (bg_mode != DWG_VIEW_BG_NONE && !detach_ws) {
        float b[C];
        if (bg_mode == DWG_VIEW_BG_IMAGE) load_row<C>(bg, n, b);
        else {
#pragma unroll
            for (int c = 0; c < C; c++) b[c] = bg[c];
        }
#pragma unroll
        for (int c = 0; c < C; c++) g -= (double)b[c] * (double)d[c];          // the products of two fp32 are exact
    }
    if (d_sparsity)
        g += (double)d_sparsity[0] * sparsity_derivative(ws, totals[0], (double)N, lambda_opacity, lambda_entropy, lambda_emptiness, mult);
    d_weights_sum[n] = (float)g;
    if (d_image_bg) {
        const float t = 1.f - ws;
        float db[C];
#pragma unroll
        for (int c = 0; c < C; c++) db[c] = t * d[c];
        store_row<C>(d_image_bg, n, db);
    }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

uint32_t slots_of(uint32_t N) { return (N + NT - 1) / NT; }

bool compose_args_ok(uint32_t N, uint32_t C, uint32_t channels_out, const float* bg, uint32_t bg_mode) {
    if (N < 1 || N >= (1u << 31) || (C != 3 && C != 4) || channels_out < 1 || channels_out > C) return false;
    if (bg_mode > DWG_VIEW_BG_IMAGE || (bg_mode == DWG_VIEW_BG_NONE) != (bg == nullptr)) return false;
    return aligned(bg, bg_mode == DWG_VIEW_BG_IMAGE && C == 4 ? 16 : 4);
}

bool lambdas_ok(double a, double b, double c, double m) { return a == a && b == b && c == c && m == m; }

}  // namespace

extern "C" {

int dwg_nerf_view_rays(const float* c2w, const float* intrinsics, const float* aabb, uint32_t H, uint32_t W, float min_near,
                       float* rays_o, float* rays_d, float* nears, float* fars, dwg_stream_t stream) {
    if (H < 1 || W < 1 || H > DWG_VIEW_MAX_SIZE || W > DWG_VIEW_MAX_SIZE || (uint64_t)H * W >= (1ull << 31) || !(min_near == min_near))
        return DWG_E_ARG;
    if (!c2w || !intrinsics || !aabb || !rays_o || !rays_d || !nears || !fars) return DWG_E_ARG;
    if (!aligned(c2w, 4) || !aligned(intrinsics, 4) || !aligned(aabb, 4) || !aligned(rays_o, 4) || !aligned(rays_d, 4) || !aligned(nears, 4) ||
        !aligned(fars, 4))
        return DWG_E_ARG;
    const uint32_t N = H * W;
    DWG_LAUNCH("nerf_view_rays", k_view_rays, dim3(slots_of(N)), dim3(NT), 0, (hipStream_t)stream, c2w, intrinsics, aabb, W, N, min_near,
               rays_o, rays_d, nears, fars);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_nerf_view_compose_workspace_bytes(uint32_t N) {
    return N < 1 || N >= (1u << 31) ? 0 : ((size_t)slots_of(N) + 1) * 3 * sizeof(double);
}

int dwg_nerf_view_compose_forward(uint32_t N, uint32_t C, uint32_t channels_out, const float* image_fg, const float* weights_sum,
                                  const float* bg, uint32_t bg_mode, double lambda_opacity, double lambda_entropy, double lambda_emptiness,
                                  double mult, float* image, float* sparsity_loss, void* workspace, size_t workspace_bytes,
                                  dwg_stream_t stream) {
    if (!compose_args_ok(N, C, channels_out, bg, bg_mode) || !lambdas_ok(lambda_opacity, lambda_entropy, lambda_emptiness, mult)) return DWG_E_ARG;
    if (!weights_sum || (image_fg == nullptr) != (image == nullptr) || !aligned(image_fg, C == 4 ? 16 : 4) || !aligned(weights_sum, 4) ||
        !aligned(image, 4) || !aligned(sparsity_loss, 4))
        return DWG_E_ARG;
    if (!image && (!sparsity_loss || bg)) return DWG_E_ARG;          // nothing to do, or a background without an image
    if (sparsity_loss && (!workspace || !aligned(workspace, 16) || workspace_bytes < dwg_nerf_view_compose_workspace_bytes(N))) return DWG_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    double* partial = sparsity_loss ? reinterpret_cast<double*>(workspace) : nullptr;
    const dim3 grid(slots_of(N));
    if (C == 3)
        DWG_LAUNCH("nerf_view_compose_forward", (k_view_compose_forward<3>), grid, dim3(NT), 0, s, N, channels_out, image_fg, weights_sum, bg,
                   bg_mode, image, partial);
    else
        DWG_LAUNCH("nerf_view_compose_forward", (k_view_compose_forward<4>), grid, dim3(NT), 0, s, N, channels_out, image_fg, weights_sum, bg,
                   bg_mode, image, partial);
    if (partial)
        DWG_LAUNCH("nerf_view_sparsity_finish", k_view_sparsity_finish, dim3(1), dim3(FT), 0, s, slots_of(N), (double)N, lambda_opacity,
                   lambda_entropy, lambda_emptiness, mult, partial, sparsity_loss);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_nerf_view_compose_backward(uint32_t N, uint32_t C, uint32_t channels_out, const float* d_image, const float* d_sparsity,
                                   const float* weights_sum, const float* bg, uint32_t bg_mode, uint32_t detach_ws, double lambda_opacity,
                                   double lambda_entropy, double lambda_emptiness, double mult, const void* workspace,
                                   size_t workspace_bytes, float* d_image_fg, float* d_weights_sum, float* d_image_bg, dwg_stream_t stream) {
    if (!compose_args_ok(N, C, channels_out, bg, bg_mode) || !lambdas_ok(lambda_opacity, lambda_entropy, lambda_emptiness, mult)) return DWG_E_ARG;
    const uintptr_t row_align = C == 4 ? 16 : 4;
    if (!weights_sum || !d_weights_sum || !aligned(weights_sum, 4) || !aligned(d_image, 4) || !aligned(d_sparsity, 4) ||
        !aligned(d_image_fg, row_align) || !aligned(d_weights_sum, 4) || !aligned(d_image_bg, row_align))
        return DWG_E_ARG;
    if (d_image_bg && bg_mode != DWG_VIEW_BG_IMAGE) return DWG_E_ARG;
    if (d_sparsity && (!workspace || !aligned(workspace, 16) || workspace_bytes < dwg_nerf_view_compose_workspace_bytes(N))) return DWG_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const double* totals = d_sparsity ? reinterpret_cast<const double*>(workspace) + 3 * (size_t)slots_of(N) : nullptr;
    const dim3 grid(slots_of(N));
    if (C == 3)
        DWG_LAUNCH("nerf_view_compose_backward", (k_view_compose_backward<3>), grid, dim3(NT), 0, s, N, channels_out, d_image, d_sparsity,
                   weights_sum, bg, bg_mode, detach_ws, lambda_opacity, lambda_entropy, lambda_emptiness, mult, totals, d_image_fg,
                   d_weights_sum, d_image_bg);
    else
        DWG_LAUNCH("nerf_view_compose_backward", (k_view_compose_backward<4>), grid, dim3(NT), 0, s, N, channels_out, d_image, d_sparsity,
                   weights_sum, bg, bg_mode, detach_ws, lambda_opacity, lambda_entropy, lambda_emptiness, mult, totals, d_image_fg,
                   d_weights_sum, d_image_bg);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
