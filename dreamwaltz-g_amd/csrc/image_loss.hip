// image_loss.hip -- the L1 + D-SSIM image reconstruction loss of the nerf2gs loop, forward and backward (include/dwg_image_loss.h,
// boundary B17).
//
//   k_image_loss_forward   one workgroup per (16 x 16 tile, plane): the tile and its 5-pixel halo of x and y are staged in LDS (zeros
//                          outside the image: the reference's zero padding), the five quantities x, y, xx, yy, xy are filtered 11 taps
//                          across into LDS and 11 taps down into registers, the SSIM map is formed, and the workgroup's sums of the map
//                          and of |x - y| go to the workgroup's own slot; with `maps` it also stores the three per-pixel derivatives
//                          the backward filters
//   k_image_loss_finish    one workgroup adds the slots batch item by batch item in a fixed order -> loss, l1, ssim, ssim per item
//   k_image_loss_backward  the same tiling: the adjoint of the zero-padded symmetric filter is the filter, so the three maps are staged
//                          and filtered like the images were, and combined with x, y and sign(x - y) at the pixel
//
// Arithmetic: the images, the window and the stored maps are fp32; the filter sums and the SSIM map are fp64.  sigma = E[xx] - mu mu
// cancels to the rounding of its operands on flat regions (C2 = 9e-4 is all that is left of the denominator there), and the vector fp64
// FMA costs this LDS-bound kernel nothing it would notice, so the cancellation is taken on operands that carry no fp32 rounding.
// Sums over pixels are fp64 in a fixed order (wave butterfly, waves in order, slots in order): no atomics, two runs give the same bits.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_image_loss.h"

namespace {

constexpr int T = DWG_IMAGE_LOSS_TILE, R = DWG_IMAGE_LOSS_WINDOW / 2, WIN = DWG_IMAGE_LOSS_WINDOW;
constexpr int HT = T + 2 * R;                          // 26: tile + halo
constexpr int LD = HT + 1;                             // row pitch of the staged fp32 tiles
constexpr int NT = T * T;                              // 256 threads, one per pixel of the tile
constexpr int NW = NT / DWG_WAVE;
constexpr int FT = 1024;                             // threads of the finishing workgroup
constexpr int64_t MAX_STRIDE = (int64_t)1 << 40;
static_assert(T == 16 && WIN == 11, "the index arithmetic below is written for 16 x 16 tiles and an 11-tap window");

// The reference's window (gaussian_loss.py:17-19): g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) evaluated in double and rounded to fp32
// (torch.Tensor of Python floats), then g / g.sum() in fp32.  These are the eleven resulting fp32 values (bit patterns 3a86cab6
// 3bf8ff01 3d13758c 3ddff87f 3e5a1e1f 3e8832b0 and mirrored), printed from that statement; their fp32 sum is exactly 1.
__device__ constexpr float KW[WIN] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                      0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
constexpr double SSIM_C1 = 0.01 * 0.01, SSIM_C2 = 0.03 * 0.03;      // the reference's Python floats 0.01 ** 2, 0.03 ** 2

struct Img {
    const float* p;
    long long sb, sc, sr, sp;                          // element strides: batch, channel, row, pixel
};

__device__ __forceinline__ size_t img_off(const Img& im, int b, int c, int y, int x) {
    return (size_t)((long long)b * im.sb + (long long)c * im.sc + (long long)y * im.sr + (long long)x * im.sp);
}

// Stage the HT x HT neighbourhood of a tile of one plane, zeros outside the image.
__device__ __forceinline__ void stage(float* __restrict__ s, const float* __restrict__ base, long long sr, long long sp, int x0, int y0,
                                      int H, int W, int tid) {
    for (int i = tid; i < HT * HT; i += NT) {
        const int r = i / HT, q = i - r * HT;
        const int gy = y0 + r, gx = x0 + q;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        s[r * LD + q] = in ? base[(long long)gy * sr + (long long)gx * sp] : 0.f;
    }
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

struct SsimPixel { double ssim, a, b, c2b; };

// The SSIM map at a pixel from the five filtered quantities, and its three derivative maps.  Contraction is off: these are the
// reference's statements (gaussian_loss.py:44-55) with every operation rounded once, so that two identical images give the numerator
// and the denominator the same bits and ssim == 1, loss == 0 exactly, as the reference's composition does.
__device__ __forceinline__ SsimPixel ssim_pixel(const double v[5]) {
#pragma clang fp contract(off)
    const double mu1 = v[0], mu2 = v[1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double sigma1_sq = v[2] - mu1_sq, sigma2_sq = v[3] - mu2_sq, sigma12 = v[4] - mu1_mu2;
    const double A1 = 2.0 * mu1_mu2 + SSIM_C1, A2 = 2.0 * sigma12 + SSIM_C2;
    const double B1 = mu1_sq + mu2_sq + SSIM_C1, B2 = sigma1_sq + sigma2_sq + SSIM_C2;
    SsimPixel o;
    o.ssim = (A1 * A2) / (B1 * B2);
    // S(mu1, sigma1_sq, sigma12) with sigma1_sq = e11 - mu1^2 and sigma12 = e12 - mu1 mu2:
    //   dS/dsigma1_sq = -S / B2,  dS/dsigma12 = 2 A1 / (B1 B2),  dS/dmu1 at fixed sigmas = (2 mu2 A2 - 2 mu1 S B2) / (B1 B2)
    const double inv = 1.0 / (B1 * B2);
    const double d_s1 = -o.ssim / B2, d_s12 = 2.0 * A1 * inv;
    o.a = (2.0 * mu2 * A2 - 2.0 * mu1 * o.ssim * B2) * inv - 2.0 * mu1 * d_s1 - mu2 * d_s12;
    o.b = d_s1;
    // c + 2 b, not c: where x == y both are +-2 / B2 (thousands) and cancel; their sum is formed here, before the fp32 rounding
    o.c2b = d_s12 + 2.0 * d_s1;
    return o;
}

__global__ __launch_bounds__(NT) void k_image_loss_forward(int C, int H, int W, Img x, Img y, float* __restrict__ maps,
                                                           double* __restrict__ partial) {
    __shared__ float s_x[HT * LD], s_y[HT * LD];
    __shared__ double s_h[5][HT][T];
    __shared__ double s_red[NW];
    const int tid = threadIdx.x, tx = tid & (T - 1), ty = tid >> 4;
    const int plane = blockIdx.z, b = plane / C, c = plane - b * C;
    const int x0 = blockIdx.x * T - R, y0 = blockIdx.y * T - R;
    stage(s_x, x.p + img_off(x, b, c, 0, 0), x.sr, x.sp, x0, y0, H, W, tid);
    stage(s_y, y.p + img_off(y, b, c, 0, 0), y.sr, y.sp, x0, y0, H, W, tid);
    __syncthreads();
    // 11 taps across: HT rows x T columns of the five quantities
    for (int i = tid; i < HT * T; i += NT) {
        const int r = i >> 4, q = i & (T - 1);
        double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; k++) {
            const double w = (double)KW[k], xv = (double)s_x[r * LD + q + k], yv = (double)s_y[r * LD + q + k];
            m1 = fma(w, xv, m1); m2 = fma(w, yv, m2);
            e11 = fma(w, xv * xv, e11); e22 = fma(w, yv * yv, e22); e12 = fma(w, xv * yv, e12);      // the products of two fp32 are exact
        }
        s_h[0][r][q] = m1; s_h[1][r][q] = m2; s_h[2][r][q] = e11; s_h[3][r][q] = e22; s_h[4][r][q] = e12;
    }
    __syncthreads();
    // 11 taps down, at this thread's pixel
    double v[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < WIN; k++) a = fma((double)KW[k], s_h[j][ty + k][tx], a);
        v[j] = a;
    }
    const int px = blockIdx.x * T + tx, py = blockIdx.y * T + ty;
    const bool inside = px < W && py < H;
    const SsimPixel sp = ssim_pixel(v);
    const double ssim = sp.ssim;
    const double dxy = (double)s_x[(ty + R) * LD + tx + R] - (double)s_y[(ty + R) * LD + tx + R];
    if (maps && inside) {
        const size_t P = (size_t)gridDim.z * H * W, at = ((size_t)plane * H + py) * W + px;
        maps[at] = (float)sp.a;
        maps[P + at] = (float)sp.b;
        maps[2 * P + at] = (float)sp.c2b;
    }
    const double sum_s = block_sum<NW>(inside ? ssim : 0.0, s_red, tid);
    const double sum_l = block_sum<NW>(inside ? fabs(dxy) : 0.0, s_red, tid);
    if (tid == 0) {
        const size_t slot = ((size_t)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * slot] = sum_s;
        partial[2 * slot + 1] = sum_l;
    }
}

// One workgroup.  The slots of a batch item are contiguous (plane-major); items are added in order.
__global__ __launch_bounds__(FT) void k_image_loss_finish(int B, long long slots_per_item, double pixels_per_item, double lambda,
                                                          const double* __restrict__ partial, float* __restrict__ scalars,
                                                          float* __restrict__ ssim_batch) {
    __shared__ double s_red[FT / DWG_WAVE];
    const int tid = threadIdx.x;
    double tot_s = 0.0, tot_l = 0.0;
    for (int b = 0; b < B; b++) {
        const double* p = partial + 2 * (size_t)b * slots_per_item;
        double a = 0.0, l = 0.0;
        for (long long i = tid; i < slots_per_item; i += FT) { a += p[2 * i]; l += p[2 * i + 1]; }
        a = block_sum<FT / DWG_WAVE>(a, s_red, tid);
        l = block_sum<FT / DWG_WAVE>(l, s_red, tid);
        if (ssim_batch && tid == 0) ssim_batch[b] = (float)(a / pixels_per_item);
        tot_s += a; tot_l += l;
    }
    if (tid == 0) {
        const double n = pixels_per_item * (double)B;
        const double l1 = tot_l / n, ssim = tot_s / n;
        scalars[0] = (float)((1.0 - lambda) * l1 + lambda * (1.0 - ssim));
        scalars[1] = (float)l1;
        scalars[2] = (float)ssim;
    }
}

__global__ __launch_bounds__(NT) void k_image_loss_backward(int C, int H, int W, Img x, Img y, const float* __restrict__ maps,
                                                            const float* __restrict__ grad_out, int per_batch, double coef_ssim,
                                                            double coef_l1, float* __restrict__ grad_x) {
    __shared__ float s_m[3][HT * LD];
    __shared__ double s_h[3][HT][T];
    const int tid = threadIdx.x, tx = tid & (T - 1), ty = tid >> 4;
    const int plane = blockIdx.z, b = plane / C, c = plane - b * C;
    const int px = blockIdx.x * T + tx, py = blockIdx.y * T + ty;
    double f[3] = {0.0, 0.0, 0.0};
    if (maps) {                                        // uniform over the launch
        const size_t P = (size_t)gridDim.z * H * W;
        for (int j = 0; j < 3; j++)
            stage(s_m[j], maps + j * P + (size_t)plane * H * W, W, 1, blockIdx.x * T - R, blockIdx.y * T - R, H, W, tid);
        __syncthreads();
        for (int i = tid; i < HT * T; i += NT) {
            const int r = i >> 4, q = i & (T - 1);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; k++) {
                const double w = (double)KW[k];
                a0 = fma(w, (double)s_m[0][r * LD + q + k], a0);
                a1 = fma(w, (double)s_m[1][r * LD + q + k], a1);
                a2 = fma(w, (double)s_m[2][r * LD + q + k], a2);
            }
            s_h[0][r][q] = a0; s_h[1][r][q] = a1; s_h[2][r][q] = a2;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; k++) a = fma((double)KW[k], s_h[j][ty + k][tx], a);
            f[j] = a;
        }
    }
    if (px >= W || py >= H) return;
    const size_t at = img_off(x, b, c, py, px);
    const float xv = x.p[at], yv = y.p[img_off(y, b, c, py, px)];
    const double d = (double)xv - (double)yv;
    const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);          // torch's abs backward: sign(0) = 0
    // rounded to fp32 BEFORE the upstream gradient multiplies it: a gradient of 3 gives exactly three times the gradient of 1
    const float t = (float)(coef_ssim * (f[0] + 2.0 * d * f[1] + (double)yv * f[2]) + coef_l1 * sgn);
    grad_x[at] = grad_out[per_batch ? b : 0] * t;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

bool sizes_ok(int32_t B, int32_t C, int32_t H, int32_t W) {
    return B >= 1 && C >= 1 && H >= 1 && W >= 1 && H <= DWG_IMAGE_LOSS_MAX_SIZE && W <= DWG_IMAGE_LOSS_MAX_SIZE &&
           (int64_t)B * C <= DWG_IMAGE_LOSS_MAX_PLANES;
}

// A stride is read only along a dimension longer than 1.  `lo` = 1 for an image that is also written in this layout, 0 for a read-only one.
bool strides_ok(const int32_t n[4], const int64_t s[4], int64_t lo) {
    for (int i = 0; i < 4; i++)
        if (n[i] > 1 && (s[i] < lo || s[i] > MAX_STRIDE)) return false;
    return true;
}

Img make_img(const float* p, const int32_t n[4], const int64_t s[4]) {
    Img im;
    im.p = p;
    im.sb = n[0] > 1 ? s[0] : 0; im.sc = n[1] > 1 ? s[1] : 0; im.sr = n[2] > 1 ? s[2] : 0; im.sp = n[3] > 1 ? s[3] : 0;
    return im;
}

size_t slots(int32_t B, int32_t C, int32_t H, int32_t W) { return (size_t)B * C * dwg_cdiv(H, T) * dwg_cdiv(W, T); }

}  // namespace

extern "C" {

size_t dwg_image_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    return sizes_ok(B, C, H, W) ? slots(B, C, H, W) * 2 * sizeof(double) : 0;
}

int dwg_image_loss_forward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t window_size, float lambda_dssim,
                           const float* x, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                           const float* y, int64_t y_batch_stride, int64_t y_channel_stride, int64_t y_row_stride, int64_t y_pixel_stride,
                           float* scalars, float* ssim_batch, float* maps, void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    if (!sizes_ok(B, C, H, W) || window_size != DWG_IMAGE_LOSS_WINDOW || !(lambda_dssim >= 0.f && lambda_dssim <= 1.f)) return DWG_E_ARG;
    const int32_t n[4] = {B, C, H, W};
    const int64_t xs[4] = {x_batch_stride, x_channel_stride, x_row_stride, x_pixel_stride};
    const int64_t ys[4] = {y_batch_stride, y_channel_stride, y_row_stride, y_pixel_stride};
    if (!x || !y || !scalars || !aligned(x, 4) || !aligned(y, 4) || !aligned(scalars, 4) || !aligned(ssim_batch, 4) || !aligned(maps, 4))
        return DWG_E_ARG;
    if (!strides_ok(n, xs, 1) || !strides_ok(n, ys, 0)) return DWG_E_ARG;
    if (!workspace || !aligned(workspace, 16) || workspace_bytes < dwg_image_loss_workspace_bytes(B, C, H, W)) return DWG_E_ARG;
    double* partial = reinterpret_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(dwg_cdiv(W, T), dwg_cdiv(H, T), B * C);
    DWG_LAUNCH("image_loss_forward", k_image_loss_forward, grid, dim3(NT), 0, s, C, H, W, make_img(x, n, xs), make_img(y, n, ys), maps, partial);
    DWG_LAUNCH("image_loss_finish", k_image_loss_finish, dim3(1), dim3(FT), 0, s, B, (long long)(slots(B, C, H, W) / B),
               (double)C * H * W, (double)lambda_dssim, (const double*)partial, scalars, ssim_batch);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_image_loss_backward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t window_size, double coef_ssim, double coef_l1,
                            const float* x, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                            const float* y, int64_t y_batch_stride, int64_t y_channel_stride, int64_t y_row_stride, int64_t y_pixel_stride,
                            const float* maps, const float* grad_out, int32_t grad_per_batch, float* grad_x, dwg_stream_t stream) {
    if (!sizes_ok(B, C, H, W) || window_size != DWG_IMAGE_LOSS_WINDOW || !(coef_ssim == coef_ssim) || !(coef_l1 == coef_l1)) return DWG_E_ARG;
    const int32_t n[4] = {B, C, H, W};
    const int64_t xs[4] = {x_batch_stride, x_channel_stride, x_row_stride, x_pixel_stride};
    const int64_t ys[4] = {y_batch_stride, y_channel_stride, y_row_stride, y_pixel_stride};
    if (!x || !y || !grad_out || !grad_x || !aligned(x, 4) || !aligned(y, 4) || !aligned(grad_out, 4) || !aligned(grad_x, 4) || !aligned(maps, 4))
        return DWG_E_ARG;
    if (!maps && coef_ssim != 0.0) return DWG_E_ARG;
    if (!strides_ok(n, xs, 1) || !strides_ok(n, ys, 0)) return DWG_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(dwg_cdiv(W, T), dwg_cdiv(H, T), B * C);
    DWG_LAUNCH("image_loss_backward", k_image_loss_backward, grid, dim3(NT), 0, s, C, H, W, make_img(x, n, xs), make_img(y, n, ys),
               coef_ssim != 0.0 ? maps : (const float*)nullptr, grad_out, (int)(grad_per_batch != 0), coef_ssim, coef_l1, grad_x);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
