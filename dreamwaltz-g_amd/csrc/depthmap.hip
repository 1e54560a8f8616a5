// depthmap.hip -- per-pixel ray cast of the posed body mesh (condition type 'depth_raw') and the NeRF pretrain loss over it
// (include/dwg_depthmap.h, boundary B9).
//
// The mesh moves every step, so no hierarchy is built.  Three launches per map:
//   k_depth_tri_setup   one thread per triangle: the per-triangle half of Moeller-Trumbore (everything that does not depend on the
//                       ray's direction -- all rays share one origin) as a 13-double record, and the triangle's screen box
//   k_depth_cast        one workgroup per 16 x 16 pixel tile: walks ALL triangle boxes (8 bytes each, coalesced), compacts the ones that
//                       overlap the tile into LDS by ballot IN TRIANGLE ORDER, stages their records in LDS, and every pixel then
//                       intersects only the listed triangles whose box holds it -- in fp64, in ascending triangle order, strict
//                       `t < best`: the lower index wins a tie.  The list is a fixed-size LDS ring that is drained whenever it could
//                       overflow: no size anywhere depends on the data
//   k_depth_image       the numpy-float32 statements of export_depth
// and two for the loss: per-workgroup partial sums in a fixed order + one finishing workgroup; the backward is one element-wise launch.
#include <hip/hip_fp16.h>

#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_depthmap.h"

namespace {

constexpr int TILE = 16, NT = 256, CAP = 512, BATCH = 128, REC = 13;
constexpr size_t HEADER_BYTES = 64;                    // word 0: bits of min(1 / t), word 1: bits of max(1 / t)
constexpr unsigned INF_BITS = 0x7f800000u;
constexpr double Z_EPS = 1e-6;                         // a vertex this close to the camera plane: the box is the whole image
// A pixel can be hit only if its centre lies inside the triangle's projection.  The projection here (fp64) and the ray the pixel
// really casts (its direction rounded to fp32: 6e-8 of fx, 1e-3 pixel at the largest image) differ by far less than this margin.
constexpr double BOX_MARGIN = 1.0 / 64;

struct Box { short x0, y0, x1, y1; };                  // inclusive pixel ranges; empty: x0 > x1

struct Cam { double R[9], T[3], fx, fy, cx, cy; };

__device__ __forceinline__ Cam load_cam(const float* __restrict__ ext, const float* __restrict__ intr) {
    Cam c;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) c.R[3 * i + j] = (double)ext[4 * i + j];
        c.T[i] = (double)ext[4 * i + 3];
    }
    c.fx = (double)intr[0]; c.fy = (double)intr[4]; c.cx = (double)intr[2]; c.cy = (double)intr[5];
    return c;
}

// The statements below are written out product by product with contraction off, so that they are the float64 statements a numpy
// caller writes (no fused multiply-add): the record of a triangle and the float32 ray of a pixel are then the same bits on both sides.
__device__ __forceinline__ void ray_origin(const Cam& c, double o[3]) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; i++) o[i] = -((c.R[i] * c.T[0] + c.R[3 + i] * c.T[1]) + c.R[6 + i] * c.T[2]);       // -R^T T
}
__device__ __forceinline__ void pixel_ray(const Cam& c, int x, int y, double d[3]) {
#pragma clang fp contract(off)
    const double dx = ((double)x + 0.5 - c.cx) / c.fx, dy = ((double)y + 0.5 - c.cy) / c.fy;
    for (int i = 0; i < 3; i++) d[i] = (double)(float)((c.R[i] * dx + c.R[3 + i] * dy) + c.R[6 + i]);          // R^T (dx, dy, 1) -> fp32
}
__device__ __forceinline__ void tri_record(const double o[3], const double v0[3], const double v1[3], const double v2[3], double* r) {
#pragma clang fp contract(off)
    double e1[3], e2[3], tv[3];
    for (int i = 0; i < 3; i++) { e1[i] = v1[i] - v0[i]; e2[i] = v2[i] - v0[i]; tv[i] = o[i] - v0[i]; }
    const double q[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    for (int i = 0; i < 3; i++) { r[i] = e1[i]; r[3 + i] = e2[i]; r[6 + i] = tv[i]; r[9 + i] = q[i]; }
    r[12] = (q[0] * e2[0] + q[1] * e2[1]) + q[2] * e2[2];
}

__device__ __forceinline__ short clamp_px(double v) { return (short)(v < -30000.0 ? -30000.0 : (v > 30000.0 ? 30000.0 : v)); }

// ---------------------------------------------------------------------------------------------------------------------
// per triangle: record + screen box (and the reset of the image's min / max words)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_depth_tri_setup(int H, int W, const float* __restrict__ ext, const float* __restrict__ intr, int V,
                                                        const float* __restrict__ verts, int F, const int* __restrict__ tris,
                                                        Box* __restrict__ boxes, double* __restrict__ recs, unsigned* __restrict__ minmax) {
    const int f = blockIdx.x * NT + threadIdx.x;
    if (f == 0) { minmax[0] = INF_BITS; minmax[1] = 0u; }
    if (f >= F) return;
    const Box empty = {1, 1, 0, 0};
    const int i0 = tris[3 * (size_t)f], i1 = tris[3 * (size_t)f + 1], i2 = tris[3 * (size_t)f + 2];
    double* r = recs + (size_t)f * REC;
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) {
        for (int i = 0; i < REC; i++) r[i] = 0.0;              // det = 0: never a hit, even if listed
        boxes[f] = empty;
        return;
    }
    const Cam c = load_cam(ext, intr);
    double o[3], v[3][3];
    ray_origin(c, o);
    const int idx[3] = {i0, i1, i2};
    for (int k = 0; k < 3; k++)
        for (int i = 0; i < 3; i++) v[k][i] = (double)verts[3 * (size_t)idx[k] + i];
    tri_record(o, v[0], v[1], v[2], r);
    // camera-space vertices -> box of the pixels whose centre can lie inside the projection
    bool finite = true, any_front = false, any_near = false;
    double lox = INFINITY, hix = -INFINITY, loy = INFINITY, hiy = -INFINITY;
    for (int k = 0; k < 3; k++) {
        double p[3];
        for (int i = 0; i < 3; i++) p[i] = c.R[3 * i] * v[k][0] + c.R[3 * i + 1] * v[k][1] + c.R[3 * i + 2] * v[k][2] + c.T[i];
        finite = finite && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
        if (p[2] > 0.0) any_front = true;
        if (!(p[2] > Z_EPS)) { any_near = true; continue; }
        const double px = c.fx * p[0] / p[2] + c.cx - 0.5, py = c.fy * p[1] / p[2] + c.cy - 0.5;      // in pixel-index units
        lox = fmin(lox, px); hix = fmax(hix, px); loy = fmin(loy, py); hiy = fmax(hiy, py);
    }
    Box b;
    if (!finite || !any_front) b = empty;                      // t is the camera-space z of the hit: t > 0 is impossible
    else if (any_near || !(isfinite(lox) && isfinite(hix) && isfinite(loy) && isfinite(hiy))) b = Box{0, 0, (short)(W - 1), (short)(H - 1)};
    else {
        b = Box{clamp_px(ceil(lox - BOX_MARGIN)), clamp_px(ceil(loy - BOX_MARGIN)), clamp_px(floor(hix + BOX_MARGIN)), clamp_px(floor(hiy + BOX_MARGIN))};
        if (b.x1 < b.x0 || b.y1 < b.y0 || b.x1 < 0 || b.y1 < 0 || b.x0 >= W || b.y0 >= H) b = empty;      // no pixel centre inside
    }
    boxes[f] = b;
}

// ---------------------------------------------------------------------------------------------------------------------
// per pixel tile: list the overlapping triangles, intersect
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_depth_cast(int H, int W, const float* __restrict__ ext, const float* __restrict__ intr, int F,
                                                   const Box* __restrict__ boxes, const double* __restrict__ recs,
                                                   float* __restrict__ t_hit, float* __restrict__ normals, unsigned* __restrict__ minmax) {
    __shared__ int s_list[CAP];
    __shared__ int s_wave[2][NT / DWG_WAVE];
    __shared__ double s_rec[BATCH * REC];
    __shared__ Box s_box[BATCH];
    __shared__ unsigned s_lo[NT / DWG_WAVE], s_hi[NT / DWG_WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int tx1 = min(tx0 + TILE, W) - 1, ty1 = min(ty0 + TILE, H) - 1;
    const int px = tx0 + (tid & (TILE - 1)), py = ty0 + (tid >> 4);
    const bool inside = px < W && py < H;
    const Cam c = load_cam(ext, intr);
    double d[3];
    pixel_ray(c, px, py, d);
    double best = INFINITY;
    int best_f = -1;

    // every listed triangle, BATCH records at a time; called by all threads with a uniform count
    auto drain = [&](int count) {
        for (int b0 = 0; b0 < count; b0 += BATCH) {
            const int n = min(BATCH, count - b0);
            __syncthreads();                                   // the list is complete / the previous batch has been read
            for (int k = tid; k < n * REC; k += NT) s_rec[k] = recs[(size_t)s_list[b0 + k / REC] * REC + (k % REC)];
            if (tid < n) s_box[tid] = boxes[s_list[b0 + tid]];
            __syncthreads();
            for (int j = 0; j < n; j++) {
                const Box bx = s_box[j];
                if (px < bx.x0 || px > bx.x1 || py < bx.y0 || py > bx.y1) continue;
                const double* r = s_rec + j * REC;             // e1, e2, tv = o - v0, q = tv x e1, q . e2
                const double p0 = d[1] * r[5] - d[2] * r[4], p1 = d[2] * r[3] - d[0] * r[5], p2 = d[0] * r[4] - d[1] * r[3];
                const double det = r[0] * p0 + r[1] * p1 + r[2] * p2;
                if (!(fabs(det) > 1e-12)) continue;
                const double un = r[6] * p0 + r[7] * p1 + r[8] * p2, wn = r[9] * d[0] + r[10] * d[1] + r[11] * d[2];
                // u, w and t below are un, wn and r[12] times 1 / det: where one of them is clearly negative (the product with det
                // below -1e-200 and |det| < 1e50, so the quotient cannot round to -0) the division is not needed to reject
                if (fabs(det) < 1e50 && (un * det < -1e-200 || wn * det < -1e-200 || r[12] * det < -1e-200)) continue;
                const double inv = 1.0 / det;
                const double u = un * inv;
                const double w = wn * inv;
                const double t = r[12] * inv;
                if (u >= 0.0 && w >= 0.0 && u + w <= 1.0 && t > 0.0 && t < best) { best = t; best_f = s_list[b0 + j]; }
            }
        }
        __syncthreads();                                       // the list may be overwritten
    };

    int count = 0, par = 0;
    for (int base = 0; base < F; base += NT) {
        const int f = base + tid;
        bool ov = false;
        if (f < F) {
            const Box bx = boxes[f];
            ov = bx.x0 <= tx1 && bx.x1 >= tx0 && bx.y0 <= ty1 && bx.y1 >= ty0;
        }
        const unsigned long long m = __ballot(ov);
        if (lane == 0) s_wave[par][wave] = __popcll(m);
        __syncthreads();
        int off = count, total = 0;
        for (int w = 0; w < NT / DWG_WAVE; w++) {
            const int n = s_wave[par][w];
            if (w < wave) off += n;
            total += n;
        }
        if (ov) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = f;        // off + rank < count + total <= CAP
        count += total;
        par ^= 1;
        if (count > CAP - NT) { drain(count); count = 0; }
    }
    drain(count);

    const float tf = (float)best;
    if (inside) {
        const size_t pix = (size_t)py * W + px;
        t_hit[pix] = tf;
        if (normals) {
            float n[3] = {0.f, 0.f, 0.f};
            if (best_f >= 0) {
                const double* r = recs + (size_t)best_f * REC;
                const double c0 = r[1] * r[5] - r[2] * r[4], c1 = r[2] * r[3] - r[0] * r[5], c2 = r[0] * r[4] - r[1] * r[3];
                const double len = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
                n[0] = (float)(c0 / len); n[1] = (float)(c1 / len); n[2] = (float)(c2 / len);
            }
            normals[3 * pix] = n[0]; normals[3 * pix + 1] = n[1]; normals[3 * pix + 2] = n[2];
        }
    }
    if (minmax) {
        // 1 / t is a non-negative float: its bit pattern orders like the value, and integer min / max do not depend on the order
        const float dinv = 1.0f / tf;
        unsigned lo = inside ? __float_as_uint(dinv) : INF_BITS, hi = inside ? __float_as_uint(dinv) : 0u;
        for (int s = 32; s > 0; s >>= 1) {
            lo = min(lo, (unsigned)__shfl_xor((int)lo, s));
            hi = max(hi, (unsigned)__shfl_xor((int)hi, s));
        }
        if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NT / DWG_WAVE; w++) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
            // one pair of atomics per tile, and none where the tile cannot move the extremum (a stale read only costs an atomic)
            if (lo < __atomic_load_n(minmax, __ATOMIC_RELAXED)) atomicMin(minmax, lo);
            if (hi > __atomic_load_n(minmax + 1, __ATOMIC_RELAXED)) atomicMax(minmax + 1, hi);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the image
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_depth_minmax(long long P, const float* __restrict__ t_hit, unsigned* __restrict__ minmax) {
    __shared__ unsigned s_lo[1024], s_hi[1024];
    const int tid = threadIdx.x;
    unsigned lo = INF_BITS, hi = 0u;
    for (long long i = tid; i < P; i += 1024) {
        const unsigned b = __float_as_uint(1.0f / t_hit[i]);
        lo = min(lo, b); hi = max(hi, b);
    }
    s_lo[tid] = lo; s_hi[tid] = hi;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) { s_lo[tid] = min(s_lo[tid], s_lo[tid + s]); s_hi[tid] = max(s_hi[tid], s_hi[tid + s]); }
        __syncthreads();
    }
    if (tid == 0) { minmax[0] = s_lo[0]; minmax[1] = s_hi[0]; }
}

__global__ __launch_bounds__(NT) void k_depth_image(long long P, const float* __restrict__ t_hit, const unsigned* __restrict__ minmax,
                                                    unsigned char* __restrict__ out_u8, float* __restrict__ out_chw) {
#pragma clang fp contract(off)
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= P) return;
    const float lo = __uint_as_float(minmax[0]);
    const float top = __uint_as_float(minmax[1]) - lo;         // max(d - lo) = max(d) - lo: the rounded subtraction is monotonic
    float d = 1.0f / t_hit[pix];                               // depth = 1.0 / depth
    d = d - lo;                                                // depth -= np.min(depth)
    int byte = 0;
    if (top > 0.f) {
        d = d / top;                                           // depth /= np.max(depth): IEEE division, hipcc's default (no fast-math here)
        const float v = d * 255.0f;
        byte = v >= 0.f ? (v < 256.f ? (int)v : 255) : 0;      // np.uint8 truncates; NaN (a NaN in a map given from outside) -> 0
    }
    if (out_u8) { out_u8[3 * pix] = (unsigned char)byte; out_u8[3 * pix + 1] = (unsigned char)byte; out_u8[3 * pix + 2] = (unsigned char)byte; }
    if (out_chw) { const float v = (float)byte / 255.f; out_chw[pix] = v; out_chw[P + pix] = v; out_chw[2 * P + pix] = v; }
}

// ---------------------------------------------------------------------------------------------------------------------
// the pretrain loss
// ---------------------------------------------------------------------------------------------------------------------
constexpr int LOSS_MAX_BLOCKS = 256, LOSS_PER_BLOCK = NT * 8;

__device__ __forceinline__ float ld(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld(const __half* p, size_t i) { return __half2float(p[i]); }
__device__ __forceinline__ void st(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st(__half* p, size_t i, float v) { p[i] = __float2half(v); }
__device__ __forceinline__ float clean(float v) { return isfinite(v) ? v : 0.f; }        // nan_to_num(nan=0, posinf=0, neginf=0)

// The differences and squares are fp32 (what the reference's fp32 mse computes per element); the SUMS are carried in fp64 in a fixed
// order -- thread-strided, LDS tree, then the finishing workgroup over the per-workgroup partials -- so the result is the correctly
// summed fp32 terms and does not depend on the launch.
template <typename T>
__global__ __launch_bounds__(NT) void k_pretrain_loss_partial(long long N, const T* __restrict__ depth, const T* __restrict__ ws,
                                                              const float* __restrict__ smpl, double* __restrict__ partial) {
    __shared__ double s_a[NT], s_b[NT];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (long long i = (long long)blockIdx.x * NT + tid; i < N; i += (long long)gridDim.x * NT) {
        const float sd = clean(smpl[i]);
        const float mask = sd > 1e-6f ? 1.f : 0.f;
        const float dm = ld(ws, (size_t)i) - mask, dd = ld(depth, (size_t)i) - sd;
        a += (double)(dm * dm); b += (double)(dd * dd);
    }
    s_a[tid] = a; s_b[tid] = b;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) { s_a[tid] += s_a[tid + s]; s_b[tid] += s_b[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { partial[2 * blockIdx.x] = s_a[0]; partial[2 * blockIdx.x + 1] = s_b[0]; }
}

__global__ __launch_bounds__(LOSS_MAX_BLOCKS) void k_pretrain_loss_finish(int blocks, long long N, const double* __restrict__ partial,
                                                                          float* __restrict__ loss) {
    __shared__ double s_a[LOSS_MAX_BLOCKS], s_b[LOSS_MAX_BLOCKS];
    const int tid = threadIdx.x;
    s_a[tid] = tid < blocks ? partial[2 * tid] : 0.0;
    s_b[tid] = tid < blocks ? partial[2 * tid + 1] : 0.0;
    __syncthreads();
    for (int s = LOSS_MAX_BLOCKS / 2; s > 0; s >>= 1) {
        if (tid < s) { s_a[tid] += s_a[tid + s]; s_b[tid] += s_b[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) loss[0] = (float)(s_a[0] / (double)N + s_b[0] / (double)N);
}

template <typename T>
__global__ __launch_bounds__(NT) void k_pretrain_loss_backward(long long N, const T* __restrict__ depth, const T* __restrict__ ws,
                                                               const float* __restrict__ smpl, const float* __restrict__ grad_loss,
                                                               T* __restrict__ g_depth, T* __restrict__ g_ws) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const float k = 2.f * grad_loss[0] / (float)N;             // 2 g is exact; three roundings per gradient: this quotient, the difference, the product
    const float sd = clean(smpl[i]);
    const float mask = sd > 1e-6f ? 1.f : 0.f;
    if (g_depth) st(g_depth, (size_t)i, (ld(depth, (size_t)i) - sd) * k);
    if (g_ws) st(g_ws, (size_t)i, (ld(ws, (size_t)i) - mask) * k);
}

int loss_blocks(long long N) {
    const long long b = (N + LOSS_PER_BLOCK - 1) / LOSS_PER_BLOCK;
    return (int)(b < 1 ? 1 : (b > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : b));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
size_t boxes_bytes(int F) { return dwg_align_up((size_t)F * sizeof(Box), 16); }

}  // namespace

extern "C" {

size_t dwg_depthmap_workspace_bytes(int32_t H, int32_t W, int32_t F) {
    if (H <= 0 || W <= 0 || F < 0) return 0;
    return HEADER_BYTES + boxes_bytes(F) + (size_t)F * REC * sizeof(double);
}

int dwg_depthmap_cast(int32_t H, int32_t W, const float* extrinsic, const float* intrinsics, int32_t V, const float* vertices, int32_t F,
                      const int32_t* triangles, float* t_hit, float* normals, int32_t want_minmax, void* workspace, size_t workspace_bytes,
                      dwg_stream_t stream) {
    if (H <= 0 || W <= 0 || H > DWG_DEPTHMAP_MAX_SIZE || W > DWG_DEPTHMAP_MAX_SIZE || V < 0 || F < 0) return DWG_E_ARG;
    if (!extrinsic || !intrinsics || !t_hit) return DWG_E_ARG;
    if (F > 0 && (V <= 0 || !vertices || !triangles)) return DWG_E_ARG;
    if (!workspace || !aligned16(workspace)) return DWG_E_ARG;
    if (workspace_bytes < dwg_depthmap_workspace_bytes(H, W, F)) return DWG_E_ARG;
    unsigned* minmax = reinterpret_cast<unsigned*>(workspace);
    Box* boxes = reinterpret_cast<Box*>(reinterpret_cast<char*>(workspace) + HEADER_BYTES);
    double* recs = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + HEADER_BYTES + boxes_bytes(F));
    hipStream_t s = (hipStream_t)stream;
    DWG_LAUNCH("depth_tri_setup", k_depth_tri_setup, dim3(F > 0 ? dwg_cdiv(F, NT) : 1), dim3(NT), 0, s, H, W, extrinsic, intrinsics, V, vertices,
               F, triangles, boxes, recs, minmax);
    DWG_LAUNCH("depth_cast", k_depth_cast, dim3(dwg_cdiv(W, TILE), dwg_cdiv(H, TILE)), dim3(NT), 0, s, H, W, extrinsic, intrinsics, F,
               (const Box*)boxes, (const double*)recs, t_hit, normals, want_minmax ? minmax : (unsigned*)nullptr);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_depthmap_image(int32_t H, int32_t W, const float* t_hit, int32_t minmax_from_cast, uint8_t* out_u8, float* out_chw,
                       void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    if (H <= 0 || W <= 0 || H > DWG_DEPTHMAP_MAX_SIZE || W > DWG_DEPTHMAP_MAX_SIZE || !t_hit || (!out_u8 && !out_chw)) return DWG_E_ARG;
    if (!workspace || !aligned16(workspace) || workspace_bytes < HEADER_BYTES) return DWG_E_ARG;
    unsigned* minmax = reinterpret_cast<unsigned*>(workspace);
    const long long P = (long long)H * W;
    hipStream_t s = (hipStream_t)stream;
    if (!minmax_from_cast) DWG_LAUNCH("depth_minmax", k_depth_minmax, dim3(1), dim3(1024), 0, s, P, t_hit, minmax);
    DWG_LAUNCH("depth_image", k_depth_image, dim3((unsigned)((P + NT - 1) / NT)), dim3(NT), 0, s, P, t_hit, (const unsigned*)minmax, out_u8,
               out_chw);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_pretrain_loss_workspace_bytes(int64_t N) { return N > 0 ? (size_t)loss_blocks(N) * 2 * sizeof(double) : 0; }

int dwg_pretrain_loss_forward(int32_t dtype, int64_t N, const void* render_depth, const void* render_ws, const float* smpl_depth,
                              float* loss, void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    if (N <= 0 || N > (int64_t)0x7fffffff || (dtype != DWG_DTYPE_F32 && dtype != DWG_DTYPE_F16)) return DWG_E_ARG;
    if (!render_depth || !render_ws || !smpl_depth || !loss) return DWG_E_ARG;
    if (!workspace || !aligned16(workspace) || workspace_bytes < dwg_pretrain_loss_workspace_bytes(N)) return DWG_E_ARG;
    const int blocks = loss_blocks(N);
    double* partial = reinterpret_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == DWG_DTYPE_F32)
        DWG_LAUNCH("pretrain_loss_partial", k_pretrain_loss_partial<float>, dim3(blocks), dim3(NT), 0, s, (long long)N,
                   (const float*)render_depth, (const float*)render_ws, smpl_depth, partial);
    else
        DWG_LAUNCH("pretrain_loss_partial", k_pretrain_loss_partial<__half>, dim3(blocks), dim3(NT), 0, s, (long long)N,
                   (const __half*)render_depth, (const __half*)render_ws, smpl_depth, partial);
    DWG_LAUNCH("pretrain_loss_finish", k_pretrain_loss_finish, dim3(1), dim3(LOSS_MAX_BLOCKS), 0, s, blocks, (long long)N,
               (const double*)partial, loss);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_pretrain_loss_backward(int32_t dtype, int64_t N, const void* render_depth, const void* render_ws, const float* smpl_depth,
                               const float* grad_loss, void* grad_depth, void* grad_ws, dwg_stream_t stream) {
    if (N <= 0 || N > (int64_t)0x7fffffff || (dtype != DWG_DTYPE_F32 && dtype != DWG_DTYPE_F16)) return DWG_E_ARG;
    if (!render_depth || !render_ws || !smpl_depth || !grad_loss || (!grad_depth && !grad_ws)) return DWG_E_ARG;
    const unsigned grid = (unsigned)((N + NT - 1) / NT);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == DWG_DTYPE_F32)
        DWG_LAUNCH("pretrain_loss_backward", k_pretrain_loss_backward<float>, dim3(grid), dim3(NT), 0, s, (long long)N,
                   (const float*)render_depth, (const float*)render_ws, smpl_depth, grad_loss, (float*)grad_depth, (float*)grad_ws);
    else
        DWG_LAUNCH("pretrain_loss_backward", k_pretrain_loss_backward<__half>, dim3(grid), dim3(NT), 0, s, (long long)N,
                   (const __half*)render_depth, (const __half*)render_ws, smpl_depth, grad_loss, (__half*)grad_depth, (__half*)grad_ws);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
