// nerf_field.hip -- the fused NeRF field of stage I (boundary B7): grid encoding -> sigma_net -> density / albedo epilogue.
//
// Native restatement of _NeRFNetwork.common_forward / local_geometry_forward (core/nerf/nerf_model.py:268-295) for the grid
// backbone.  A workgroup (4 waves) takes 64 points at a time:
//   1. the 64 x L grid lookups (gridenc_common.h, the same code as gridenc.hip) fill an LDS tile enc[64][2L];
//   2. each wave runs its 16 rows through the layers on the matrix cores (16x16 output blocks, weights resident in LDS),
//      every layer's output going back to LDS; nothing between x and (sigma, albedo) is written to HBM;
//   3. one thread per point applies the density activation / prior and the albedo sigmoid and writes the outputs.
// The backward recomputes 1-2 per tile, then walks the layers backwards in LDS: dZ_l -> dW_l (MFMA over the tile's 64 points,
// accumulated in registers across the workgroup's tiles), db_l, dZ_{l-1} = (dZ_l W_l) * relu'.  The encoding gradient goes to
// HBM in the [points, 2L] layout that the slab-binned table gradient of gridenc.hip reads.  The per-workgroup weight-gradient
// partials are summed by a second kernel in workgroup order; no float atomics anywhere, so the gradients are bit-reproducible.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_gridenc.h"
#include "../../include/dwg_nerf.h"
#include "../../include/dwg_nerf_render.h"
#include "../../include/dwg_occupancy.h"
#include "../../include/dwg_pointcloud.h"
#include "fd_normal.h"
#include "gridenc_common.h"
#include "morton.h"
#include "occupancy_common.h"
#include "pointcloud_index.h"
#include "raymarch_common.h"

namespace {

constexpr int NF_TILE = 64;                 // points per workgroup tile (4 waves x 16 rows)
constexpr int NF_MAXS = 13;                 // weight-gradient blocks per wave: (16 + 16 + 16 + 4) 16x16 blocks of 4 layers / 4 waves
constexpr int NF_BWD_WG = 1024;             // workgroups of the backward (4 per CU): the number of weight-gradient partials
constexpr uint64_t NF_CHUNK = 1ull << 20;   // points per backward chunk (bounds the d_enc and table-gradient workspace)
constexpr int NR_SLOTS = 256;               // inference render: ray slots per workgroup, one per thread
constexpr int NR_ITERS = 32;                // inference render: marching iterations (refills included) of a thread per round
constexpr uint32_t NR_DEFAULT_WG = 512;     // inference render: persistent workgroups when the caller names no number

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct NfP {
    GridP g;
    const float2* table;                    // embeddings [offsets[L]] (C = 2)
    const int* offsets;
    float bound, inv2b;
    uint32_t nl, W;                         // layers, out_dim
    uint32_t K[4], N[4], KP[4], NP[4];      // true and padded (multiple of 16) in / out widths per layer
    const float* w[4];
    const float* b[4];
    uint32_t act, prior, sig, raw;
    const float* sigma_scale;
    // LDS layout, in elements of the operand type: weights [NP][KP + pad], activations [64][width + pad]
    uint32_t woff[4], wst[4];
    uint32_t aoff[5], ast[5];               // 0: enc, 1..nl-1: hidden outputs, nl: last layer's output
    uint32_t bias_byte_off;                 // float bias[4][64] after the operand-typed part
    // weight-gradient partial layout (floats): W_l [N][K], then b_l [N]; the last slot is sigma_scale's
    uint32_t pw[4], pb[4], P;
    uint32_t bb[5];                         // prefix over layers of the 16x16 weight-gradient blocks: wave w owns blocks w, w + 4, ...
    uint32_t sumN;                          // biases: thread t < sumN owns one
};

template <typename T> struct Mm;
template <> struct Mm<_Float16> {
    static constexpr int KS = 16, NJ = 4;
    typedef _Float16 frag __attribute__((ext_vector_type(4)));
    __device__ static f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
    __device__ static void set(frag& f, int j, _Float16 v) { f[j] = v; }
};
template <> struct Mm<float> {
    static constexpr int KS = 4, NJ = 1;
    typedef float frag;
    __device__ static f32x4 mma(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    __device__ static void set(frag& f, int, float v) { f = v; }
};

// One 16x16 output block of D = A B over K (multiple of the MFMA's k step) from LDS: A(i, k) = A[i * sa + k * ska] with
// ska == 1 when AK (contiguous along k), B(k, j) = B[k * sbk + j * sb] with sbk == 1 when BK.  Lane l holds D[4 (l >> 4) + v][l & 15].
template <typename T, bool AK, bool BK>
__device__ __forceinline__ f32x4 mma_block(const T* A, uint32_t sa, uint32_t ska, const T* B, uint32_t sbk, uint32_t sb, uint32_t K, f32x4 acc) {
    typedef Mm<T> M;
    const uint32_t lane = threadIdx.x & 63u, r = lane & 15u, q = lane >> 4;
    for (uint32_t k0 = 0; k0 < K; k0 += M::KS) {
        const uint32_t k = k0 + M::NJ * q;
        typename M::frag a, b;
        if (AK) a = *reinterpret_cast<const typename M::frag*>(A + r * sa + k);
        else {
#pragma unroll
            for (int j = 0; j < M::NJ; j++) M::set(a, j, A[r * sa + (k + j) * ska]);
        }
        if (BK) b = *reinterpret_cast<const typename M::frag*>(B + k + r * sb);
        else {
#pragma unroll
            for (int j = 0; j < M::NJ; j++) M::set(b, j, B[(k + j) * sbk + r * sb]);
        }
        acc = M::mma(a, b, acc);
    }
    return acc;
}

__device__ __forceinline__ float nf_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }      // F.softplus, beta 1, threshold 20
__device__ __forceinline__ float nf_softplus_bwd(float g, float x) { if (x > 20.f) return g; const float z = expf(x); return g * z / (z + 1.f); }

__device__ __forceinline__ float nf_prior(const NfP& p, float x0, float x1, float x2) {
    if (p.prior == 0) return 0.f;
    const float d = x0 * x0 + x1 * x1 + x2 * x2;                            // nerf_model.py:43
    if (p.prior == 1) return 5.f * expf(-d / 0.08f);                        // gaussian: peak 5, std 0.2
    return 10.f * (1.f - sqrtf(d) / 0.5f);                                  // sqrt: blob density 10, radius 0.5
}

// weights (rounded to T) and biases into LDS; padding zero
template <typename T>
__device__ void load_weights(const NfP& p, T* lds, float* bias) {
    for (uint32_t l = 0; l < p.nl; l++) {
        T* w = lds + p.woff[l];
        const uint32_t n_el = p.NP[l] * p.wst[l];
        for (uint32_t e = threadIdx.x; e < n_el; e += 256) {
            const uint32_t n = e / p.wst[l], k = e - n * p.wst[l];
            w[e] = (T)((n < p.N[l] && k < p.K[l]) ? p.w[l][n * p.K[l] + k] : 0.f);
        }
        for (uint32_t n = threadIdx.x; n < 64; n += 256) bias[l * 64 + n] = n < p.N[l] ? p.b[l][n] : 0.f;
    }
    // the encoding's padding columns are never written by a lookup: zero them once
    T* e = lds + p.aoff[0];
    for (uint32_t i = threadIdx.x; i < NF_TILE * p.ast[0]; i += 256) e[i] = (T)0.f;
}


// Where a tile's x comes from: component i (0 .. 3 NF_TILE - 1) of the tile that starts at point p0.
struct XPoints {                            // x [M, 3] in memory
    const float* __restrict__ x;
    __device__ __forceinline__ float operator()(uint64_t p0, uint32_t i) const { return x[p0 * 3 + i]; }
};
struct XLattice {                           // the lattice of dwg_pointcloud.h: flat index -> chunk -> (ix, iy, iz) -> the axis tables
    PcLattice l;
    const float* __restrict__ ax;
    const float* __restrict__ ay;
    const float* __restrict__ az;
    __device__ __forceinline__ float operator()(uint64_t p0, uint32_t i) const {
        const uint32_t pt = i / 3u, k = i - 3u * pt;
        uint32_t ix, iy, iz;
        pc_lattice_decode(l, (uint32_t)p0 + pt, ix, iy, iz);
        return k == 0 ? ax[ix] : k == 1 ? ay[iy] : az[iz];
    }
};

struct XOccupancy {                         // the jittered cell points of dwg_occupancy.h: flat cell index -> (cascade, ix, iy, iz) -> occ_point
    OccLattice l;
    __device__ __forceinline__ float operator()(uint64_t p0, uint32_t i) const {
        const uint32_t pt = i / 3u;
        return occ_point(l, (uint32_t)p0 + pt, i - 3u * pt);
    }
};

struct XPointsFd {                          // x [M, 3] in memory (pass 0) or its shift pass - 1 of the finite-difference normal, made in registers
    const float* __restrict__ x;
    uint32_t pass;
    float eps, bound;
    __device__ __forceinline__ float operator()(uint64_t p0, uint32_t i) const {
        const float v = x[p0 * 3 + i];
        return pass == 0u ? v : fd_shift(v, i % 3u, pass - 1u, eps, bound);
    }
};
struct XStaged {                            // the pending samples of the inference render, compacted into LDS in slot order
    const float* s;
    __device__ __forceinline__ float operator()(uint64_t p0, uint32_t i) const { return s[(uint32_t)p0 * 3u + i]; }
};
struct XStagedFd {                          // those samples (pass 0) or their shift pass - 1 of the finite-difference normal (fd_normal.h)
    const float* s;
    uint32_t pass;
    float eps, bound;
    __device__ __forceinline__ float operator()(uint64_t p0, uint32_t i) const {
        const float v = s[(uint32_t)p0 * 3u + i];
        return pass == 0u ? v : fd_shift(v, i % 3u, pass - 1u, eps, bound);
    }
};

// x of the tile -> sx, the encoder's (x + bound) / (2 bound) -> sxn, the 64 x L lookups -> enc, then the layers; points at or past
// `mend` are encoded from x = 0 (their outputs are never stored).  Ends with a barrier: every layer output is in LDS.
template <typename T, typename XS>
__device__ void field_tile(const NfP& p, const XS& x, uint64_t mend, uint64_t p0, T* lds, const float* bias, float* sx, float* sxn) {
    for (uint32_t i = threadIdx.x; i < NF_TILE * 3; i += 256) {
        const float v = p0 + i / 3 < mend ? x(p0, i) : 0.f;
        sx[i] = v;
        sxn[i] = (v + p.bound) * p.inv2b;       // torch evaluates the division by the Python scalar 2 bound as a product with its inverse
    }
    __syncthreads();
    T* enc = lds + p.aoff[0];
    const uint32_t L = p.g.L, est = p.ast[0];
    for (uint32_t t = threadIdx.x; t < NF_TILE * L; t += 256) {
        const uint32_t pt = t / L, level = t - pt * L;
        Cell c = locate(p.g, p.offsets, level, sxn[3 * pt], sxn[3 * pt + 1], sxn[3 * pt + 2]);
        float r0 = 0.f, r1 = 0.f;
        if (!c.oob) {
            const float2* g = p.table + (uint32_t)p.offsets[level];
            float2 v[8];
#pragma unroll
            for (int idx = 0; idx < 8; idx++) {
                uint32_t gx = c.g[0] + (idx & 1), gy = c.g[1] + ((idx >> 1) & 1), gz = c.g[2] + ((idx >> 2) & 1);
                v[idx] = g[grid_index(p.g.gridtype, p.g.align_corners, c.hsize, c.res, gx, gy, gz) >> 1];
                if (sizeof(T) == 2) { v[idx].x = (float)(_Float16)v[idx].x; v[idx].y = (float)(_Float16)v[idx].y; }   // the fp16 table (grid.py:47-48)
            }
#pragma unroll
            for (int idx = 0; idx < 8; idx++) {
                float w = ((idx & 1) ? c.w[0] : 1.f - c.w[0]) * ((idx & 2) ? c.w[1] : 1.f - c.w[1]) * ((idx & 4) ? c.w[2] : 1.f - c.w[2]);
                r0 += w * v[idx].x; r1 += w * v[idx].y;
            }
        }
        enc[pt * est + 2 * level] = (T)r0;
        enc[pt * est + 2 * level + 1] = (T)r1;
    }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, r = lane & 15u, q = lane >> 4;
    for (uint32_t l = 0; l < p.nl; l++) {
        const T* X = lds + p.aoff[l] + wave * 16u * p.ast[l];
        T* Y = lds + p.aoff[l + 1] + wave * 16u * p.ast[l + 1];
        const T* Wl = lds + p.woff[l];
        const bool relu = l + 1 < p.nl;
        for (uint32_t cb = 0; cb < p.NP[l] / 16u; cb++) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = mma_block<T, true, true>(X, p.ast[l], 1u, Wl + cb * 16u * p.wst[l], 1u, p.wst[l], p.KP[l], acc);
            const uint32_t col = cb * 16u + r;
            const float bv = bias[l * 64u + col];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                float y = acc[v] + bv;
                if (relu && y < 0.f) y = 0.f;
                Y[(4u * q + v) * p.ast[l + 1] + col] = (T)y;
            }
        }
        __syncthreads();
    }
}

template <typename T>
__device__ __forceinline__ void lds_carve(const NfP& p, unsigned char* smem, T*& lds, float*& bias, float*& sx, float*& sxn, float*& red) {
    lds = reinterpret_cast<T*>(smem);
    bias = reinterpret_cast<float*>(smem + p.bias_byte_off);
    sx = bias + 256;
    sxn = sx + NF_TILE * 3;
    red = sxn + NF_TILE * 3;
}

// density of a point from the last layer's first output h0 (es = exp(sigma_scale), read by `scaling` only)
__device__ __forceinline__ float nf_sigma(const NfP& p, float h0, const float* x, float es) {
    if (p.raw) return h0;
    const float xv = h0 + nf_prior(p, x[0], x[1], x[2]);
    return p.act == 0 ? expf(xv) : p.act == 1 ? nf_softplus(xv) : nf_softplus(xv * es - 1.f);
}

template <typename T>
__global__ __launch_bounds__(256) void k_nf_fwd(NfP p, const float* __restrict__ x, uint64_t M, uint64_t ntiles, float* __restrict__ sigma,
                                                T* __restrict__ albedo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds; float *bias, *sx, *sxn, *red;
    lds_carve(p, smem, lds, bias, sx, sxn, red);
    load_weights(p, lds, bias);
    const float es = p.act == 2 ? expf(*p.sigma_scale) : 0.f;
    const uint32_t W = p.W;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t p0 = tile * NF_TILE;
        field_tile(p, XPoints{x}, M, p0, lds, bias, sx, sxn);
        const uint32_t t = threadIdx.x;
        if (t < NF_TILE && p0 + t < M) {
            const uint64_t pt = p0 + t;
            const T* o = lds + p.aoff[p.nl] + t * p.ast[p.nl];
            sigma[pt] = nf_sigma(p, (float)o[0], sx + 3 * t, es);
            T* a = albedo + pt * (W - 1u);
            for (uint32_t c = 1; c < W; c++) {
                float v = (float)o[c];
                if (p.sig) v = 1.f / (1.f + expf(-v));
                a[c - 1] = (T)v;
            }
        }
        __syncthreads();
    }
}

// The field at x and the density at its six shifts (dwg_nerf_field_forward_fd): k_nf_fwd's tile loop with seven passes of field_tile per
// tile through XPointsFd.  Pass 0 stores what k_nf_fwd stores; pass s stores the density of shift s - 1, with the prior taken at the
// shifted point (sx holds it), into sigma_fd [M, 6].  The shifted points exist in registers and LDS only.
template <typename T>
__global__ __launch_bounds__(256) void k_nf_fwd_fd(NfP p, const float* __restrict__ x, uint64_t M, uint64_t ntiles, float eps, float* __restrict__ sigma,
                                                   T* __restrict__ albedo, float* __restrict__ sigma_fd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds; float *bias, *sx, *sxn, *red;
    lds_carve(p, smem, lds, bias, sx, sxn, red);
    load_weights(p, lds, bias);
    const float es = p.act == 2 ? expf(*p.sigma_scale) : 0.f;
    const uint32_t W = p.W;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t p0 = tile * NF_TILE;
        for (uint32_t pass = 0; pass < 7u; ++pass) {
            field_tile(p, XPointsFd{x, pass, eps, p.bound}, M, p0, lds, bias, sx, sxn);
            const uint32_t t = threadIdx.x;
            if (t < NF_TILE && p0 + t < M) {
                const uint64_t pt = p0 + t;
                const T* o = lds + p.aoff[p.nl] + t * p.ast[p.nl];
                const float sg = nf_sigma(p, (float)o[0], sx + 3 * t, es);
                if (pass == 0u) {
                    sigma[pt] = sg;
                    T* a = albedo + pt * (W - 1u);
                    for (uint32_t c = 1; c < W; c++) {
                        float v = (float)o[c];
                        if (p.sig) v = 1.f / (1.f + expf(-v));
                        a[c - 1] = (T)v;
                    }
                } else sigma_fd[pt * 6u + (pass - 1u)] = sg;
            }
            __syncthreads();
        }
    }
}

// Density only, at the points of a lattice (dwg_pc_lattice_sigma): k_nf_fwd with the tile's x staged from the axis tables and without the
// albedo.  minmax [DWG_PC_MINMAX_PAIRS][2]: this workgroup's (min, max) of the densities it wrote (NaN skipped), and (+inf, -inf) in the
// pairs no workgroup owns (gridDim.x <= DWG_PC_MINMAX_PAIRS).
template <typename T>
__global__ __launch_bounds__(256) void k_nf_lattice(NfP p, XLattice x, uint64_t M, uint64_t ntiles, float* __restrict__ sigma,
                                                    float* __restrict__ minmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds; float *bias, *sx, *sxn, *red;
    lds_carve(p, smem, lds, bias, sx, sxn, red);
    load_weights(p, lds, bias);
    const float es = p.act == 2 ? expf(*p.sigma_scale) : 0.f;
    float lo = INFINITY, hi = -INFINITY;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t p0 = tile * NF_TILE;
        field_tile(p, x, M, p0, lds, bias, sx, sxn);
        const uint32_t t = threadIdx.x;
        if (t < NF_TILE && p0 + t < M) {
            const T* o = lds + p.aoff[p.nl] + t * p.ast[p.nl];
            const float s = nf_sigma(p, (float)o[0], sx + 3 * t, es);
            sigma[p0 + t] = s;
            lo = fminf(lo, s); hi = fmaxf(hi, s);
        }
        __syncthreads();
    }
    // the tile loop ended with a barrier: sx / sxn are free
    if (threadIdx.x < NF_TILE) { sx[threadIdx.x] = lo; sxn[threadIdx.x] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < NF_TILE; i++) { lo = fminf(lo, sx[i]); hi = fmaxf(hi, sxn[i]); }
        minmax[2u * blockIdx.x] = lo; minmax[2u * blockIdx.x + 1u] = hi;
        for (uint32_t j = blockIdx.x + gridDim.x; j < (uint32_t)DWG_PC_MINMAX_PAIRS; j += gridDim.x) { minmax[2u * j] = INFINITY; minmax[2u * j + 1u] = -INFINITY; }
    }
}

// Density only, at the jittered cell points of the occupancy grid (dwg_occ_lattice_sigma): k_nf_lattice with that source and the store
// at the cell's Morton index.  M = C H^3 is a multiple of NF_TILE, so a tile is whole and lies in one cascade.
template <typename T>
__global__ __launch_bounds__(256) void k_nf_occupancy(NfP p, XOccupancy x, uint64_t M, uint64_t ntiles, uint32_t blob, float* __restrict__ tmp_grid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds; float *bias, *sx, *sxn, *red;
    lds_carve(p, smem, lds, bias, sx, sxn, red);
    load_weights(p, lds, bias);
    const float es = p.act == 2 ? expf(*p.sigma_scale) : 0.f;
    const uint32_t lg3 = 3u * x.l.lg;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t p0 = tile * NF_TILE;
        field_tile(p, x, M, p0, lds, bias, sx, sxn);
        const uint32_t t = threadIdx.x;
        if (t < NF_TILE && p0 + t < M) {
            const T* o = lds + p.aoff[p.nl] + t * p.ast[p.nl];
            float s = nf_sigma(p, (float)o[0], sx + 3 * t, es);
            if (blob) s += occ_blob(sx[3 * t], sx[3 * t + 1], sx[3 * t + 2]);
            const uint32_t g = (uint32_t)p0 + t, c = g >> lg3;
            uint32_t ix, iy, iz;
            occ_decode(x.l.lg, g & ((1u << lg3) - 1u), ix, iy, iz);
            tmp_grid[((size_t)c << lg3) + morton3d(ix, iy, iz)] = s;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// inference render (boundary B14): march, field and composite of a ray from near to its end in one persistent launch
// ---------------------------------------------------------------------------------------------------------------------------------
struct RenderP {
    const float* rays_o;
    const float* rays_d;
    const float* nears;
    const float* fars;
    uint32_t N, max_steps;
    float T_thresh;
    uint32_t binarize;
    float* weights_sum;
    float* depth;
    float* image;
    int32_t* counts;
};

struct ShadeP {                             // the shaded render (boundary B15): forward() of nerf_model.py:86-103 per sample
    uint32_t shading;                       // shade_math.h: DWG_SHADE_NORMAL, _TEXTURELESS, _LAMBERTIAN
    const float* light_d;                   // [3]; read for the last two
    float ratio, one_minus_ratio;           // ambient_ratio and the Python scalar 1 - ambient_ratio as torch hands it to the kernel
    float eps, bound;                       // normal()'s epsilon; the clamp of the shifted points
};

// The colour of a sample from its density gradient g (shade_math.h: fd_normalize) and albedo: forward()'s statements for shading
// 'normal', 'textureless' and 'lambertian', without FP contraction.  l = -light_d.  shade_math.h's shade_color holds the same three
// statements for the training kernels and the host build.  Calling it here with the constant NC gives the same bits, but the compiler
// then schedules k_nf_render_shaded differently and the f32 render measured 2 - 5 % slower on an MI355X; with this copy the kernel's
// instructions are the ones it had.
template <int NC>
__device__ __forceinline__ void shade_sample(const ShadeP& sh, float lx, float ly, float lz, float g0, float g1, float g2, const float (&alb)[NC],
                                             float (&rgb)[NC]) {
#pragma clang fp contract(off)
    float n[3];
    fd_normalize(g0, g1, g2, n);
#pragma unroll
    for (int k = 0; k < NC; ++k) rgb[k] = 0.f;
    if (sh.shading == DWG_SHADE_NORMAL) {
        rgb[0] = (n[0] + 1.f) / 2.f; rgb[1] = (n[1] + 1.f) / 2.f; rgb[2] = (n[2] + 1.f) / 2.f;
        return;
    }
    const float dot = (n[0] * lx + n[1] * ly) + n[2] * lz;
    const float lam = sh.ratio + sh.one_minus_ratio * (dot < 0.f ? 0.f : dot);      // clamp(min=0): NaN stays NaN
    if (sh.shading == DWG_SHADE_TEXTURELESS) { rgb[0] = lam; rgb[1] = lam; rgb[2] = lam; }
    else {
#pragma unroll
        for (int k = 0; k < NC; ++k) rgb[k] = alb[k] * lam;
    }
}

// One ray per thread (NR_SLOTS slots).  A round: every thread marches its ray to the next sample (taking the workgroup's next ray from
// the LDS cursor when its slot is free), the pending samples are compacted into `stage` in slot order, field_tile runs on every 64 of
// them and each owner composites its sample from its row of the last layer's output.  Workgroup w of G owns the 64-ray blocks w, w + G,
// ...: the cursor counts through them.  Which slot or round a ray lands in changes no arithmetic of the ray.
//
// SHADED (k_nf_render_shaded): field_tile runs seven times on every 64 pending samples, through XStagedFd: the samples, then their six
// shifts.  The owner keeps the sample's density and albedo from pass 0, one density of each +- pair and the three components of the
// gradient in named registers, and shades (shade_sample) before it composites (raymarch_common.h: composite_sample).  NC is the width of the image: with four channels the colour of
// 'normal' and 'textureless' is the reference's zero pad in the fourth.
template <typename T, int NC, bool SHADED>
__device__ __forceinline__ void nf_render(const NfP& p, const MarchP& m, const RenderP& q, const ShadeP& sh, unsigned char* smem) {
    T* lds; float *bias, *sx, *sxn, *red;
    lds_carve(p, smem, lds, bias, sx, sxn, red);
    float* stage = red + NF_TILE;                                               // [NR_SLOTS][3]
    uint32_t* ctl = reinterpret_cast<uint32_t*>(stage + NR_SLOTS * 3);          // [0..3] pending per wave, [4..7] unfinished threads per wave, [8] cursor
    load_weights(p, lds, bias);
    if (threadIdx.x == 0) ctl[8] = 0u;
    __syncthreads();
    const float es = p.act == 2 ? expf(*p.sigma_scale) : 0.f;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool binarize = q.binarize != 0;
    float lx = 0.f, ly = 0.f, lz = 0.f;                                         // -l
    if constexpr (SHADED) {
        if (sh.shading >= DWG_SHADE_TEXTURELESS) { lx = -sh.light_d[0]; ly = -sh.light_d[1]; lz = -sh.light_d[2]; }
    }
    Ray ray = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float t = 0.f, far = 0.f, ws = 0.f, d = 0.f, col[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) col[k] = 0.f;
    uint32_t idx = 0, cnt = 0;
    bool have = false, done = false;                                            // a ray in the slot; no ray left for this thread
    auto finish = [&]() {
        q.weights_sum[idx] = ws;
        q.depth[idx] = d;
#pragma unroll
        for (int k = 0; k < NC; ++k) q.image[(size_t)NC * idx + k] = col[k];
        if (q.counts) q.counts[idx] = (int32_t)cnt;
        have = false;
    };
    for (;;) {
        bool pend = false;
        float cx = 0.f, cy = 0.f, cz = 0.f, dt = 0.f;
        for (int it = 0; it < NR_ITERS && !done; ++it) {
            if (!have) {
                const uint32_t j = atomicAdd(&ctl[8], 1u);
                const uint64_t n = ((uint64_t)(j >> 6) * gridDim.x + blockIdx.x) * 64u + (j & 63u);
                if (n >= q.N) { done = true; break; }
                idx = (uint32_t)n;
                ray = load_ray(q.rays_o + 3 * (size_t)idx, q.rays_d + 3 * (size_t)idx);
                far = q.fars[idx];
                t = start_t(m, q.nears[idx], 0.f);
                ws = 0.f; d = 0.f; cnt = 0u;
#pragma unroll
                for (int k = 0; k < NC; ++k) col[k] = 0.f;
                have = true;
            }
            if (!(t < far)) { finish(); continue; }
            if (march_iter(m, ray, t, cx, cy, cz, dt)) { pend = true; break; }
        }
        const unsigned long long bp = __ballot(pend), bl = __ballot(!done);
        if (lane == 0) { ctl[wave] = (uint32_t)__popcll(bp); ctl[4 + wave] = (uint32_t)__popcll(bl); }
        __syncthreads();
        uint32_t pos = 0, total = 0, unfinished = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t c = ctl[i];
            if (i < wave) pos += c;
            total += c;
            unfinished += ctl[4 + i];
        }
        if (total == 0u && unfinished == 0u) break;
        pos += (uint32_t)__popcll(bp & ((1ull << lane) - 1ull));
        if (pend) { stage[3 * pos] = cx; stage[3 * pos + 1] = cy; stage[3 * pos + 2] = cz; }
        __syncthreads();
        for (uint32_t base = 0; base < total; base += NF_TILE) {
            if constexpr (SHADED) {
                const bool mine = pend && pos - base < (uint32_t)NF_TILE;       // pos < base wraps past NF_TILE
                const uint32_t r = pos - base;
                float sigma = 0.f, s_pos = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f, alb[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) alb[k] = 0.f;
                for (uint32_t pass = 0; pass < 7u; ++pass) {
                    field_tile(p, XStagedFd{stage, pass, sh.eps, sh.bound}, (uint64_t)total, (uint64_t)base, lds, bias, sx, sxn);
                    if (mine) {
                        const T* o = lds + p.aoff[p.nl] + r * p.ast[p.nl];
                        const float sg = nf_sigma(p, (float)o[0], sx + 3 * r, es);     // sx holds the shifted point: the prior is taken there
                        if (pass == 0u) {
                            sigma = sg;
                            if (sh.shading == DWG_SHADE_LAMBERTIAN) {
#pragma unroll
                                for (int k = 0; k < NC; ++k) {
                                    float v = (float)o[1 + k];
                                    if (p.sig) v = 1.f / (1.f + expf(-v));
                                    alb[k] = (float)(T)v;
                                }
                            }
                        } else if (pass & 1u) s_pos = sg;
                        else {
                            const float g = fd_gradient(s_pos, sg, sh.eps);
                            if (pass == 2u) g0 = g; else if (pass == 4u) g1 = g; else g2 = g;
                        }
                    }
                    __syncthreads();
                }
                if (mine) {
                    float rgb[NC];
                    shade_sample<NC>(sh, lx, ly, lz, g0, g1, g2, alb, rgb);
                    const bool stop = composite_sample<NC>(sigma, rgb, t, dt, q.T_thresh, binarize, ws, d, col);
                    ++cnt;
                    if (stop || cnt >= q.max_steps) finish();
                }
                continue;
            }
            field_tile(p, XStaged{stage}, (uint64_t)total, (uint64_t)base, lds, bias, sx, sxn);
            if (pend && pos - base < (uint32_t)NF_TILE) {                       // pos < base wraps past NF_TILE
                const uint32_t r = pos - base;
                const T* o = lds + p.aoff[p.nl] + r * p.ast[p.nl];
                const float sigma = nf_sigma(p, (float)o[0], sx + 3 * r, es);
                float rgb[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    float v = (float)o[1 + k];
                    if (p.sig) v = 1.f / (1.f + expf(-v));
                    rgb[k] = (float)(T)v;                                       // k_nf_fwd stores the albedo in T; the loop widens that tensor
                }
                const bool stop = composite_sample<NC>(sigma, rgb, t, dt, q.T_thresh, binarize, ws, d, col);
                ++cnt;
                if (stop || cnt >= q.max_steps) finish();
            }
            __syncthreads();
        }
    }
}

template <typename T, int NC>
__global__ __launch_bounds__(256) void k_nf_render(NfP p, MarchP m, RenderP q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    nf_render<T, NC, false>(p, m, q, ShadeP{}, smem);
}

template <typename T, int NC>
__global__ __launch_bounds__(256) void k_nf_render_shaded(NfP p, MarchP m, RenderP q, ShadeP sh) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    nf_render<T, NC, true>(p, m, q, sh, smem);
}

// One chunk [m0, m0 + n) of the backward.  partial: [gridDim.x][P] floats, overwritten when `first`, else added to.  XS: where the
// points come from (XPoints, or XPointsFd for a pass of dwg_nerf_field_backward_fd); the density gradient of point pt is
// dsigma[pt * ds_stride].  ALB false: the albedo has no gradient (the shifted points of the normal), the columns 1.. of d(last layer
// output) are zero without a buffer of zeros being read.
template <typename T, typename XS, bool ALB>
__global__ __launch_bounds__(256) void k_nf_bwd(NfP p, XS x, uint64_t m0, uint64_t n, const float* __restrict__ dsigma, uint32_t ds_stride,
                                                const T* __restrict__ dalbedo, float* __restrict__ d_enc, float* __restrict__ xn_out,
                                                float* __restrict__ partial, int first, int want_w) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds; float *bias, *sx, *sxn, *red;
    lds_carve(p, smem, lds, bias, sx, sxn, red);
    load_weights(p, lds, bias);
    const float es = p.act == 2 ? expf(*p.sigma_scale) : 0.f;
    const uint32_t W = p.W, nl = p.nl;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, r = lane & 15u, q = lane >> 4;
    const uint64_t mend = m0 + n, ntiles = (n + NF_TILE - 1) / NF_TILE;
    // the bias this thread owns
    uint32_t bl = 4, bn = 0;
    {
        uint32_t base = 0;
        for (uint32_t l = 0; l < nl; l++) {
            if (threadIdx.x >= base && threadIdx.x < base + p.N[l]) { bl = l; bn = threadIdx.x - base; }
            base += p.N[l];
        }
    }
    f32x4 acc[NF_MAXS];
#pragma unroll
    for (int s = 0; s < NF_MAXS; s++) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float acc_b = 0.f, acc_s = 0.f;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t p0 = m0 + tile * NF_TILE;
        field_tile(p, x, mend, p0, lds, bias, sx, sxn);
        // d(last layer output), rounded to the operand type where autograd hands the reference an fp16 gradient
        if (threadIdx.x < NF_TILE) {
            const uint32_t t = threadIdx.x;
            const uint64_t pt = p0 + t;
            const bool valid = pt < mend;
            T* o = lds + p.aoff[nl] + t * p.ast[nl];
            float d[16];
#pragma unroll
            for (int c = 0; c < 16; c++) d[c] = 0.f;
            if (valid) {
                if (xn_out) { for (int k = 0; k < 3; k++) xn_out[(pt - m0) * 3 + k] = sxn[3 * t + k]; }
                const float g = dsigma[pt * ds_stride];
                const float h0 = (float)o[0];
                if (p.raw) d[0] = g;
                else {
                    const float xv = h0 + nf_prior(p, sx[3 * t], sx[3 * t + 1], sx[3 * t + 2]);
                    if (p.act == 0) d[0] = g * expf(fminf(fmaxf(xv, -15.f), 15.f));         // trunc_exp's backward (nerf_utils.py:189-191)
                    else if (p.act == 1) d[0] = nf_softplus_bwd(g, xv);
                    else { const float dy = nf_softplus_bwd(g, xv * es - 1.f); d[0] = dy * es; acc_s += dy * xv; }
                }
                if constexpr (ALB) {
                    const T* da = dalbedo + pt * (W - 1u);
#pragma unroll
                    for (int c = 1; c < 16; c++) {
                        if ((uint32_t)c < W) {
                            float gv = (float)da[c - 1];
                            if (p.sig) { const float a = (float)(T)(1.f / (1.f + expf(-(float)o[c]))); gv = gv * (1.f - a) * a; }
                            d[c] = gv;
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 16; c++) o[c] = (T)d[c];
        }
        __syncthreads();
        for (int l = (int)nl - 1; l >= 0; l--) {
            const T* Z = lds + p.aoff[l + 1];
            const uint32_t zs = p.ast[l + 1];
            T* X = lds + p.aoff[l];
            const uint32_t xs = p.ast[l];
            if (want_w) {
                const uint32_t nkb = p.KP[l] / 16u, b0 = p.bb[l], b1 = p.bb[l + 1];
#pragma unroll
                for (int s = 0; s < NF_MAXS; s++) {
                    const uint32_t gb = wave + 4u * s;
                    if (gb >= b0 && gb < b1) {
                        const uint32_t loc = gb - b0, nb = loc / nkb, kb = loc - nb * nkb;
                        // dW[n][k] += sum_p dZ[p][n] X[p][k]
                        acc[s] = mma_block<T, false, false>(Z + nb * 16u, 1u, zs, X + kb * 16u, xs, 1u, (uint32_t)NF_TILE, acc[s]);
                    }
                }
                if (bl == (uint32_t)l) {
                    float sb = 0.f;
                    for (uint32_t pp = 0; pp < NF_TILE; pp++) sb += (float)Z[pp * zs + bn];
                    acc_b += sb;
                }
            }
            const uint32_t ncb = p.KP[l] / 16u;
            const T* Wl = lds + p.woff[l];
            f32x4 dx[4];
#pragma unroll
            for (int cb = 0; cb < 4; cb++) {
                dx[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
                // dX[i][j] = sum_n dZ[i][n] W[n][j]
                if ((uint32_t)cb < ncb && (l > 0 || d_enc))
                    dx[cb] = mma_block<T, true, false>(Z + wave * 16u * zs, zs, 1u, Wl + cb * 16u, p.wst[l], 1u, p.NP[l], dx[cb]);
            }
            if (l > 0) {
                __syncthreads();            // every wave's weight-gradient reads of X are done
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    if ((uint32_t)cb >= ncb) continue;
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        T* e = X + (wave * 16u + 4u * q + v) * xs + cb * 16u + r;
                        *e = (T)((float)*e > 0.f ? dx[cb][v] : 0.f);          // relu' from the layer's (rounded) output
                    }
                }
            } else if (d_enc) {
                const uint32_t K0 = p.K[0];
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    if ((uint32_t)cb >= ncb) continue;
                    const uint32_t col = cb * 16u + r;
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        const uint64_t pt = p0 + wave * 16u + 4u * q + v;
                        if (pt < mend && col < K0) d_enc[(pt - m0) * K0 + col] = dx[cb][v];
                    }
                }
            }
            __syncthreads();
        }
    }
    if (!want_w) return;
    float* P = partial + (size_t)blockIdx.x * p.P;
#pragma unroll
    for (int s = 0; s < NF_MAXS; s++) {
        const uint32_t gb = wave + 4u * s;
        if (gb >= p.bb[nl]) continue;
        uint32_t l = 0;
        while (gb >= p.bb[l + 1]) l++;
        const uint32_t nkb = p.KP[l] / 16u, loc = gb - p.bb[l], nb = loc / nkb, kb = loc - nb * nkb;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint32_t nn = nb * 16u + 4u * q + v, k = kb * 16u + r;
            if (nn < p.N[l] && k < p.K[l]) {
                float* e = P + p.pw[l] + nn * p.K[l] + k;
                *e = (first ? 0.f : *e) + acc[s][v];
            }
        }
    }
    if (bl < nl) { float* e = P + p.pb[bl] + bn; *e = (first ? 0.f : *e) + acc_b; }
    if (threadIdx.x < NF_TILE) red[threadIdx.x] = acc_s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < NF_TILE; i++) s += red[i];
        float* e = P + p.P - 1u;
        *e = (first ? 0.f : *e) + s;
    }
}

// sum of the G partials of every parameter, in workgroup order
__global__ __launch_bounds__(256) void k_nf_reduce(NfP p, uint32_t G, const float* __restrict__ partial, dwg_nerf_field_grads gr) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.P) return;
    float* dst = nullptr;
    if (i == p.P - 1u) dst = gr.sigma_scale;
    else {
        for (uint32_t l = 0; l < p.nl; l++) {
            if (i >= p.pw[l] && i < p.pb[l]) dst = gr.weight[l] ? gr.weight[l] + (i - p.pw[l]) : nullptr;
            else if (i >= p.pb[l] && i < p.pb[l] + p.N[l]) dst = gr.bias[l] ? gr.bias[l] + (i - p.pb[l]) : nullptr;
        }
    }
    if (!dst) return;
    float s = 0.f;
    for (uint32_t g = 0; g < G; g++) s += partial[(size_t)g * p.P + i];
    if (i == p.P - 1u) s *= expf(*p.sigma_scale);           // d/d sigma_scale of exp(sigma_scale), after the sum (as autograd orders it)
    *dst = gr.accumulate ? *dst + s : s;
}

int make_params(const dwg_nerf_field_desc* d, NfP& p, size_t& lds_bytes) {
    if (!d) return DWG_E_ARG;
    const uint32_t L = d->num_levels, nl = d->num_layers;
    if (L == 0 || L > 32 || nl == 0 || nl > DWG_NERF_MAX_LAYERS || d->out_dim < 2 || d->out_dim > 16) return DWG_E_ARG;
    if (nl > 1 && (d->hidden == 0 || d->hidden > 64)) return DWG_E_ARG;
    if (d->precision > 1 || d->density_activation > 2 || d->density_prior > 2 || d->gridtype > 1 || d->interp > 1) return DWG_E_ARG;
    if (!(d->bound > 0.f) || !d->embeddings || !d->offsets) return DWG_E_ARG;
    if (d->density_activation == 2 && !d->sigma_scale) return DWG_E_ARG;
    for (uint32_t l = 0; l < nl; l++) if (!d->weight[l] || !d->bias[l]) return DWG_E_ARG;
    p = NfP{};
    p.g = GridP{0u, L, d->log2_per_level_scale, d->base_resolution, d->gridtype, d->align_corners ? 1u : 0u, d->interp, 1u};
    p.table = reinterpret_cast<const float2*>(d->embeddings);
    p.offsets = d->offsets;
    p.bound = d->bound;
    p.inv2b = 1.0f / (2.0f * d->bound);
    p.nl = nl; p.W = d->out_dim;
    p.act = d->density_activation; p.prior = d->density_prior; p.sig = d->albedo_sigmoid ? 1u : 0u; p.raw = d->raw ? 1u : 0u;
    p.sigma_scale = d->sigma_scale;
    const uint32_t esz = d->precision ? 2u : 4u, pad = 16u / esz;
    uint32_t off = 0, poff = 0;
    p.bb[0] = 0;
    p.sumN = 0;
    for (uint32_t l = 0; l < nl; l++) {
        p.K[l] = l == 0 ? 2u * L : d->hidden;
        p.N[l] = l + 1 == nl ? d->out_dim : d->hidden;
        p.KP[l] = (p.K[l] + 15u) / 16u * 16u;
        p.NP[l] = (p.N[l] + 15u) / 16u * 16u;
        p.w[l] = d->weight[l]; p.b[l] = d->bias[l];
        p.woff[l] = off; p.wst[l] = p.KP[l] + pad; off += p.NP[l] * p.wst[l];
        p.pw[l] = poff; p.pb[l] = poff + p.N[l] * p.K[l]; poff = p.pb[l] + p.N[l];
        p.bb[l + 1] = p.bb[l] + (p.NP[l] / 16u) * (p.KP[l] / 16u);
        p.sumN += p.N[l];
    }
    p.P = poff + 1u;
    p.aoff[0] = off; p.ast[0] = p.KP[0] + pad; off += NF_TILE * p.ast[0];
    for (uint32_t l = 0; l < nl; l++) { p.aoff[l + 1] = off; p.ast[l + 1] = p.NP[l] + pad; off += NF_TILE * p.ast[l + 1]; }
    p.bias_byte_off = (uint32_t)dwg_align_up((size_t)off * esz, 16);
    lds_bytes = p.bias_byte_off + (256 + 2 * NF_TILE * 3 + NF_TILE) * sizeof(float);
    if (lds_bytes > 160 * 1024 || p.bb[nl] > 4u * NF_MAXS || p.sumN > 256) return DWG_E_ARG;
    return DWG_OK;
}

template <typename K>
void lds_opt_in(K* kernel, bool& done) {
    if (!done) { hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); done = true; }
}

uint64_t nf_chunk(uint64_t M) { return M < NF_CHUNK ? M : NF_CHUNK; }
uint32_t nf_bwd_groups(uint64_t M) { const uint64_t t = (M + NF_TILE - 1) / NF_TILE; return (uint32_t)(t < NF_BWD_WG ? t : NF_BWD_WG); }

// one launch of k_nf_bwd over the chunk [m0, m0 + n)
template <typename T, typename XS, bool ALB>
void launch_bwd(const NfP& p, const XS& x, uint64_t m0, uint64_t n, const float* dsigma, uint32_t ds_stride, const void* dalbedo, float* d_enc,
                float* xn, float* partial, int first, int want_w, uint32_t G, size_t lds, hipStream_t st) {
    static bool attr = false; lds_opt_in(&k_nf_bwd<T, XS, ALB>, attr);
    DWG_LAUNCH("nerf_field_bwd", (k_nf_bwd<T, XS, ALB>), dim3(G), dim3(256), lds, st, p, x, m0, n, dsigma, ds_stride, (const T*)dalbedo, d_enc, xn,
               partial, first, want_w);
}

template <typename T, int NC>
int launch_render(const NfP& p, const MarchP& m, const RenderP& q, unsigned grid, size_t lds, hipStream_t st) {
    static bool attr = false; lds_opt_in(&k_nf_render<T, NC>, attr);
    DWG_LAUNCH("nf_render", (k_nf_render<T, NC>), dim3(grid), dim3(256), lds, st, p, m, q);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

template <typename T, int NC>
int launch_render_shaded(const NfP& p, const MarchP& m, const RenderP& q, const ShadeP& sh, unsigned grid, size_t lds, hipStream_t st) {
    static bool attr = false; lds_opt_in(&k_nf_render_shaded<T, NC>, attr);
    DWG_LAUNCH("nf_render_shaded", (k_nf_render_shaded<T, NC>), dim3(grid), dim3(256), lds, st, p, m, q, sh);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

// the checks dwg_nerf_render_infer and dwg_nerf_render_shaded share; lds: the field's bytes in, the render's out
int render_args(const dwg_nerf_field_desc* desc, NfP& p, size_t& lds, float bound, uint32_t max_steps, uint32_t C, uint32_t H) {
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (!march_args_ok(bound, max_steps, C, H)) return DWG_E_ARG;
    if (desc->raw || (desc->out_dim != 4 && desc->out_dim != 5)) return DWG_E_ARG;
    lds += (NR_SLOTS * 3 + 16) * sizeof(float);
    if (lds > 160 * 1024) return DWG_E_ARG;
    return DWG_OK;
}

unsigned render_grid(uint32_t N, uint32_t max_workgroups) {
    const uint32_t blocks = (uint32_t)(((uint64_t)N + 63u) / 64u), cap = max_workgroups ? max_workgroups : NR_DEFAULT_WG;
    return blocks < cap ? blocks : cap;
}

}  // namespace

extern "C" {

int dwg_nerf_field_forward(const dwg_nerf_field_desc* desc, const float* x, uint64_t M, float* sigma, void* albedo, dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (M == 0) return DWG_OK;
    if (!x || !sigma || !albedo) return DWG_E_ARG;
    const uint64_t ntiles = (M + NF_TILE - 1) / NF_TILE;
    const unsigned grid = (unsigned)(ntiles < 4096 ? ntiles : 4096);
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) {
        static bool attr = false; lds_opt_in(&k_nf_fwd<_Float16>, attr);
        DWG_LAUNCH("nerf_field_fwd", k_nf_fwd<_Float16>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, sigma, (_Float16*)albedo);
    } else {
        static bool attr = false; lds_opt_in(&k_nf_fwd<float>, attr);
        DWG_LAUNCH("nerf_field_fwd", k_nf_fwd<float>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, sigma, (float*)albedo);
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_nerf_field_backward_workspace_bytes(const dwg_nerf_field_desc* desc, uint64_t M) {
    NfP p;
    size_t lds = 0;
    if (make_params(desc, p, lds) || M == 0) return 0;
    const uint64_t ch = nf_chunk(M);
    size_t b = dwg_align_up((size_t)nf_bwd_groups(M) * p.P * sizeof(float), 256) + dwg_align_up((size_t)ch * p.K[0] * sizeof(float), 256) +
               dwg_align_up((size_t)ch * 3 * sizeof(float), 256);
    if (desc->host_offsets) b += dwg_grid_backward_slabs_workspace_bytes((uint32_t)ch, desc->num_levels, (uint32_t)desc->host_offsets[desc->num_levels]);
    return b;
}

int dwg_nerf_field_backward(const dwg_nerf_field_desc* desc, const float* x, uint64_t M, const float* dsigma, const void* dalbedo,
                            const dwg_nerf_field_grads* grads, void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (!grads) return DWG_E_ARG;
    if (M == 0) return DWG_OK;
    if (!x || !dsigma || !dalbedo) return DWG_E_ARG;
    bool want_w = grads->sigma_scale != nullptr;
    for (uint32_t l = 0; l < p.nl; l++) want_w = want_w || grads->weight[l] || grads->bias[l];
    const bool want_t = grads->embeddings != nullptr;
    if (grads->sigma_scale && p.act != 2) return DWG_E_ARG;
    if (want_t) {
        if (!desc->host_offsets) return DWG_E_ARG;
        if ((uint64_t)desc->host_offsets[desc->num_levels] > 16384ull * 4096ull) return DWG_E_ARG;      // the slab pass's table limit
    }
    if (!want_w && !want_t) return DWG_OK;
    if (!workspace || ((uintptr_t)workspace & 255u)) return DWG_E_ARG;
    if (workspace_bytes < dwg_nerf_field_backward_workspace_bytes(desc, M)) return DWG_E_CAPACITY;
    const uint64_t ch = nf_chunk(M);
    const uint32_t G = nf_bwd_groups(M);
    unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
    float* partial = reinterpret_cast<float*>(w); w += dwg_align_up((size_t)G * p.P * sizeof(float), 256);
    float* d_enc = reinterpret_cast<float*>(w); w += dwg_align_up((size_t)ch * p.K[0] * sizeof(float), 256);
    float* xn = reinterpret_cast<float*>(w); w += dwg_align_up((size_t)ch * 3 * sizeof(float), 256);
    void* slab_ws = w;
    const size_t slab_bytes = want_t ? workspace_bytes - (size_t)(w - reinterpret_cast<unsigned char*>(workspace)) : 0;
    hipStream_t st = (hipStream_t)stream;
    for (uint64_t m0 = 0; m0 < M; m0 += ch) {
        const uint64_t n = M - m0 < ch ? M - m0 : ch;
        if (desc->precision)
            launch_bwd<_Float16, XPoints, true>(p, XPoints{x}, m0, n, dsigma, 1u, dalbedo, want_t ? d_enc : nullptr, want_t ? xn : nullptr, partial,
                                                m0 == 0 ? 1 : 0, want_w ? 1 : 0, G, lds, st);
        else
            launch_bwd<float, XPoints, true>(p, XPoints{x}, m0, n, dsigma, 1u, dalbedo, want_t ? d_enc : nullptr, want_t ? xn : nullptr, partial,
                                             m0 == 0 ? 1 : 0, want_w ? 1 : 0, G, lds, st);
        DWG_RETURN_IF_LAUNCH_FAILED();
        if (want_t) {
            rc = dwg_grid_encode_backward_slabs(d_enc, xn, desc->embeddings, desc->offsets, grads->embeddings, (uint32_t)n, 3u, 2u,
                                                desc->num_levels, desc->log2_per_level_scale, desc->base_resolution, nullptr, nullptr,
                                                desc->gridtype, desc->align_corners ? 1u : 0u, desc->interp, 1u, desc->host_offsets,
                                                slab_ws, slab_bytes, /*accumulate*/ 1, stream);
            if (rc) return rc;
        }
    }
    if (want_w) {
        DWG_LAUNCH("nerf_field_wgrad_reduce", k_nf_reduce, dim3((p.P + 255u) / 256u), dim3(256), 0, st, p, G, (const float*)partial, *grads);
        DWG_RETURN_IF_LAUNCH_FAILED();
    }
    return DWG_OK;
}

int dwg_nerf_field_forward_fd(const dwg_nerf_field_desc* desc, const float* x, uint64_t M, float epsilon, float* sigma, void* albedo,
                              float* sigma_fd, dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (desc->raw || !(epsilon > 0.f)) return DWG_E_ARG;
    if (M == 0) return DWG_OK;
    if (!x || !sigma || !albedo || !sigma_fd) return DWG_E_ARG;
    const uint64_t ntiles = (M + NF_TILE - 1) / NF_TILE;
    const unsigned grid = (unsigned)(ntiles < 4096 ? ntiles : 4096);
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) {
        static bool attr = false; lds_opt_in(&k_nf_fwd_fd<_Float16>, attr);
        DWG_LAUNCH("nerf_field_fwd_fd", k_nf_fwd_fd<_Float16>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, epsilon, sigma, (_Float16*)albedo, sigma_fd);
    } else {
        static bool attr = false; lds_opt_in(&k_nf_fwd_fd<float>, attr);
        DWG_LAUNCH("nerf_field_fwd_fd", k_nf_fwd_fd<float>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, epsilon, sigma, (float*)albedo, sigma_fd);
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_nerf_field_backward_fd(const dwg_nerf_field_desc* desc, const float* x, uint64_t M, float epsilon, const float* dsigma, const void* dalbedo,
                               const float* dsigma_fd, const dwg_nerf_field_grads* grads, void* workspace, size_t workspace_bytes,
                               dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (!grads || desc->raw || !(epsilon > 0.f)) return DWG_E_ARG;
    if (M == 0) return DWG_OK;
    if (!x || !dsigma || !dsigma_fd) return DWG_E_ARG;
    bool want_w = grads->sigma_scale != nullptr;
    for (uint32_t l = 0; l < p.nl; l++) want_w = want_w || grads->weight[l] || grads->bias[l];
    const bool want_t = grads->embeddings != nullptr;
    if (grads->sigma_scale && p.act != 2) return DWG_E_ARG;
    if (want_t) {
        if (!desc->host_offsets) return DWG_E_ARG;
        if ((uint64_t)desc->host_offsets[desc->num_levels] > 16384ull * 4096ull) return DWG_E_ARG;      // the slab pass's table limit
    }
    if (!want_w && !want_t) return DWG_OK;
    if (!workspace || ((uintptr_t)workspace & 255u)) return DWG_E_ARG;
    if (workspace_bytes < dwg_nerf_field_backward_workspace_bytes(desc, M)) return DWG_E_CAPACITY;
    const uint64_t ch = nf_chunk(M);
    const uint32_t G = nf_bwd_groups(M);
    unsigned char* w = reinterpret_cast<unsigned char*>(workspace);
    float* partial = reinterpret_cast<float*>(w); w += dwg_align_up((size_t)G * p.P * sizeof(float), 256);
    float* d_enc = reinterpret_cast<float*>(w); w += dwg_align_up((size_t)ch * p.K[0] * sizeof(float), 256);
    float* xn = reinterpret_cast<float*>(w); w += dwg_align_up((size_t)ch * 3 * sizeof(float), 256);
    void* slab_ws = w;
    const size_t slab_bytes = want_t ? workspace_bytes - (size_t)(w - reinterpret_cast<unsigned char*>(workspace)) : 0;
    float* de = want_t ? d_enc : nullptr;
    float* xo = want_t ? xn : nullptr;
    const int ww = want_w ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    // The six shifted point sets first, chunk by chunk and in their +- pairs, then the points themselves: the two gradients of a pair
    // have opposite signs and, through 0.5 / (eps |g|), can be many orders larger than the point's own, so they meet in the partials
    // before anything smaller is added (on a constant density they cancel there exactly).  `first`: the very first launch.
    int first = 1;
    for (uint32_t round = 0; round < 2u; ++round) {
        for (uint64_t m0 = 0; m0 < M; m0 += ch) {
            const uint64_t n = M - m0 < ch ? M - m0 : ch;
            for (uint32_t pass = round ? 0u : 1u; pass < (round ? 1u : 7u); ++pass) {
                // pass 0: the points, with the density's own gradient and the albedo's when there is one; pass s: shift s - 1, column s - 1 of dsigma_fd
                const XPointsFd xs{x, pass, epsilon, p.bound};
                const float* ds = pass ? dsigma_fd + (pass - 1u) : dsigma;
                const uint32_t stride = pass ? 6u : 1u;
                if (desc->precision) {
                    if (pass == 0u && dalbedo) launch_bwd<_Float16, XPointsFd, true>(p, xs, m0, n, ds, stride, dalbedo, de, xo, partial, first, ww, G, lds, st);
                    else launch_bwd<_Float16, XPointsFd, false>(p, xs, m0, n, ds, stride, nullptr, de, xo, partial, first, ww, G, lds, st);
                } else {
                    if (pass == 0u && dalbedo) launch_bwd<float, XPointsFd, true>(p, xs, m0, n, ds, stride, dalbedo, de, xo, partial, first, ww, G, lds, st);
                    else launch_bwd<float, XPointsFd, false>(p, xs, m0, n, ds, stride, nullptr, de, xo, partial, first, ww, G, lds, st);
                }
                DWG_RETURN_IF_LAUNCH_FAILED();
                first = 0;
                if (want_t) {
                    rc = dwg_grid_encode_backward_slabs(d_enc, xn, desc->embeddings, desc->offsets, grads->embeddings, (uint32_t)n, 3u, 2u,
                                                        desc->num_levels, desc->log2_per_level_scale, desc->base_resolution, nullptr, nullptr,
                                                        desc->gridtype, desc->align_corners ? 1u : 0u, desc->interp, 1u, desc->host_offsets,
                                                        slab_ws, slab_bytes, /*accumulate*/ 1, stream);
                    if (rc) return rc;
                }
            }
        }
    }
    if (want_w) {
        DWG_LAUNCH("nerf_field_wgrad_reduce", k_nf_reduce, dim3((p.P + 255u) / 256u), dim3(256), 0, st, p, G, (const float*)partial, *grads);
        DWG_RETURN_IF_LAUNCH_FAILED();
    }
    return DWG_OK;
}

int dwg_pc_lattice_sigma(const dwg_nerf_field_desc* desc, const float* ax, const float* ay, const float* az, uint32_t nx, uint32_t ny,
                         uint32_t nz, uint32_t split, float* sigma, float* minmax, dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (desc->raw || split == 0) return DWG_E_ARG;
    const uint64_t M = (uint64_t)nx * ny * nz;
    if (M == 0) return DWG_OK;
    if ((uint64_t)nx * ny >= (1ull << 32) || M >= (1ull << 32)) return DWG_E_ARG;
    if (!ax || !ay || !az || !sigma || !minmax) return DWG_E_ARG;
    const uint64_t ntiles = (M + NF_TILE - 1) / NF_TILE;
    const unsigned grid = (unsigned)(ntiles < DWG_PC_MINMAX_PAIRS ? ntiles : DWG_PC_MINMAX_PAIRS);
    const XLattice x{pc_lattice(nx, ny, nz, split), ax, ay, az};
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) {
        static bool attr = false; lds_opt_in(&k_nf_lattice<_Float16>, attr);
        DWG_LAUNCH("pc_lattice_sigma", k_nf_lattice<_Float16>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, sigma, minmax);
    } else {
        static bool attr = false; lds_opt_in(&k_nf_lattice<float>, attr);
        DWG_LAUNCH("pc_lattice_sigma", k_nf_lattice<float>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, sigma, minmax);
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_occ_lattice_sigma(const dwg_nerf_field_desc* desc, const float* axis, const float* noise, const float* scale, const float* half,
                          uint32_t C, uint32_t H, uint32_t random_sigmas, float* tmp_grid, dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    uint32_t lg = 0;
    if (desc->raw || !occ_limits(C, H, lg)) return DWG_E_ARG;
    if (!axis || !noise || !scale || !half || !tmp_grid) return DWG_E_ARG;
    const uint64_t M = (uint64_t)C << (3u * lg);
    const uint64_t ntiles = M / NF_TILE;                    // H >= 4: H^3 is a multiple of 64
    const unsigned grid = (unsigned)(ntiles < 4096 ? ntiles : 4096);
    const XOccupancy x{OccLattice{axis, noise, scale, half, lg}};
    const uint32_t blob = random_sigmas ? 1u : 0u;
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) {
        static bool attr = false; lds_opt_in(&k_nf_occupancy<_Float16>, attr);
        DWG_LAUNCH("occ_lattice_sigma", k_nf_occupancy<_Float16>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, blob, tmp_grid);
    } else {
        static bool attr = false; lds_opt_in(&k_nf_occupancy<float>, attr);
        DWG_LAUNCH("occ_lattice_sigma", k_nf_occupancy<float>, dim3(grid), dim3(256), lds, st, p, x, M, ntiles, blob, tmp_grid);
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_nerf_render_infer(const dwg_nerf_field_desc* desc, const float* rays_o, const float* rays_d, const float* nears, const float* fars,
                          uint32_t N, const uint8_t* bitfield, float bound, uint32_t contract, float dt_gamma, uint32_t max_steps, uint32_t C,
                          uint32_t H, float T_thresh, uint32_t binarize, float* weights_sum, float* depth, float* image, int32_t* counts,
                          uint32_t max_workgroups, dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = render_args(desc, p, lds, bound, max_steps, C, H);
    if (rc) return rc;
    if (N == 0) return DWG_OK;
    if (!rays_o || !rays_d || !nears || !fars || !bitfield || !weights_sum || !depth || !image) return DWG_E_ARG;
    const MarchP m = make_march(bitfield, bound, contract, dt_gamma, max_steps, C, H);
    const RenderP q{rays_o, rays_d, nears, fars, N, max_steps, T_thresh, binarize, weights_sum, depth, image, counts};
    const unsigned grid = render_grid(N, max_workgroups);
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) return desc->out_dim == 4 ? launch_render<_Float16, 3>(p, m, q, grid, lds, st) : launch_render<_Float16, 4>(p, m, q, grid, lds, st);
    return desc->out_dim == 4 ? launch_render<float, 3>(p, m, q, grid, lds, st) : launch_render<float, 4>(p, m, q, grid, lds, st);
}

int dwg_nerf_render_shaded(const dwg_nerf_field_desc* desc, const float* rays_o, const float* rays_d, const float* nears, const float* fars,
                           uint32_t N, const uint8_t* bitfield, float bound, uint32_t contract, float dt_gamma, uint32_t max_steps, uint32_t C,
                           uint32_t H, float T_thresh, uint32_t binarize, uint32_t shading, const float* light_d, float ambient_ratio,
                           float epsilon, float* weights_sum, float* depth, float* image, int32_t* counts, uint32_t max_workgroups,
                           dwg_stream_t stream) {
    NfP p;
    size_t lds = 0;
    int rc = render_args(desc, p, lds, bound, max_steps, C, H);
    if (rc) return rc;
    if (shading < DWG_SHADE_NORMAL || shading > DWG_SHADE_LAMBERTIAN || (shading >= DWG_SHADE_TEXTURELESS && !light_d) || !(epsilon > 0.f))
        return DWG_E_ARG;
    if (shading == DWG_SHADE_LAMBERTIAN && desc->out_dim == 5) return DWG_E_ARG;      // albedo [., 4] * lambertian plus the zero pad: five channels into four
    if (N == 0) return DWG_OK;
    if (!rays_o || !rays_d || !nears || !fars || !bitfield || !weights_sum || !depth || !image) return DWG_E_ARG;
    const MarchP m = make_march(bitfield, bound, contract, dt_gamma, max_steps, C, H);
    const RenderP q{rays_o, rays_d, nears, fars, N, max_steps, T_thresh, binarize, weights_sum, depth, image, counts};
    // the field's own bound clamps the shifted points (normal() clamps to self.bound, which common_forward normalises by)
    const ShadeP sh{shading, light_d, ambient_ratio, (float)(1.0 - (double)ambient_ratio), epsilon, desc->bound};
    const unsigned grid = render_grid(N, max_workgroups);
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) return desc->out_dim == 4 ? launch_render_shaded<_Float16, 3>(p, m, q, sh, grid, lds, st) : launch_render_shaded<_Float16, 4>(p, m, q, sh, grid, lds, st);
    return desc->out_dim == 4 ? launch_render_shaded<float, 3>(p, m, q, sh, grid, lds, st) : launch_render_shaded<float, 4>(p, m, q, sh, grid, lds, st);
}

}  // extern "C"
