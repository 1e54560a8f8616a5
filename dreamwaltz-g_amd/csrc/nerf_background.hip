// nerf_background.hip -- the learned background of stage I (boundary B22, bg_mode 'nerf'): frequency encoding of the ray direction ->
// bg_net -> sigmoid / identity, one launch.
//
// Native restatement of _NeRFNetwork.background's learned mode (core/nerf/nerf_model.py:134-139, 248-256) on the tile scheme of
// nerf_field.hip.  A workgroup (4 waves) takes 64 rays at a time:
//   1. the 64 x (3 + 6 degree) columns of the encoding (freq_math.h, fp32) fill an LDS tile enc[64][KP], K padded to the MFMA step with
//      zeros;
//   2. each wave runs its 16 rows through the layers on the matrix cores (16x16 output blocks, the weights of all layers resident in
//      LDS), every layer's output going back to LDS; nothing between rays_d and the [N, C] image is written to HBM;
//   3. one thread per ray applies the epilogue and writes its row.
// The backward recomputes 1-2 per tile, then walks the layers backwards in LDS: dZ_l -> dW_l (MFMA over the tile's 64 rays, accumulated
// in registers across the workgroup's tiles), db_l, dZ_{l-1} = (dZ_l W_l) * relu'.  The per-workgroup partials are summed by a second
// kernel in workgroup order; no float atomics anywhere, so the gradients are bit-reproducible.  The directions get no gradient.
// The MFMA tile helpers (Mm, mma_block) are nerf_field.hip's statements, restated here so that that unit compiles as it did.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_nerf_background.h"
#include "freq_math.h"

namespace {

constexpr int BG_TILE = 64;                 // rays per workgroup tile (4 waves x 16 rows)
constexpr int BG_MAXL = DWG_NERF_BG_MAX_LAYERS;
constexpr int BG_MAXS = 9;                  // weight-gradient blocks per wave: (16 + 16 + 4) 16x16 blocks of 3 layers / 4 waves
constexpr uint32_t BG_FWD_WG = 4096;        // workgroups of the forward at most
constexpr uint32_t BG_BWD_WG = 512;         // workgroups of the backward at most (2 per CU): the number of weight-gradient partials
constexpr size_t BG_LDS_MAX = 160 * 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct BgP {
    uint32_t K0;                            // encoder_bg's width, 3 + 6 degree
    uint32_t nl, C, sig;                    // layers, out_dim, the sigmoid epilogue
    uint32_t K[BG_MAXL], N[BG_MAXL], KP[BG_MAXL], NP[BG_MAXL];      // true and padded (multiple of 16) in / out widths per layer
    const float* w[BG_MAXL];
    const float* b[BG_MAXL];
    // LDS layout, in elements of the operand type: weights [NP][KP + pad], activations [64][width + pad]
    uint32_t woff[BG_MAXL], wst[BG_MAXL];
    uint32_t aoff[BG_MAXL + 1], ast[BG_MAXL + 1];       // 0: enc, 1..nl-1: hidden outputs, nl: last layer's output
    uint32_t bias_byte_off;                 // float bias[BG_MAXL][64] after the operand-typed part, then the tile's directions [64][3]
    // gradient partial layout (floats): W_l [N][K], then b_l [N]
    uint32_t pw[BG_MAXL], pb[BG_MAXL], P;
    uint32_t bb[BG_MAXL + 1];               // prefix over layers of the 16x16 weight-gradient blocks: wave w owns blocks w, w + 4, ...
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

// weights (rounded to T) and biases into LDS; padding zero.  The encoding's padding columns are written by every tile (bg_tile).
template <typename T>
__device__ void load_weights(const BgP& p, T* lds, float* bias) {
    for (uint32_t l = 0; l < p.nl; l++) {
        T* w = lds + p.woff[l];
        const uint32_t n_el = p.NP[l] * p.wst[l];
        for (uint32_t e = threadIdx.x; e < n_el; e += 256) {
            const uint32_t n = e / p.wst[l], k = e - n * p.wst[l];
            w[e] = (T)((n < p.N[l] && k < p.K[l]) ? p.w[l][n * p.K[l] + k] : 0.f);
        }
        for (uint32_t n = threadIdx.x; n < 64; n += 256) bias[l * 64 + n] = n < p.N[l] ? p.b[l][n] : 0.f;
    }
}

template <typename T>
__device__ __forceinline__ void lds_carve(const BgP& p, unsigned char* smem, T*& lds, float*& bias, float*& sx) {
    lds = reinterpret_cast<T*>(smem);
    bias = reinterpret_cast<float*>(smem + p.bias_byte_off);
    sx = bias + BG_MAXL * 64;
}

// the directions of the tile -> sx, their encoding (fp32, rounded to T on the store: the operand's rounding) -> enc, then the layers; rays
// at or past N are encoded from d = 0 (their outputs are never stored).  Ends with a barrier: every layer output is in LDS.
template <typename T>
__device__ void bg_tile(const BgP& p, const float* __restrict__ dirs, uint32_t N, uint32_t p0, T* lds, const float* bias, float* sx) {
    for (uint32_t i = threadIdx.x; i < BG_TILE * 3; i += 256) sx[i] = p0 + i / 3u < N ? dirs[(size_t)p0 * 3u + i] : 0.f;
    __syncthreads();
    T* enc = lds + p.aoff[0];
    const uint32_t KP0 = p.KP[0], est = p.ast[0];
    for (uint32_t t = threadIdx.x; t < BG_TILE * KP0; t += 256) {
        const uint32_t pt = t / KP0, c = t - pt * KP0;
        enc[pt * est + c] = (T)(c < p.K0 ? freq_column(sx + 3u * pt, c) : 0.f);
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

__device__ __forceinline__ float bg_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

template <typename T>
__global__ __launch_bounds__(256) void k_bg_fwd(BgP p, const float* __restrict__ dirs, uint32_t N, uint32_t ntiles, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds; float *bias, *sx;
    lds_carve(p, smem, lds, bias, sx);
    load_weights(p, lds, bias);
    const uint32_t C = p.C;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t p0 = tile * BG_TILE;
        bg_tile(p, dirs, N, p0, lds, bias, sx);
        // the tile's rows are contiguous in out: thread t writes element t of the [rows, C] block
        const uint32_t rows = N - p0 < (uint32_t)BG_TILE ? N - p0 : (uint32_t)BG_TILE;
        for (uint32_t t = threadIdx.x; t < rows * C; t += 256) {
            const uint32_t pt = t / C, c = t - pt * C;
            float v = (float)lds[p.aoff[p.nl] + pt * p.ast[p.nl] + c];
            if (p.sig) v = (float)(T)bg_sigmoid(v);          // under f16 the sigmoid's output is a half tensor
            out[(size_t)p0 * C + t] = v;
        }
        __syncthreads();
    }
}

// partial: [gridDim.x][P] floats, overwritten.
template <typename T>
__global__ __launch_bounds__(256) void k_bg_bwd(BgP p, const float* __restrict__ dirs, uint32_t N, uint32_t ntiles, const float* __restrict__ d_out,
                                                float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds; float *bias, *sx;
    lds_carve(p, smem, lds, bias, sx);
    load_weights(p, lds, bias);
    const uint32_t C = p.C, nl = p.nl;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, r = lane & 15u, q = lane >> 4;
    // the bias this thread owns
    uint32_t bl = BG_MAXL, bn = 0;
    {
        uint32_t base = 0;
        for (uint32_t l = 0; l < nl; l++) {
            if (threadIdx.x >= base && threadIdx.x < base + p.N[l]) { bl = l; bn = threadIdx.x - base; }
            base += p.N[l];
        }
    }
    f32x4 acc[BG_MAXS];
#pragma unroll
    for (int s = 0; s < BG_MAXS; s++) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float acc_b = 0.f;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t p0 = tile * BG_TILE;
        bg_tile(p, dirs, N, p0, lds, bias, sx);
        // d(last layer output), rounded to the operand type where autograd hands the reference an fp16 gradient
        if (threadIdx.x < BG_TILE) {
            const uint32_t t = threadIdx.x, pt = p0 + t;
            T* o = lds + p.aoff[nl] + t * p.ast[nl];
            float d[16];
#pragma unroll
            for (int c = 0; c < 16; c++) d[c] = 0.f;
            if (pt < N) {
                const float* g = d_out + (size_t)pt * C;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    if ((uint32_t)c < C) {
                        float gv = (float)(T)g[c];
                        if (p.sig) { const float a = (float)(T)bg_sigmoid((float)o[c]); gv = gv * (1.f - a) * a; }
                        d[c] = gv;
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
            const uint32_t nkb = p.KP[l] / 16u, b0 = p.bb[l], b1 = p.bb[l + 1];
#pragma unroll
            for (int s = 0; s < BG_MAXS; s++) {
                const uint32_t gb = wave + 4u * s;
                if (gb >= b0 && gb < b1) {
                    const uint32_t loc = gb - b0, nb = loc / nkb, kb = loc - nb * nkb;
                    // dW[n][k] += sum_p dZ[p][n] X[p][k]
                    acc[s] = mma_block<T, false, false>(Z + nb * 16u, 1u, zs, X + kb * 16u, xs, 1u, (uint32_t)BG_TILE, acc[s]);
                }
            }
            if (bl == (uint32_t)l) {
                float sb = 0.f;
                for (uint32_t pp = 0; pp < BG_TILE; pp++) sb += (float)Z[pp * zs + bn];
                acc_b += sb;
            }
            if (l > 0) {                    // the encoding has no gradient: layer 0 stops at its weights
                const uint32_t ncb = p.KP[l] / 16u;
                const T* Wl = lds + p.woff[l];
                f32x4 dx[4];
#pragma unroll
                for (int cb = 0; cb < 4; cb++) {
                    dx[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
                    // dX[i][j] = sum_n dZ[i][n] W[n][j]
                    if ((uint32_t)cb < ncb)
                        dx[cb] = mma_block<T, true, false>(Z + wave * 16u * zs, zs, 1u, Wl + cb * 16u, p.wst[l], 1u, p.NP[l], dx[cb]);
                }
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
            }
            __syncthreads();
        }
    }
    float* P = partial + (size_t)blockIdx.x * p.P;
#pragma unroll
    for (int s = 0; s < BG_MAXS; s++) {
        const uint32_t gb = wave + 4u * s;
        if (gb >= p.bb[nl]) continue;
        uint32_t l = 0;
        while (gb >= p.bb[l + 1]) l++;
        const uint32_t nkb = p.KP[l] / 16u, loc = gb - p.bb[l], nb = loc / nkb, kb = loc - nb * nkb;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint32_t nn = nb * 16u + 4u * q + v, k = kb * 16u + r;
            if (nn < p.N[l] && k < p.K[l]) P[p.pw[l] + nn * p.K[l] + k] = acc[s][v];
        }
    }
    if (bl < nl) P[p.pb[bl] + bn] = acc_b;
}

// sum of the G partials of every parameter, in workgroup order
__global__ __launch_bounds__(256) void k_bg_reduce(BgP p, uint32_t G, const float* __restrict__ partial, dwg_nerf_bg_grads gr) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.P) return;
    float* dst = nullptr;
    for (uint32_t l = 0; l < p.nl; l++) {
        if (i >= p.pw[l] && i < p.pb[l]) dst = gr.weight[l] ? gr.weight[l] + (i - p.pw[l]) : nullptr;
        else if (i >= p.pb[l] && i < p.pb[l] + p.N[l]) dst = gr.bias[l] ? gr.bias[l] + (i - p.pb[l]) : nullptr;
    }
    if (!dst) return;
    float s = 0.f;
    for (uint32_t g = 0; g < G; g++) s += partial[(size_t)g * p.P + i];
    *dst = s;
}

__global__ __launch_bounds__(256) void k_freq_encode(const float* __restrict__ dirs, uint64_t total, uint32_t K0, float* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint64_t pt = i / K0;
    const uint32_t c = (uint32_t)(i - pt * K0);
    const float x[3] = {dirs[pt * 3u], dirs[pt * 3u + 1u], dirs[pt * 3u + 2u]};
    out[i] = freq_column(x, c);
}

int make_params(const dwg_nerf_bg_desc* d, BgP& p, size_t& lds_bytes) {
    if (!d) return DWG_E_ARG;
    const uint32_t nl = d->num_layers;
    if (d->degree == 0 || d->degree > DWG_NERF_BG_MAX_DEGREE || nl == 0 || nl > (uint32_t)BG_MAXL) return DWG_E_ARG;
    if (nl > 1 && d->hidden != 16 && d->hidden != 32 && d->hidden != 64) return DWG_E_ARG;
    if ((d->out_dim != 3 && d->out_dim != 4) || d->precision > 1 || d->sigmoid > 1) return DWG_E_ARG;
    for (uint32_t l = 0; l < nl; l++) if (!d->weight[l] || !d->bias[l]) return DWG_E_ARG;
    p = BgP{};
    p.K0 = freq_output_dim(d->degree);
    p.nl = nl; p.C = d->out_dim; p.sig = d->sigmoid;
    const uint32_t esz = d->precision ? 2u : 4u, pad = 16u / esz;
    uint32_t off = 0, poff = 0;
    p.bb[0] = 0;
    p.sumN = 0;
    for (uint32_t l = 0; l < nl; l++) {
        p.K[l] = l == 0 ? p.K0 : d->hidden;
        p.N[l] = l + 1 == nl ? d->out_dim : d->hidden;
        p.KP[l] = (p.K[l] + 15u) / 16u * 16u;
        p.NP[l] = (p.N[l] + 15u) / 16u * 16u;
        p.w[l] = d->weight[l]; p.b[l] = d->bias[l];
        p.woff[l] = off; p.wst[l] = p.KP[l] + pad; off += p.NP[l] * p.wst[l];
        p.pw[l] = poff; p.pb[l] = poff + p.N[l] * p.K[l]; poff = p.pb[l] + p.N[l];
        p.bb[l + 1] = p.bb[l] + (p.NP[l] / 16u) * (p.KP[l] / 16u);
        p.sumN += p.N[l];
    }
    p.P = poff;
    p.aoff[0] = off; p.ast[0] = p.KP[0] + pad; off += BG_TILE * p.ast[0];
    for (uint32_t l = 0; l < nl; l++) { p.aoff[l + 1] = off; p.ast[l + 1] = p.NP[l] + pad; off += BG_TILE * p.ast[l + 1]; }
    p.bias_byte_off = (uint32_t)dwg_align_up((size_t)off * esz, 16);
    lds_bytes = p.bias_byte_off + (BG_MAXL * 64 + BG_TILE * 3) * sizeof(float);
    if (lds_bytes > BG_LDS_MAX || p.bb[nl] > 4u * BG_MAXS || p.sumN > 256) return DWG_E_ARG;
    return DWG_OK;
}

template <typename K>
void lds_opt_in(K* kernel, bool& done) {
    if (!done) { hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BG_LDS_MAX); done = true; }
}

uint32_t bg_tiles(uint32_t N) { return (uint32_t)(((uint64_t)N + BG_TILE - 1) / BG_TILE); }

}  // namespace

extern "C" {

int dwg_nerf_freq_encode(uint32_t N, const float* dirs, uint32_t degree, float* out, dwg_stream_t stream) {
    if (degree == 0 || degree > DWG_NERF_BG_MAX_DEGREE || N >= (1u << 31)) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (!dirs || !out) return DWG_E_ARG;
    const uint32_t K0 = freq_output_dim(degree);
    const uint64_t total = (uint64_t)N * K0;
    DWG_LAUNCH("nerf_freq_encode", k_freq_encode, dim3((unsigned)((total + 255u) / 256u)), dim3(256), 0, (hipStream_t)stream, dirs, total, K0, out);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_nerf_bg_forward(uint32_t N, const float* dirs, const dwg_nerf_bg_desc* desc, float* out, dwg_stream_t stream) {
    BgP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (N >= (1u << 31)) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (!dirs || !out) return DWG_E_ARG;
    const uint32_t ntiles = bg_tiles(N);
    const unsigned grid = ntiles < BG_FWD_WG ? ntiles : BG_FWD_WG;
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) {
        static bool attr = false; lds_opt_in(&k_bg_fwd<_Float16>, attr);
        DWG_LAUNCH("nerf_bg_fwd", k_bg_fwd<_Float16>, dim3(grid), dim3(256), lds, st, p, dirs, N, ntiles, out);
    } else {
        static bool attr = false; lds_opt_in(&k_bg_fwd<float>, attr);
        DWG_LAUNCH("nerf_bg_fwd", k_bg_fwd<float>, dim3(grid), dim3(256), lds, st, p, dirs, N, ntiles, out);
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_nerf_bg_backward_workspace_bytes(const dwg_nerf_bg_desc* desc) {
    BgP p;
    size_t lds = 0;
    if (make_params(desc, p, lds)) return 0;
    return dwg_align_up((size_t)BG_BWD_WG * p.P * sizeof(float), 256);
}

int dwg_nerf_bg_backward(uint32_t N, const float* dirs, const float* d_out, const dwg_nerf_bg_desc* desc, const dwg_nerf_bg_grads* grads,
                         void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    BgP p;
    size_t lds = 0;
    int rc = make_params(desc, p, lds);
    if (rc) return rc;
    if (!grads || N >= (1u << 31)) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (!dirs || !d_out) return DWG_E_ARG;
    bool want = false;
    for (uint32_t l = 0; l < p.nl; l++) want = want || grads->weight[l] || grads->bias[l];
    if (!want) return DWG_OK;
    if (!workspace || ((uintptr_t)workspace & 255u)) return DWG_E_ARG;
    if (workspace_bytes < dwg_nerf_bg_backward_workspace_bytes(desc)) return DWG_E_CAPACITY;
    const uint32_t ntiles = bg_tiles(N);
    const uint32_t G = ntiles < BG_BWD_WG ? ntiles : BG_BWD_WG;
    float* partial = reinterpret_cast<float*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (desc->precision) {
        static bool attr = false; lds_opt_in(&k_bg_bwd<_Float16>, attr);
        DWG_LAUNCH("nerf_bg_bwd", k_bg_bwd<_Float16>, dim3(G), dim3(256), lds, st, p, dirs, N, ntiles, d_out, partial);
    } else {
        static bool attr = false; lds_opt_in(&k_bg_bwd<float>, attr);
        DWG_LAUNCH("nerf_bg_bwd", k_bg_bwd<float>, dim3(G), dim3(256), lds, st, p, dirs, N, ntiles, d_out, partial);
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    DWG_LAUNCH("nerf_bg_wgrad_reduce", k_bg_reduce, dim3((p.P + 255u) / 256u), dim3(256), 0, st, p, G, (const float*)partial, *grads);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
