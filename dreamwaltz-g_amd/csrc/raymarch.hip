// raymarch.hip -- occupancy-grid ray marcher and compositing of the NeRF stage for gfx950 (boundary B6).
//
// Native restatement of the reference's CUDA extension (core/nerf/raymarching/rgb/src/raymarching.cu: utils :92-326,
// march_rays_train :338-475, composite_rays_train :501-695, march_rays :714-829, composite_rays :843-925; the latent variant differs only
// in the colour width and has no `binarize`).  Two departures, both invisible to the callers:
//   - march_rays_train: count pass (one lane per ray) -> three-launch exclusive scan of the counts (scan_common.h, which
//     nerf_train.hip and pointcloud.hip use too) -> write pass.  The offsets are ray-major and the output is bit-reproducible (the
//     reference takes them with atomicAdd).
//   - composite_rays_train: one WAVE per ray instead of one lane per ray.  The 64 lanes take 64 consecutive samples of the ray at a time
//     (coalesced loads of its contiguous range), the transmittance is a wave prefix product and the running sums are wave prefix sums;
//     the ray stops after the first lane whose transmittance drops below T_thresh (ballot).  Forward and backward run the same scan code,
//     so the backward's running sums reproduce the forward's totals bit for bit, as the reference's sequential loops do.
//     The `_live` forward (boundary B18, dwg_nerf_train.h) is the same kernel, which then also reports where each ray stopped.
// k_packbits serves dwg_raymarch_packbits and dwg_raymarch_packbits_dev, the last stage of occupancy.hip's dwg_occ_update.
// FP contraction is off in this file: the float32 restatement (tests/raymarch_cases.py) rounds every operation separately, and a
// one-ulp change of t moves a sample across a voxel boundary.  No float atomics anywhere.
#include <float.h>

#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_raymarch.h"
#include "morton.h"
#include "raymarch_common.h"
#include "scan_common.h"

#pragma clang fp contract(off)

namespace {

constexpr float kRPi = 0.3183098861837907f;
constexpr int kRaysPerWave = 4;                     // composite: consecutive rays owned by one wave

// ---------------------------------------------------------------------------------------------------------------------------------
// utils
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void k_near_far(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ aabb,
                           uint32_t N, float min_near, float* __restrict__ nears, float* __restrict__ fars) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const Ray r = load_ray(rays_o + 3 * n, rays_d + 3 * n);
    float near, far;
    near_far_ray(r, aabb, min_near, near, far);
    nears[n] = near;
    fars[n] = far;
}

__global__ void k_sph_from_ray(const float* __restrict__ rays_o, const float* __restrict__ rays_d, float radius, uint32_t N,
                               float* __restrict__ coords) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float ox = rays_o[3 * n], oy = rays_o[3 * n + 1], oz = rays_o[3 * n + 2];
    const float dx = rays_d[3 * n], dy = rays_d[3 * n + 1], dz = rays_d[3 * n + 2];
    const float A = dx * dx + dy * dy + dz * dz;
    const float B = ox * dx + oy * dy + oz * dz;
    const float C = ox * ox + oy * oy + oz * oz - radius * radius;
    const float t = (-B + sqrtf(B * B - A * C)) / A;
    const float x = ox + t * dx, y = oy + t * dy, z = oz + t * dz;
    const float theta = atan2f(sqrtf(x * x + z * z), y);
    const float phi = atan2f(z, x);
    coords[2 * n] = 2.f * theta * kRPi - 1.f;
    coords[2 * n + 1] = phi * kRPi;
}

__global__ void k_morton3d(const int32_t* __restrict__ coords, uint32_t N, int32_t* __restrict__ indices) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    indices[n] = (int32_t)morton3d((uint32_t)coords[3 * n], (uint32_t)coords[3 * n + 1], (uint32_t)coords[3 * n + 2]);
}

__global__ void k_morton3d_invert(const int32_t* __restrict__ indices, uint32_t N, int32_t* __restrict__ coords) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const uint32_t ind = (uint32_t)indices[n];
    coords[3 * n] = (int32_t)morton3d_invert(ind);
    coords[3 * n + 1] = (int32_t)morton3d_invert(ind >> 1);
    coords[3 * n + 2] = (int32_t)morton3d_invert(ind >> 2);
}

// T = float: the threshold itself (dwg_raymarch_packbits); T = const float*: where it lies in device memory (dwg_raymarch_packbits_dev)
__device__ __forceinline__ float thresh_of(float t) { return t; }
__device__ __forceinline__ float thresh_of(const float* t) { return *t; }

template <typename T>
__global__ void k_packbits(const float4* __restrict__ grid, uint32_t N, T thresh_arg, uint8_t* __restrict__ bitfield) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float thresh = thresh_of(thresh_arg);
    const float4 a = grid[2 * n], b = grid[2 * n + 1];
    const uint32_t bits = (a.x > thresh ? 1u : 0u) | (a.y > thresh ? 2u : 0u) | (a.z > thresh ? 4u : 0u) | (a.w > thresh ? 8u : 0u) |
                          (b.x > thresh ? 16u : 0u) | (b.y > thresh ? 32u : 0u) | (b.z > thresh ? 64u : 0u) | (b.w > thresh ? 128u : 0u);
    bitfield[n] = (uint8_t)bits;
}

__global__ void k_flatten_rays(const int32_t* __restrict__ rays, uint32_t N, uint32_t M, int32_t* __restrict__ res) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const uint32_t off = (uint32_t)rays[2 * n], cnt = (uint32_t)rays[2 * n + 1];
    if (off > M || cnt > M - off) return;
    for (uint32_t i = 0; i < cnt; ++i) res[off + i] = (int32_t)n;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// training march: count pass, scan, write pass
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void k_march_count(MarchP p, const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ nears,
                              const float* __restrict__ fars, const float* __restrict__ noises, uint32_t N, uint32_t max_steps,
                              int32_t* __restrict__ rays) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const Ray r = load_ray(rays_o + 3 * n, rays_d + 3 * n);
    const float far = fars[n];
    float t = start_t(p, nears[n], noises[n]);
    uint32_t step = 0;
    float cx, cy, cz, dt;
    while (t < far && step < max_steps)
        if (march_iter(p, r, t, cx, cy, cz, dt)) ++step;
    rays[2 * n + 1] = (int32_t)step;
}

__global__ void k_march_write(MarchP p, const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ nears,
                              const float* __restrict__ fars, const float* __restrict__ noises, uint32_t N, uint32_t M,
                              const int32_t* __restrict__ rays, float* __restrict__ xyzs, float* __restrict__ dirs, float* __restrict__ ts) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const uint32_t off = (uint32_t)rays[2 * n], cnt = (uint32_t)rays[2 * n + 1];
    if (off > M || cnt > M - off) return;
    const Ray r = load_ray(rays_o + 3 * n, rays_d + 3 * n);
    const float far = fars[n];
    float t = start_t(p, nears[n], noises[n]);
    uint32_t step = 0;
    float cx, cy, cz, dt;
    while (t < far && step < cnt) {
        if (march_iter(p, r, t, cx, cy, cz, dt)) {
            const size_t i = (size_t)off + step;
            xyzs[3 * i] = cx; xyzs[3 * i + 1] = cy; xyzs[3 * i + 2] = cz;
            dirs[3 * i] = r.dx; dirs[3 * i + 1] = r.dy; dirs[3 * i + 2] = r.dz;
            *reinterpret_cast<float2*>(ts + 2 * i) = make_float2(t, dt);
            ++step;
        }
    }
}

// the scan of the counts (scan_common.h): the count of ray n is rays[n][1], its offset goes to rays[n][0]
struct RayCount {
    const int32_t* rays;
    __device__ __forceinline__ uint32_t operator()(uint32_t n) const { return (uint32_t)rays[2 * n + 1]; }
};
struct RayOffset {
    int32_t* rays;
    __device__ __forceinline__ void operator()(uint32_t n, uint32_t off, uint32_t) const { rays[2 * n] = (int32_t)off; }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// training composite: one wave per ray, 64 samples per iteration
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_incl_scan_add(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float u = __shfl_up(v, d, 64);
        if (lane >= d) v = v + u;
    }
    return v;
}
__device__ __forceinline__ float wave_incl_scan_mul(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float u = __shfl_up(v, d, 64);
        if (lane >= d) v = v * u;
    }
    return v;
}
__device__ __forceinline__ float lane63(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }

// State of a ray between 64-sample chunks: transmittance and running sums (colour channels, weight sum, depth).  Wave-uniform.
template <int NC>
struct Carry {
    float T, acc[NC], ws, d;
};

// Per-lane values of one chunk.  keep: the lane's sample is composited (inside the ray and not after the stop sample).
template <int NC>
struct Lane {
    float sigma, ts0, ts1, rgb[NC];
    float w, Tpost, acc[NC], ws, d;
    bool keep;
};

// Composites samples [base, base+64) of a ray starting at `off` with `cnt` samples onto `c`; returns true when the ray stops (T < T_thresh)
// inside this chunk.  Identical code in the forward and the backward pass.
template <int NC>
__device__ __forceinline__ bool composite_chunk(const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ ts,
                                                uint32_t off, uint32_t cnt, uint32_t base, float T_thresh, bool binarize, Carry<NC>& c,
                                                Lane<NC>& L) {
    const int lane = dwg_lane();
    const uint32_t i = base + lane;
    const bool in = i < cnt;
    const size_t g = (size_t)off + i;
    L.sigma = 0.f; L.ts0 = 0.f; L.ts1 = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) L.rgb[k] = 0.f;
    if (in) {
        L.sigma = sigmas[g];
        const float2 t2 = *reinterpret_cast<const float2*>(ts + 2 * g);
        L.ts0 = t2.x; L.ts1 = t2.y;
        if (NC == 4) {
            const float4 q = *reinterpret_cast<const float4*>(rgbs + 4 * g);
            L.rgb[0] = q.x; L.rgb[1] = q.y; L.rgb[2] = q.z; L.rgb[NC - 1] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < NC; ++k) L.rgb[k] = rgbs[NC * g + k];
        }
    }
    const float real_alpha = 1.f - expf(-L.sigma * L.ts1);
    const float alpha = binarize ? (real_alpha > 0.5f ? 1.f : 0.f) : real_alpha;
    const float om = in ? 1.f - alpha : 1.f;
    const float P = wave_incl_scan_mul(om, lane);
    float Pex = __shfl_up(P, 1, 64);
    if (lane == 0) Pex = 1.f;
    const float Tpre = c.T * Pex;
    L.Tpost = Tpre * om;
    const unsigned long long stop = __ballot(in && L.Tpost < T_thresh);
    const int f = stop ? __builtin_ctzll(stop) : 64;
    L.keep = in && lane <= f;
    L.w = L.keep ? alpha * Tpre : 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        L.acc[k] = c.acc[k] + wave_incl_scan_add(L.w * L.rgb[k], lane);
        c.acc[k] = lane63(L.acc[k]);
    }
    L.ws = c.ws + wave_incl_scan_add(L.w, lane);
    c.ws = lane63(L.ws);
    L.d = c.d + wave_incl_scan_add(L.w * L.ts0, lane);
    c.d = lane63(L.d);
    c.T = lane63(L.Tpost);
    return stop != 0ull;
}

template <int NC>
__device__ __forceinline__ bool ray_ok(const int32_t* rays, uint32_t n, uint32_t M, uint32_t& off, uint32_t& cnt) {
    off = (uint32_t)rays[2 * n];
    cnt = (uint32_t)rays[2 * n + 1];
    return cnt != 0 && off <= M && cnt <= M - off;
}

// The forward pass.  LIVE (dwg_raymarch_composite_rays_train_forward_live): also live[n] = the number of leading samples of ray n that were
// composited (base + f + 1 in the chunk where the stop fires, cnt for a ray that never stops, 0 for a ray ray_ok rejects), and `weights`
// may be NULL.  Without LIVE `live` is not touched.
template <int NC, bool LIVE>
__global__ __launch_bounds__(256) void k_composite_fwd(const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                       const float* __restrict__ ts, const int32_t* __restrict__ rays, uint32_t M, uint32_t N,
                                                       float T_thresh, uint32_t binarize, float* __restrict__ weights,
                                                       float* __restrict__ weights_sum, float* __restrict__ depth, float* __restrict__ image,
                                                       int32_t* __restrict__ live) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = dwg_lane();
    for (uint32_t r = 0; r < kRaysPerWave; ++r) {
        const uint32_t n = wave * kRaysPerWave + r;
        if (n >= N) return;
        uint32_t off, cnt, used = 0;
        Carry<NC> c;
        c.T = 1.f; c.ws = 0.f; c.d = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) c.acc[k] = 0.f;
        if (ray_ok<NC>(rays, n, M, off, cnt)) {
            for (uint32_t base = 0; base < cnt; base += 64) {
                Lane<NC> L;
                const bool stop = composite_chunk<NC>(sigmas, rgbs, ts, off, cnt, base, T_thresh, binarize != 0, c, L);
                if (LIVE) {
                    if (L.keep && weights) weights[(size_t)off + base + lane] = L.w;
                    used = base + (uint32_t)__popcll(__ballot(L.keep));     // the kept lanes are 0..f, or every lane inside the ray
                } else {
                    if (L.keep) weights[(size_t)off + base + lane] = L.w;
                }
                if (stop) break;
            }
        }
        if (lane == 0) {
            weights_sum[n] = c.ws;
            depth[n] = c.d;
#pragma unroll
            for (int k = 0; k < NC; ++k) image[(size_t)NC * n + k] = c.acc[k];
            if (LIVE) live[n] = (int32_t)used;
        }
    }
}

template <int NC>
__global__ __launch_bounds__(256) void k_composite_bwd(const float* __restrict__ grad_weights, const float* __restrict__ grad_weights_sum,
                                                       const float* __restrict__ grad_depth, const float* __restrict__ grad_image,
                                                       const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                       const float* __restrict__ ts, const int32_t* __restrict__ rays,
                                                       const float* __restrict__ weights_sum, const float* __restrict__ depth,
                                                       const float* __restrict__ image, uint32_t M, uint32_t N, float T_thresh,
                                                       uint32_t binarize, float* __restrict__ grad_sigmas, float* __restrict__ grad_rgbs) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = dwg_lane();
    for (uint32_t r = 0; r < kRaysPerWave; ++r) {
        const uint32_t n = wave * kRaysPerWave + r;
        if (n >= N) return;
        uint32_t off, cnt;
        if (!ray_ok<NC>(rays, n, M, off, cnt)) continue;
        float gimg[NC], fin[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) { gimg[k] = grad_image[(size_t)NC * n + k]; fin[k] = image[(size_t)NC * n + k]; }
        const float gws = grad_weights_sum[n], gd = grad_depth[n], ws_final = weights_sum[n], d_final = depth[n];
        Carry<NC> c;
        c.T = 1.f; c.ws = 0.f; c.d = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k) c.acc[k] = 0.f;
        for (uint32_t base = 0; base < cnt; base += 64) {
            Lane<NC> L;
            const bool stop = composite_chunk<NC>(sigmas, rgbs, ts, off, cnt, base, T_thresh, binarize != 0, c, L);
            if (L.keep) {
                const size_t g = (size_t)off + base + lane;
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    grad_rgbs[NC * g + k] = gimg[k] * L.w;
                    const float term = gimg[k] * (L.Tpost * L.rgb[k] - (fin[k] - L.acc[k]));
                    s = k == 0 ? term : s + term;
                }
                s = s + (gws + grad_weights[g]) * (L.Tpost - (ws_final - L.ws));
                s = s + gd * (L.Tpost * L.ts0 - (d_final - L.d));
                grad_sigmas[g] = L.ts1 * s;
            }
            if (stop) break;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// inference
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void k_march_rays(MarchP p, uint32_t n_alive, uint32_t n_step, const int32_t* __restrict__ rays_alive,
                             const float* __restrict__ rays_t, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                             const float* __restrict__ nears, const float* __restrict__ fars, uint32_t N, float* __restrict__ xyzs,
                             float* __restrict__ dirs, float* __restrict__ ts, const float* __restrict__ noises) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int idx = rays_alive[n];
    if (idx < 0 || (uint32_t)idx >= N) return;
    const Ray r = load_ray(rays_o + 3 * (size_t)idx, rays_d + 3 * (size_t)idx);
    (void)nears;
    const float far = fars[idx];
    float t = start_t(p, rays_t[idx], noises[n]);
    uint32_t step = 0;
    float cx, cy, cz, dt;
    while (t < far && step < n_step) {
        if (march_iter(p, r, t, cx, cy, cz, dt)) {
            const size_t i = (size_t)n * n_step + step;
            xyzs[3 * i] = cx; xyzs[3 * i + 1] = cy; xyzs[3 * i + 2] = cz;
            dirs[3 * i] = r.dx; dirs[3 * i + 1] = r.dy; dirs[3 * i + 2] = r.dz;
            ts[2 * i] = t; ts[2 * i + 1] = dt;
            ++step;
        }
    }
}

template <int NC>
__global__ void k_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, uint32_t binarize, int32_t* __restrict__ rays_alive,
                                 float* __restrict__ rays_t, const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                 const float* __restrict__ ts, uint32_t N, float* __restrict__ weights_sum, float* __restrict__ depth,
                                 float* __restrict__ image) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int idx = rays_alive[n];
    if (idx < 0 || (uint32_t)idx >= N) return;
    float t = rays_t[idx];
    float d = depth[idx], ws = weights_sum[idx], col[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) col[k] = image[(size_t)NC * idx + k];
    uint32_t step = 0;
    while (step < n_step) {
        const size_t i = (size_t)n * n_step + step;
        if (ts[2 * i] == 0.f) break;
        t = ts[2 * i];
        float rgb[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) rgb[k] = rgbs[NC * i + k];
        if (composite_sample<NC>(sigmas[i], rgb, t, ts[2 * i + 1], T_thresh, binarize != 0, ws, d, col)) break;
        ++step;
    }
    if (step < n_step) rays_alive[n] = -1;
    else rays_t[idx] = t;
    weights_sum[idx] = ws;
    depth[idx] = d;
#pragma unroll
    for (int k = 0; k < NC; ++k) image[(size_t)NC * idx + k] = col[k];
}

inline dim3 grid1d(uint32_t n, uint32_t bs) { return dim3((n + bs - 1) / bs); }

// The checks and the channel dispatch of the two training-composite forwards.  The plain one wants `weights` when there are samples;
// LIVE wants `live` and takes weights == NULL.
template <bool LIVE>
int composite_fwd(const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, uint32_t M, uint32_t N, uint32_t channels,
                  float T_thresh, uint32_t binarize, float* weights, float* weights_sum, float* depth, float* image, int32_t* live,
                  dwg_stream_t stream) {
    if (channels != 3 && channels != 4) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (!rays || !weights_sum || !depth || !image || (LIVE && !live)) return DWG_E_ARG;
    if (M != 0 && (!sigmas || !rgbs || !ts || (!LIVE && !weights))) return DWG_E_ARG;
    if (((uintptr_t)ts & 7) || (channels == 4 && ((uintptr_t)rgbs & 15))) return DWG_E_ARG;
    const uint32_t waves = (N + kRaysPerWave - 1) / kRaysPerWave;
    const auto kernel = channels == 3 ? k_composite_fwd<3, LIVE> : k_composite_fwd<4, LIVE>;
    DWG_LAUNCH_W(LIVE ? "rm_composite_fwd_live" : "rm_composite_fwd", "k_composite_fwd", 0.0, kernel, dim3((waves + 3) / 4), dim3(256), 0,
                 (hipStream_t)stream, sigmas, rgbs, ts, rays, M, N, T_thresh, binarize, weights, weights_sum, depth, image, live);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // namespace

extern "C" {

int dwg_raymarch_near_far_from_aabb(const float* rays_o, const float* rays_d, const float* aabb, uint32_t N, float min_near, float* nears,
                                    float* fars, dwg_stream_t stream) {
    if (N == 0) return DWG_OK;
    if (!rays_o || !rays_d || !aabb || !nears || !fars) return DWG_E_ARG;
    DWG_LAUNCH("rm_near_far", k_near_far, grid1d(N, 256), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, aabb, N, min_near, nears, fars);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords, dwg_stream_t stream) {
    if (N == 0) return DWG_OK;
    if (!rays_o || !rays_d || !coords) return DWG_E_ARG;
    DWG_LAUNCH("rm_sph_from_ray", k_sph_from_ray, grid1d(N, 256), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, radius, N, coords);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_morton3d(const int32_t* coords, uint32_t N, int32_t* indices, dwg_stream_t stream) {
    if (N == 0) return DWG_OK;
    if (!coords || !indices) return DWG_E_ARG;
    DWG_LAUNCH("rm_morton3d", k_morton3d, grid1d(N, 256), dim3(256), 0, (hipStream_t)stream, coords, N, indices);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_morton3d_invert(const int32_t* indices, uint32_t N, int32_t* coords, dwg_stream_t stream) {
    if (N == 0) return DWG_OK;
    if (!coords || !indices) return DWG_E_ARG;
    DWG_LAUNCH("rm_morton3d_invert", k_morton3d_invert, grid1d(N, 256), dim3(256), 0, (hipStream_t)stream, indices, N, coords);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_packbits(const float* grid, uint32_t N, float density_thresh, uint8_t* bitfield, dwg_stream_t stream) {
    if (N == 0) return DWG_OK;
    if (!grid || !bitfield || ((uintptr_t)grid & 15)) return DWG_E_ARG;
    DWG_LAUNCH("rm_packbits", k_packbits<float>, grid1d(N, 256), dim3(256), 0, (hipStream_t)stream, (const float4*)grid, N, density_thresh,
               bitfield);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_packbits_dev(const float* grid, uint32_t N, const float* density_thresh, uint8_t* bitfield, dwg_stream_t stream) {
    if (N == 0) return DWG_OK;
    if (!grid || !density_thresh || !bitfield || ((uintptr_t)grid & 15)) return DWG_E_ARG;
    DWG_LAUNCH("occ_packbits", k_packbits<const float*>, grid1d(N, 256), dim3(256), 0, (hipStream_t)stream, (const float4*)grid, N,
               density_thresh, bitfield);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_flatten_rays(const int32_t* rays, uint32_t N, uint32_t M, int32_t* res, dwg_stream_t stream) {
    if (N == 0 || M == 0) return DWG_OK;
    if (!rays || !res) return DWG_E_ARG;
    DWG_LAUNCH("rm_flatten_rays", k_flatten_rays, grid1d(N, 256), dim3(256), 0, (hipStream_t)stream, rays, N, M, res);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_raymarch_train_workspace_bytes(uint32_t N) { return scan_workspace_bytes(N); }

int dwg_raymarch_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid, float bound, uint32_t contract,
                                  float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, const float* nears,
                                  const float* fars, float* xyzs, float* dirs, float* ts, uint32_t M, int32_t* rays, int32_t* counter,
                                  const float* noises, void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    if (!march_args_ok(bound, max_steps, C, H)) return DWG_E_ARG;
    if (!counter) return DWG_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (xyzs == nullptr) {
        if (dirs || ts) return DWG_E_ARG;
        if (N == 0) return DWG_OK;               // no rays: counter unchanged
        if (!rays_o || !rays_d || !grid || !nears || !fars || !rays || !noises) return DWG_E_ARG;
        if (!workspace || workspace_bytes < dwg_raymarch_train_workspace_bytes(N)) return DWG_E_CAPACITY;
        const MarchP p = make_march(grid, bound, contract, dt_gamma, max_steps, C, H);
        DWG_LAUNCH("rm_march_count", k_march_count, grid1d(N, 128), dim3(128), 0, st, p, rays_o, rays_d, nears, fars, noises, N, max_steps,
                   rays);
        scan_counts({"rm_scan_block_sums", "rm_scan_sums", "rm_scan_down"}, RayCount{rays}, RayOffset{rays}, N, (uint32_t*)workspace,
                    (uint32_t*)counter, true, st);                  // the offsets start from counter[0], which receives the total
        DWG_RETURN_IF_LAUNCH_FAILED();
        return DWG_OK;
    }
    if (!dirs || !ts) return DWG_E_ARG;
    if (N == 0 || M == 0) return DWG_OK;
    if (!rays_o || !rays_d || !grid || !nears || !fars || !rays || !noises || ((uintptr_t)ts & 7)) return DWG_E_ARG;
    const MarchP p = make_march(grid, bound, contract, dt_gamma, max_steps, C, H);
    DWG_LAUNCH("rm_march_write", k_march_write, grid1d(N, 128), dim3(128), 0, st, p, rays_o, rays_d, nears, fars, noises, N, M, rays, xyzs,
               dirs, ts);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_composite_rays_train_forward(const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, uint32_t M,
                                              uint32_t N, uint32_t channels, float T_thresh, uint32_t binarize, float* weights,
                                              float* weights_sum, float* depth, float* image, dwg_stream_t stream) {
    return composite_fwd<false>(sigmas, rgbs, ts, rays, M, N, channels, T_thresh, binarize, weights, weights_sum, depth, image, nullptr, stream);
}

int dwg_raymarch_composite_rays_train_forward_live(const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays, uint32_t M,
                                                   uint32_t N, uint32_t channels, float T_thresh, uint32_t binarize, float* weights,
                                                   float* weights_sum, float* depth, float* image, int32_t* live, dwg_stream_t stream) {
    return composite_fwd<true>(sigmas, rgbs, ts, rays, M, N, channels, T_thresh, binarize, weights, weights_sum, depth, image, live, stream);
}

int dwg_raymarch_composite_rays_train_backward(const float* grad_weights, const float* grad_weights_sum, const float* grad_depth,
                                               const float* grad_image, const float* sigmas, const float* rgbs, const float* ts,
                                               const int32_t* rays, const float* weights_sum, const float* depth, const float* image,
                                               uint32_t M, uint32_t N, uint32_t channels, float T_thresh, uint32_t binarize,
                                               float* grad_sigmas, float* grad_rgbs, dwg_stream_t stream) {
    if (channels != 3 && channels != 4) return DWG_E_ARG;
    if (N == 0 || M == 0) return DWG_OK;
    if (!grad_weights || !grad_weights_sum || !grad_depth || !grad_image || !sigmas || !rgbs || !ts || !rays || !weights_sum || !depth ||
        !image || !grad_sigmas || !grad_rgbs)
        return DWG_E_ARG;
    if (((uintptr_t)ts & 7) || (channels == 4 && ((uintptr_t)rgbs & 15))) return DWG_E_ARG;
    const uint32_t waves = (N + kRaysPerWave - 1) / kRaysPerWave;
    const dim3 g((waves + 3) / 4);
    if (channels == 3)
        DWG_LAUNCH("rm_composite_bwd", k_composite_bwd<3>, g, dim3(256), 0, (hipStream_t)stream, grad_weights, grad_weights_sum, grad_depth,
                   grad_image, sigmas, rgbs, ts, rays, weights_sum, depth, image, M, N, T_thresh, binarize, grad_sigmas, grad_rgbs);
    else
        DWG_LAUNCH("rm_composite_bwd", k_composite_bwd<4>, g, dim3(256), 0, (hipStream_t)stream, grad_weights, grad_weights_sum, grad_depth,
                   grad_image, sigmas, rgbs, ts, rays, weights_sum, depth, image, M, N, T_thresh, binarize, grad_sigmas, grad_rgbs);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t, const float* rays_o,
                            const float* rays_d, float bound, uint32_t contract, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                            const uint8_t* grid, const float* nears, const float* fars, uint32_t N, float* xyzs, float* dirs, float* ts,
                            const float* noises, dwg_stream_t stream) {
    if (!march_args_ok(bound, max_steps, C, H)) return DWG_E_ARG;
    if (n_alive == 0 || n_step == 0) return DWG_OK;
    if (!rays_alive || !rays_t || !rays_o || !rays_d || !grid || !fars || !xyzs || !dirs || !ts || !noises) return DWG_E_ARG;
    const MarchP p = make_march(grid, bound, contract, dt_gamma, max_steps, C, H);
    DWG_LAUNCH("rm_march_rays", k_march_rays, grid1d(n_alive, 128), dim3(128), 0, (hipStream_t)stream, p, n_alive, n_step, rays_alive, rays_t,
               rays_o, rays_d, nears, fars, N, xyzs, dirs, ts, noises);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_raymarch_composite_rays(uint32_t n_alive, uint32_t n_step, uint32_t channels, float T_thresh, uint32_t binarize, int32_t* rays_alive,
                                float* rays_t, const float* sigmas, const float* rgbs, const float* ts, uint32_t N, float* weights_sum,
                                float* depth, float* image, dwg_stream_t stream) {
    if (channels != 3 && channels != 4) return DWG_E_ARG;
    if (n_alive == 0 || n_step == 0) return DWG_OK;
    if (!rays_alive || !rays_t || !sigmas || !rgbs || !ts || !weights_sum || !depth || !image) return DWG_E_ARG;
    if (channels == 3)
        DWG_LAUNCH("rm_composite_rays", k_composite_rays<3>, grid1d(n_alive, 128), dim3(128), 0, (hipStream_t)stream, n_alive, n_step,
                   T_thresh, binarize, rays_alive, rays_t, sigmas, rgbs, ts, N, weights_sum, depth, image);
    else
        DWG_LAUNCH("rm_composite_rays", k_composite_rays<4>, grid1d(n_alive, 128), dim3(128), 0, (hipStream_t)stream, n_alive, n_step,
                   T_thresh, binarize, rays_alive, rays_t, sigmas, rgbs, ts, N, weights_sum, depth, image);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
