// nerf_train.hip -- the training render of the NeRF stage for gfx950 (boundary B18, include/dwg_nerf_train.h): offsets of the samples
// the training composite used, and the gather that keeps only those for the backward.
//
// composite_rays_train (the reference's core/nerf/raymarching/rgb/src/raymarching.cu:541-569) stops a ray at the first sample after which
// T < T_thresh; its backward (:652-694) writes no gradient past it, and the field backward over those rows adds zeros.  raymarch.hip's
// k_composite_fwd<NC, LIVE> reports live[n], the count of leading samples ray n composited.  Here:
//   - scan_counts (scan_common.h, the deterministic three-launch exclusive scan that raymarch.hip's training march uses too) over
//     live[], written as (offset, live) pairs -- the `rays` layout the composite backward reads.
//   - k_nt_gather: one wave per ray (kRaysPerWave consecutive rays per wave, as the composite) walks the ray's live rows and copies the
//     elements of every per-sample array in its table of slots (GatherSlot: source, destination, elements per row, element size) from
//     the ray's range in the full buffers to its range in the live ones.  Consecutive lanes take consecutive elements of a contiguous
//     range: coalesced on both sides.  dwg_nerf_train_gather_live fills up to four slots, dwg_nerf_train_gather_live_rows one.
// Integer adds and bit-for-bit copies only: no float arithmetic, no atomics.
//
// The shaded training render (boundary B19) gathers one more per-sample array through the rows entry (the six shifted densities) and
// adds the two streaming kernels over shade_math.h, one sample per thread: k_nt_shade_fwd (six densities, albedo -> colour) and
// k_nt_shade_bwd (d colour -> d of the six densities, d albedo), which load a sample through one helper and launch through one
// function.  Per-sample arithmetic only: nothing is summed across samples.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_nerf_train.h"
#include "scan_common.h"
#include "shade_math.h"

namespace {

constexpr int kRaysPerWave = 4;

// the scan of the live counts (scan_common.h): the count of ray n is max(live[n], 0), the pair (offset, count) goes to rays_live[n]
struct LiveCount {
    const int32_t* live;
    __device__ __forceinline__ uint32_t operator()(uint32_t n) const {
        const int32_t v = live[n];
        return v > 0 ? (uint32_t)v : 0u;
    }
};
struct LivePair {
    int32_t* rays_live;
    __device__ __forceinline__ void operator()(uint32_t n, uint32_t off, uint32_t cnt) const {
        *reinterpret_cast<int2*>(rays_live + 2 * (size_t)n) = make_int2((int32_t)off, (int32_t)cnt);
    }
};

// rows [so, so + cnt) of src -> rows [dof, dof + cnt) of dst, `w` elements per row, as one contiguous range of elements
template <typename T>
__device__ __forceinline__ void copy_rows(const T* __restrict__ src, T* __restrict__ dst, size_t so, size_t dof, uint32_t cnt, uint32_t w,
                                          int lane) {
    const T* s = src + so * w;
    T* d = dst + dof * w;
    const size_t n = (size_t)cnt * w;
    for (size_t i = (size_t)lane; i < n; i += 64) d[i] = s[i];
}

// One per-sample array of the gather: rows of `w` elements of `esz` bytes -- 4, or 2 where a row may start on a half-word.
struct GatherSlot {
    const void* src; void* dst;
    uint32_t w, esz;
};
constexpr uint32_t kGatherSlots = 4;
struct GatherP {
    GatherSlot s[kGatherSlots];
    uint32_t n;                             // slots filled
};

__global__ __launch_bounds__(256) void k_nt_gather(GatherP p, const int32_t* __restrict__ rays, const int32_t* __restrict__ rays_live, uint32_t N,
                                                   uint32_t M, uint32_t M_live) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = dwg_lane();
    for (uint32_t r = 0; r < kRaysPerWave; ++r) {
        const uint32_t n = wave * kRaysPerWave + r;
        if (n >= N) return;
        const int2 src = *reinterpret_cast<const int2*>(rays + 2 * (size_t)n);
        const int2 dst = *reinterpret_cast<const int2*>(rays_live + 2 * (size_t)n);
        const uint32_t so = (uint32_t)src.x, sc = (uint32_t)src.y, dof = (uint32_t)dst.x, cnt = (uint32_t)dst.y;
        if (cnt == 0 || cnt > sc || so > M || sc > M - so || dof > M_live || cnt > M_live - dof) continue;
#pragma unroll
        for (uint32_t j = 0; j < kGatherSlots; ++j) {
            if (j >= p.n) break;
            const GatherSlot& g = p.s[j];
            if (g.esz == 2u) copy_rows<uint16_t>((const uint16_t*)g.src, (uint16_t*)g.dst, so, dof, cnt, g.w, lane);
            else copy_rows<uint32_t>((const uint32_t*)g.src, (uint32_t*)g.dst, so, dof, cnt, g.w, lane);
        }
    }
}

// What the two gather entry points share: the checks on the ray tables and the slots, and the launch.
int gather(const GatherP& p, const int32_t* rays, const int32_t* rays_live, uint32_t N, uint32_t M, uint32_t M_live, hipStream_t stream) {
    if (M_live > M) return DWG_E_ARG;
    if (N == 0 || M == 0 || M_live == 0) return DWG_OK;
    if (!rays || !rays_live || ((uintptr_t)rays & 7) || ((uintptr_t)rays_live & 7)) return DWG_E_ARG;
    for (uint32_t j = 0; j < p.n; ++j)
        if (!p.s[j].src || !p.s[j].dst || (((uintptr_t)p.s[j].src | (uintptr_t)p.s[j].dst) & (p.s[j].esz - 1))) return DWG_E_ARG;
    if (p.n == 0) return DWG_OK;
    const uint32_t waves = (N + kRaysPerWave - 1) / kRaysPerWave;
    DWG_LAUNCH("nt_gather", k_nt_gather, dim3((waves + 3) / 4), dim3(256), 0, stream, p, rays, rays_live, N, M, M_live);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

struct ShadeTrainP {
    uint32_t shading;                       // shade_math.h: DWG_SHADE_NORMAL, _TEXTURELESS, _LAMBERTIAN
    const float* light_d;                   // [3] on the device; read for the last two
    float ratio, one_minus_ratio, eps;
    uint32_t M, ch;
};

// What both shade kernels read of sample i: l = -light_d (the lambert shadings), the six densities, the albedo ('lambertian' only, which
// has three channels).  T: the albedo's type.
template <typename T>
__device__ __forceinline__ void shade_load(const ShadeTrainP& p, const float* __restrict__ sigma_fd, const T* __restrict__ albedo, uint32_t i,
                                           float (&l)[3], float (&s)[6], float (&alb)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) l[k] = p.shading >= DWG_SHADE_TEXTURELESS ? -p.light_d[k] : 0.f;
    const float2* sp = reinterpret_cast<const float2*>(sigma_fd) + 3 * (size_t)i;
    const float2 a = sp[0], b = sp[1], c = sp[2];
    s[0] = a.x; s[1] = a.y; s[2] = b.x; s[3] = b.y; s[4] = c.x; s[5] = c.y;
#pragma unroll
    for (int k = 0; k < 3; ++k) alb[k] = p.shading == DWG_SHADE_LAMBERTIAN ? (float)albedo[3 * (size_t)i + k] : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void k_nt_shade_fwd(ShadeTrainP p, const float* __restrict__ sigma_fd, const T* __restrict__ albedo,
                                                      float* __restrict__ rgbs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.M) return;
    float l[3], s[6], alb[3], n[3], rgb[3];
    shade_load(p, sigma_fd, albedo, i, l, s, alb);
    shade_normal(s, p.eps, n);
    shade_color(p.shading, p.ratio, p.one_minus_ratio, l[0], l[1], l[2], n[0], n[1], n[2], alb, 3, rgb);
    float* o = rgbs + (size_t)p.ch * i;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
    if (p.ch == 4u) o[3] = 0.f;                                                     // the reference's zero pad of a latent colour
}

template <typename T>
__global__ __launch_bounds__(256) void k_nt_shade_bwd(ShadeTrainP p, const float* __restrict__ sigma_fd, const T* __restrict__ albedo,
                                                      const float* __restrict__ grad_rgbs, float* __restrict__ dsigma_fd, T* __restrict__ dalbedo) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= p.M) return;
    float l[3], s[6], alb[3], ds[6], da[3] = {0.f, 0.f, 0.f};
    shade_load(p, sigma_fd, albedo, i, l, s, alb);
    const float* gp = grad_rgbs + (size_t)p.ch * i;
    const float g[3] = {gp[0], gp[1], gp[2]};                                       // a fourth channel is the pad's: dropped
    shade_backward(p.shading, p.ratio, p.one_minus_ratio, l[0], l[1], l[2], p.eps, s, alb, g, ds, da);
    float2* dp = reinterpret_cast<float2*>(dsigma_fd) + 3 * (size_t)i;
    dp[0] = make_float2(ds[0], ds[1]); dp[1] = make_float2(ds[2], ds[3]); dp[2] = make_float2(ds[4], ds[5]);
    if (dalbedo) {
        T* o = dalbedo + (size_t)p.ch * i;
        for (uint32_t k = 0; k < p.ch; ++k) o[k] = (T)(k < 3u ? da[k] : 0.f);
    }
}

// What the two shade entry points share: the checks (with M == 0 of the scalars only), the parameter block and the launch by the
// albedo's type.  grad_rgbs == NULL: the forward into out [M, ch]; else the backward into out [M, 6] and dalbedo.
int shade(uint32_t shading, const float* sigma_fd, const void* albedo, uint32_t albedo_f16, const float* light_d, float ratio, float eps, uint32_t M,
          uint32_t ch, const float* grad_rgbs, float* out, void* dalbedo, hipStream_t stream) {
    if (shading < DWG_SHADE_NORMAL || shading > DWG_SHADE_LAMBERTIAN || (ch != 3 && ch != 4) || albedo_f16 > 1) return DWG_E_ARG;
    if (!(eps > 0.f) || ratio != ratio) return DWG_E_ARG;
    if (shading == DWG_SHADE_LAMBERTIAN && ch != 3) return DWG_E_ARG;               // four albedo channels plus the pad: five into four
    if (M == 0) return DWG_OK;
    if (shading >= DWG_SHADE_TEXTURELESS && !light_d) return DWG_E_ARG;
    if (shading == DWG_SHADE_LAMBERTIAN && !albedo) return DWG_E_ARG;
    if (!sigma_fd || ((uintptr_t)sigma_fd & 7)) return DWG_E_ARG;
    const ShadeTrainP p{shading, light_d, ratio, (float)(1.0 - (double)ratio), eps, M, ch};
    const dim3 grid((M + 255u) / 256u);
    if (!grad_rgbs) {
        if (albedo_f16) DWG_LAUNCH("nt_shade_fwd", k_nt_shade_fwd<_Float16>, grid, dim3(256), 0, stream, p, sigma_fd, (const _Float16*)albedo, out);
        else DWG_LAUNCH("nt_shade_fwd", k_nt_shade_fwd<float>, grid, dim3(256), 0, stream, p, sigma_fd, (const float*)albedo, out);
    } else if (albedo_f16) {
        DWG_LAUNCH("nt_shade_bwd", k_nt_shade_bwd<_Float16>, grid, dim3(256), 0, stream, p, sigma_fd, (const _Float16*)albedo, grad_rgbs, out,
                   (_Float16*)dalbedo);
    } else {
        DWG_LAUNCH("nt_shade_bwd", k_nt_shade_bwd<float>, grid, dim3(256), 0, stream, p, sigma_fd, (const float*)albedo, grad_rgbs, out, (float*)dalbedo);
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // namespace

extern "C" {

size_t dwg_nerf_train_workspace_bytes(uint32_t N) { return scan_workspace_bytes(N); }

int dwg_nerf_train_compact_offsets(const int32_t* live, uint32_t N, int32_t* rays_live, int32_t* total, void* workspace,
                                   size_t workspace_bytes, dwg_stream_t stream) {
    if (N == 0) return DWG_OK;
    if (!live || !rays_live || !total || ((uintptr_t)rays_live & 7)) return DWG_E_ARG;
    if (!workspace || ((uintptr_t)workspace & 3)) return DWG_E_ARG;
    if (workspace_bytes < dwg_nerf_train_workspace_bytes(N)) return DWG_E_CAPACITY;
    scan_counts({"nt_block_sums", "nt_scan_sums", "nt_scan_down"}, LiveCount{live}, LivePair{rays_live}, N, (uint32_t*)workspace,
                (uint32_t*)total, false, (hipStream_t)stream);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_nerf_train_gather_live(const int32_t* rays, const int32_t* rays_live, uint32_t N, uint32_t M, uint32_t M_live, const float* xyzs,
                               float* xyzs_live, const float* ts, float* ts_live, const float* sigmas, float* sigmas_live, const void* rgbs,
                               void* rgbs_live, uint32_t channels, uint32_t rgbs_f16, dwg_stream_t stream) {
    if (channels != 3 && channels != 4) return DWG_E_ARG;
    if (rgbs_f16 > 1) return DWG_E_ARG;
    if (!xyzs != !xyzs_live || !ts != !ts_live || !sigmas != !sigmas_live || !rgbs != !rgbs_live) return DWG_E_ARG;
    // f16 colours: 8-byte latent rows are two words; 6-byte rgb rows start on any half-word
    const GatherSlot slots[kGatherSlots] = {{xyzs, xyzs_live, 3, 4}, {ts, ts_live, 2, 4}, {sigmas, sigmas_live, 1, 4},
                                            {rgbs, rgbs_live, rgbs_f16 ? (channels == 4 ? 2u : 3u) : channels, rgbs_f16 && channels == 3 ? 2u : 4u}};
    GatherP p{};
    for (const GatherSlot& s : slots)
        if (s.src) p.s[p.n++] = s;
    return gather(p, rays, rays_live, N, M, M_live, (hipStream_t)stream);
}

int dwg_nerf_train_gather_live_rows(const int32_t* rays, const int32_t* rays_live, uint32_t N, uint32_t M, uint32_t M_live, const float* src,
                                    float* dst, uint32_t floats_per_row, dwg_stream_t stream) {
    if (floats_per_row == 0 || floats_per_row > 64) return DWG_E_ARG;
    GatherP p{};
    p.s[p.n++] = {src, dst, floats_per_row, 4};
    return gather(p, rays, rays_live, N, M, M_live, (hipStream_t)stream);
}

int dwg_nerf_train_shade_forward(uint32_t shading, const float* sigma_fd, const void* albedo, uint32_t albedo_f16, const float* light_d,
                                 float ambient_ratio, float epsilon, uint32_t M, uint32_t channels, float* rgbs, dwg_stream_t stream) {
    if (M && (!rgbs || ((uintptr_t)rgbs & 3))) return DWG_E_ARG;
    return shade(shading, sigma_fd, albedo, albedo_f16, light_d, ambient_ratio, epsilon, M, channels, nullptr, rgbs, nullptr, (hipStream_t)stream);
}

int dwg_nerf_train_shade_backward(uint32_t shading, const float* sigma_fd, const void* albedo, uint32_t albedo_f16, const float* light_d,
                                  float ambient_ratio, float epsilon, uint32_t M, uint32_t channels, const float* grad_rgbs, float* dsigma_fd,
                                  void* dalbedo, dwg_stream_t stream) {
    if (M) {
        if (!grad_rgbs || !dsigma_fd || (((uintptr_t)grad_rgbs) & 3) || ((uintptr_t)dsigma_fd & 7)) return DWG_E_ARG;
        if (shading == DWG_SHADE_LAMBERTIAN && !dalbedo) return DWG_E_ARG;
        if ((uintptr_t)dalbedo & (albedo_f16 ? 1 : 3)) return DWG_E_ARG;
    }
    return shade(shading, sigma_fd, albedo, albedo_f16, light_d, ambient_ratio, epsilon, M, channels, grad_rgbs, dsigma_fd, dalbedo,
                 (hipStream_t)stream);
}

}  // extern "C"
