// occupancy.hip -- the occupancy-grid update of the NeRF stage (boundary B13, include/dwg_occupancy.h): the reference's statements
// nerf_renderer.py:137-147 (decayed maximum, mean / min / max of the valid cells, min(mean, density_thresh), packbits) as three launches
// with no host round trip, and the materialised cell points.  The density pass itself is nerf_field.hip's k_nf_occupancy.
//   k_occ_ema       grid-strided over float4s; every lane keeps (count, fp64 sum, min, max, NaN seen) of the valid cells it updated, a
//                   wave folds its lanes with shuffles, thread 0 folds the four waves in order -> one partial per workgroup
//   k_occ_finalize  one workgroup: thread t folds partials t, t + 256, ... in order, then the same wave / workgroup fold -> stats [8]
//   packbits        dwg_raymarch_packbits_dev of raymarch.hip: its k_packbits with the threshold read from stats
// The assignment of cells to lanes depends on C and H alone and every fold has a fixed order, so the statistics are bit-reproducible.
// No atomics.
#include <math.h>

#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_occupancy.h"
#include "../../include/dwg_raymarch.h"
#include "occupancy_common.h"

namespace {

constexpr uint32_t OCC_MAX_WG = 1024;       // partials of the EMA pass (4 workgroups per CU)

struct OccPartial {
    double sum;
    uint64_t count;
    float lo, hi;
    uint32_t nan, pad;
};

__device__ __forceinline__ void occ_fold(OccPartial& a, const OccPartial& b) {
    a.sum += b.sum; a.count += b.count; a.lo = fminf(a.lo, b.lo); a.hi = fmaxf(a.hi, b.hi); a.nan |= b.nan;
}

// lanes -> wave (lane 0 holds it) -> workgroup (thread 0 holds it); red: one slot per wave
__device__ __forceinline__ void occ_fold_workgroup(OccPartial& v, OccPartial* red) {
    for (int off = 32; off > 0; off >>= 1) {
        OccPartial o;
        o.sum = __shfl_down(v.sum, off);
        o.count = ((uint64_t)__shfl_down((unsigned)(v.count >> 32), off) << 32) | (uint64_t)__shfl_down((unsigned)v.count, off);
        o.lo = __shfl_down(v.lo, off); o.hi = __shfl_down(v.hi, off); o.nan = __shfl_down(v.nan, off);
        occ_fold(v, o);
    }
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < blockDim.x / 64u; w++) occ_fold(v, red[w]);
    }
}

__device__ __forceinline__ void occ_cell(float& g, float t, float decay, OccPartial& v) {
    if (!(g >= 0.f)) return;                                // invalid (negative or NaN): left as it is, out of the statistics
    const float a = g * decay;
    const bool nan = a != a || t != t;
    const float r = nan ? NAN : (a < t ? t : a);            // torch.maximum
    g = r;
    v.count++;
    v.sum += (double)r;
    if (nan) v.nan = 1u;
    else { v.lo = fminf(v.lo, r); v.hi = fmaxf(v.hi, r); }
}

__global__ __launch_bounds__(256) void k_occ_ema(float4* __restrict__ grid, const float4* __restrict__ tmp, uint32_t n4, float decay,
                                                 OccPartial* __restrict__ partial) {
    __shared__ OccPartial red[4];
    OccPartial v{0.0, 0ull, INFINITY, -INFINITY, 0u, 0u};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        float4 g = grid[i];
        const float4 t = tmp[i];
        occ_cell(g.x, t.x, decay, v); occ_cell(g.y, t.y, decay, v); occ_cell(g.z, t.z, decay, v); occ_cell(g.w, t.w, decay, v);
        grid[i] = g;
    }
    occ_fold_workgroup(v, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

__device__ __forceinline__ float occ_log_clamp(float v) {
    const float l = logf(v);
    return l != l ? l : fminf(15.f, fmaxf(-15.f, l));       // torch.clamp keeps NaN
}

__global__ __launch_bounds__(256) void k_occ_finalize(const OccPartial* __restrict__ partial, uint32_t G, float density_thresh, float* __restrict__ stats) {
    __shared__ OccPartial red[4];
    OccPartial v{0.0, 0ull, INFINITY, -INFINITY, 0u, 0u};
    for (uint32_t i = threadIdx.x; i < G; i += 256u) occ_fold(v, partial[i]);
    occ_fold_workgroup(v, red);
    if (threadIdx.x != 0) return;
    const float mean = (float)(v.sum / (double)v.count);
    const float lo = v.nan ? NAN : v.lo, hi = v.nan ? NAN : v.hi;
    stats[0] = mean; stats[1] = lo; stats[2] = hi;
    stats[3] = occ_log_clamp(lo); stats[4] = occ_log_clamp(hi);
    stats[5] = density_thresh < mean ? density_thresh : mean;       // Python's min(mean, density_thresh)
    stats[6] = __uint_as_float((uint32_t)v.count); stats[7] = __uint_as_float((uint32_t)(v.count >> 32));
}

__global__ void k_occ_points(OccLattice l, uint64_t n3, float* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3) return;
    const uint32_t g = (uint32_t)(e / 3u);
    out[e] = occ_point(l, g, (uint32_t)(e - 3ull * g));
}

uint32_t occ_groups(uint32_t n4) { const uint32_t g = (n4 + 255u) / 256u; return g < OCC_MAX_WG ? g : OCC_MAX_WG; }

}  // namespace

extern "C" {

int dwg_occ_lattice_points(const float* axis, const float* noise, const float* scale, const float* half, uint32_t C, uint32_t H,
                           float* points_out, dwg_stream_t stream) {
    uint32_t lg = 0;
    if (!occ_limits(C, H, lg)) return DWG_E_ARG;
    if (!axis || !noise || !scale || !half || !points_out) return DWG_E_ARG;
    const uint64_t n3 = ((uint64_t)C << (3u * lg)) * 3ull;              // < 3 * 2^32; blocks of 256: below 2^31
    DWG_LAUNCH("occ_lattice_points", k_occ_points, dim3((unsigned)((n3 + 255ull) / 256ull)), dim3(256), 0, (hipStream_t)stream,
               OccLattice{axis, noise, scale, half, lg}, n3, points_out);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_occ_update_workspace_bytes(uint32_t C, uint32_t H) {
    uint32_t lg = 0;
    if (!occ_limits(C, H, lg)) return 0;
    return (size_t)occ_groups((uint32_t)(((uint64_t)C << (3u * lg)) / 4u)) * sizeof(OccPartial);
}

int dwg_occ_update(float* density_grid, const float* tmp_grid, uint32_t C, uint32_t H, float decay, float density_thresh, uint8_t* bitfield,
                   float* stats, void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    uint32_t lg = 0;
    if (!occ_limits(C, H, lg)) return DWG_E_ARG;
    if (!density_grid || !tmp_grid || !bitfield || !stats || !workspace) return DWG_E_ARG;
    if (((uintptr_t)density_grid & 15) || ((uintptr_t)tmp_grid & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)stats & 3)) return DWG_E_ARG;
    if (workspace_bytes < dwg_occ_update_workspace_bytes(C, H)) return DWG_E_CAPACITY;
    const uint64_t N = (uint64_t)C << (3u * lg);
    const uint32_t n4 = (uint32_t)(N / 4u), G = occ_groups(n4);
    OccPartial* partial = reinterpret_cast<OccPartial*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    DWG_LAUNCH("occ_ema", k_occ_ema, dim3(G), dim3(256), 0, st, (float4*)density_grid, (const float4*)tmp_grid, n4, decay, partial);
    DWG_RETURN_IF_LAUNCH_FAILED();
    DWG_LAUNCH("occ_finalize", k_occ_finalize, dim3(1), dim3(256), 0, st, (const OccPartial*)partial, G, density_thresh, stats);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return dwg_raymarch_packbits_dev(density_grid, (uint32_t)(N / 8u), stats + 5, bitfield, stream);
}

}  // extern "C"
