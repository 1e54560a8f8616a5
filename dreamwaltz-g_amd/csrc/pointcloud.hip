// pointcloud.hip -- the NeRF stage's point-cloud export (boundary B12, include/dwg_pointcloud.h) around the fused field of
// nerf_field.hip: ordered selection of the lattice points above the density threshold, their coordinates, the shifted points of the
// finite-difference normal, colours and normals of the survivors, and the bounding-box keep mask.
//
// The selection is deterministic by construction: a block takes SEL_BLOCK consecutive entries as SEL_ITERS rounds of 256 (round-major,
// so ascending in memory), every wave counts a round's survivors with ballot + popcount, the block counts are scanned by one workgroup
// (k_scan_sums of scan_common.h, shared with raymarch.hip and nerf_train.hip), and the write pass gives each surviving lane the slot
// block base + (rounds and waves before it) + lanes below it in the ballot.
// No atomic decides a slot.  The pointwise kernels are one lane per output element (or per point where a point's outputs depend on
// each other); nothing here uses LDS beyond the scans' few words.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_pointcloud.h"
#include "fd_normal.h"
#include "pointcloud_index.h"
#include "scan_common.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_ITERS = 8;
constexpr uint32_t SEL_BLOCK = SEL_THREADS * SEL_ITERS;       // entries per block

struct AboveF32 {
    const float* __restrict__ v;
    float thresh;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return v[i] > thresh; }      // false for NaN
};
struct FlagU8 {
    const uint8_t* __restrict__ f;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return f[i] != 0; }
};

__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// survivors of this block per (round, wave) -> cnt[SEL_ITERS * SEL_WAVES]; returns this lane's predicate bits (bit j: round j) and
// fills below[j] with the surviving lanes below it in its wave in round j
template <typename P>
__device__ __forceinline__ uint32_t sel_count(const P& pred, uint64_t M, uint32_t* cnt, uint32_t* below) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t base = (uint64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < SEL_ITERS; j++) {
        const uint64_t i = base + (uint64_t)j * SEL_THREADS;
        const bool s = i < M && pred(i);
        const unsigned long long b = __ballot(s);
        if (below) below[j] = lanes_below(b);
        if (s) bits |= 1u << j;
        if (lane == 0) cnt[j * SEL_WAVES + wave] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    return bits;
}

template <typename P>
__global__ __launch_bounds__(SEL_THREADS) void k_sel_block_sums(P pred, uint64_t M, uint32_t* __restrict__ sums) {
    __shared__ uint32_t cnt[SEL_ITERS * SEL_WAVES];
    sel_count(pred, M, cnt, nullptr);
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int k = 0; k < SEL_ITERS * SEL_WAVES; k++) s += cnt[k];
        sums[blockIdx.x] = s;
    }
}

template <typename P>
__global__ __launch_bounds__(SEL_THREADS) void k_sel_write(P pred, uint64_t M, const uint32_t* __restrict__ sums, uint32_t* __restrict__ idx_out,
                                                           uint64_t capacity) {
    __shared__ uint32_t cnt[SEL_ITERS * SEL_WAVES];
    uint32_t below[SEL_ITERS];
    const uint32_t bits = sel_count(pred, M, cnt, below);
    if (threadIdx.x == 0) {                                     // exclusive scan over (round, wave): the order of the entries in memory
        uint32_t s = 0;
        for (int k = 0; k < SEL_ITERS * SEL_WAVES; k++) { const uint32_t c = cnt[k]; cnt[k] = s; s += c; }
    }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * SEL_BLOCK + threadIdx.x;
    const uint64_t bbase = sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SEL_ITERS; j++) {
        if (bits & (1u << j)) {
            const uint64_t slot = bbase + cnt[j * SEL_WAVES + wave] + below[j];
            if (slot < capacity) idx_out[slot] = (uint32_t)(base + (uint64_t)j * SEL_THREADS);
        }
    }
}

__global__ __launch_bounds__(256) void k_pc_lattice_points(uint64_t n3, const uint32_t* __restrict__ idx, PcLattice l, uint32_t M,
                                                           const float* __restrict__ ax, const float* __restrict__ ay,
                                                           const float* __restrict__ az, float* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n3) return;
    const uint64_t pt = e / 3u;
    const uint32_t k = (uint32_t)(e - 3u * pt), f = idx[pt];
    float v = __builtin_nanf("");
    if (f < M) {
        uint32_t ix, iy, iz;
        pc_lattice_decode(l, f, ix, iy, iz);
        v = k == 0 ? ax[ix] : k == 1 ? ay[iy] : az[iz];
    }
    out[e] = v;
}

__global__ __launch_bounds__(256) void k_pc_fd_points(uint64_t n3, const float* __restrict__ points, float eps, float bound, float* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= 6u * n3) return;
    const uint32_t s = (uint32_t)(e / n3);                      // 0 .. 5: +x, -x, +y, -y, +z, -z
    const uint64_t r = e - (uint64_t)s * n3;
    out[e] = fd_shift(points[r], (uint32_t)(r % 3u), s, eps, bound);
}

__global__ __launch_bounds__(256) void k_pc_finish(uint64_t n, uint32_t C, const float* __restrict__ albedo, const float* __restrict__ sig6,
                                                   float eps, float* __restrict__ colors, float* __restrict__ normals) {
    // every product and every sum below is rounded on its own, as the torch statements this restates do.  The compiler contracts
    // a * b + c by default, and HIP's __fmul_rn / __fadd_rn are plain operators that it contracts all the same.
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (C == 3u) {
        for (int j = 0; j < 3; j++) colors[3u * i + j] = albedo[3u * i + j];
    } else {
        // latent_to_rgb's decode matrix (to_point_cloud.py:16-22), rows L1..L4, columns R G B
        const float m[4][3] = {{0.298f, 0.207f, 0.208f}, {0.187f, 0.286f, 0.173f}, {-0.158f, 0.189f, 0.264f}, {-0.184f, -0.271f, -0.473f}};
        const float4 a = *reinterpret_cast<const float4*>(albedo + 4u * i);
        // products rounded one by one and summed in k order
        for (int j = 0; j < 3; j++) colors[3u * i + j] = ((a.x * m[0][j] + a.y * m[1][j]) + a.z * m[2][j]) + a.w * m[3][j];
    }
    const float s[6] = {sig6[i], sig6[n + i], sig6[2u * n + i], sig6[3u * n + i], sig6[4u * n + i], sig6[5u * n + i]};
    shade_normal(s, eps, normals + 3u * i);
}

__global__ __launch_bounds__(256) void k_pc_outside_boxes(uint64_t n, const float* __restrict__ points, uint32_t nb, const double* __restrict__ boxes,
                                                          uint8_t* __restrict__ keep) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double x = (double)points[3u * i], y = (double)points[3u * i + 1u], z = (double)points[3u * i + 2u];
    uint8_t k = 1;
    for (uint32_t b = 0; b < nb; b++) {
        const double* c = boxes + 6u * b;
        if (x >= c[0] && y >= c[1] && z >= c[2] && x <= c[3] && y <= c[4] && z <= c[5]) { k = 0; break; }
    }
    keep[i] = k;
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255u) / 256u); }
constexpr uint64_t MAX_ELEMS = 256ull * 0x7fffffffull;          // one lane per element, 256 per block, 2^31 - 1 blocks

template <typename P>
int select(const P& pred, uint64_t M, uint32_t* idx_out, uint64_t capacity, uint32_t* count_out, void* workspace, size_t workspace_bytes,
           dwg_stream_t stream) {
    const uint32_t nb = (uint32_t)((M + SEL_BLOCK - 1) / SEL_BLOCK);
    uint32_t* sums = reinterpret_cast<uint32_t*>(workspace);
    hipStream_t st = (hipStream_t)stream;
    DWG_LAUNCH("pc_select_block_sums", k_sel_block_sums<P>, dim3(nb), dim3(SEL_THREADS), 0, st, pred, M, sums);
    DWG_LAUNCH("pc_select_scan_sums", k_scan_sums, dim3(1), dim3(kScanSumsThreads), 0, st, sums, nb, count_out, 0u);
    DWG_LAUNCH("pc_select_write", k_sel_write<P>, dim3(nb), dim3(SEL_THREADS), 0, st, pred, M, (const uint32_t*)sums, idx_out, capacity);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int select_args(uint64_t M, const void* in, const uint32_t* idx_out, const uint32_t* count_out, const void* workspace, size_t workspace_bytes) {
    if (M >= (1ull << 32)) return DWG_E_ARG;
    if (M == 0) return DWG_OK;
    if (!in || !idx_out || !count_out || !workspace || ((uintptr_t)workspace & 3u)) return DWG_E_ARG;
    if (workspace_bytes < dwg_pc_select_workspace_bytes(M)) return DWG_E_CAPACITY;
    return DWG_OK;
}

}  // namespace

extern "C" {

size_t dwg_pc_select_workspace_bytes(uint64_t M) {
    if (M == 0 || M >= (1ull << 32)) return 0;
    return (size_t)((M + SEL_BLOCK - 1) / SEL_BLOCK) * sizeof(uint32_t);
}

int dwg_pc_select_above(uint64_t M, const float* values, float thresh, uint32_t* idx_out, uint64_t capacity, uint32_t* count_out,
                        void* workspace, size_t workspace_bytes, dwg_stream_t stream) {
    const int rc = select_args(M, values, idx_out, count_out, workspace, workspace_bytes);
    if (rc || M == 0) return rc;
    return select(AboveF32{values, thresh}, M, idx_out, capacity, count_out, workspace, workspace_bytes, stream);
}

int dwg_pc_select_flags(uint64_t M, const uint8_t* flags, uint32_t* idx_out, uint64_t capacity, uint32_t* count_out, void* workspace,
                        size_t workspace_bytes, dwg_stream_t stream) {
    const int rc = select_args(M, flags, idx_out, count_out, workspace, workspace_bytes);
    if (rc || M == 0) return rc;
    return select(FlagU8{flags}, M, idx_out, capacity, count_out, workspace, workspace_bytes, stream);
}

int dwg_pc_lattice_points(uint64_t n, const uint32_t* idx, const float* ax, const float* ay, const float* az, uint32_t nx, uint32_t ny,
                          uint32_t nz, uint32_t split, float* points_out, dwg_stream_t stream) {
    const uint64_t M = (uint64_t)nx * ny * nz;
    if (split == 0 || (uint64_t)nx * ny >= (1ull << 32) || M >= (1ull << 32) || n > MAX_ELEMS / 3u) return DWG_E_ARG;
    if (n == 0) return DWG_OK;
    if (!idx || !points_out) return DWG_E_ARG;
    if (M && (!ax || !ay || !az)) return DWG_E_ARG;
    const PcLattice l = M ? pc_lattice(nx, ny, nz, split) : PcLattice{1u, 1u, 1u, 1u, 1u, 1u};      // M == 0: every index is out of range
    DWG_LAUNCH("pc_lattice_points", k_pc_lattice_points, dim3(blocks_for(3u * n)), dim3(256), 0, (hipStream_t)stream, 3u * n, idx, l,
               (uint32_t)M, ax, ay, az, points_out);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_pc_fd_points(uint64_t n, const float* points, float eps, float bound, float* out, dwg_stream_t stream) {
    if (!(bound >= 0.f) || eps != eps || n > MAX_ELEMS / 18u) return DWG_E_ARG;
    if (n == 0) return DWG_OK;
    if (!points || !out) return DWG_E_ARG;
    DWG_LAUNCH("pc_fd_points", k_pc_fd_points, dim3(blocks_for(18u * n)), dim3(256), 0, (hipStream_t)stream, 3u * n, points, eps, bound, out);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_pc_finish(uint64_t n, uint32_t C, const float* albedo, const float* sig6, float eps, float* colors_out, float* normals_out,
                  dwg_stream_t stream) {
    if ((C != 3u && C != 4u) || eps != eps || n > MAX_ELEMS) return DWG_E_ARG;
    if (n == 0) return DWG_OK;
    if (!albedo || !sig6 || !colors_out || !normals_out) return DWG_E_ARG;
    if (C == 4u && ((uintptr_t)albedo & 15u)) return DWG_E_ARG;
    DWG_LAUNCH("pc_finish", k_pc_finish, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, C, albedo, sig6, eps, colors_out, normals_out);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_pc_outside_boxes(uint64_t n, const float* points, uint32_t nb, const double* boxes, uint8_t* keep, dwg_stream_t stream) {
    if (n > MAX_ELEMS) return DWG_E_ARG;
    if (n == 0) return DWG_OK;
    if (!points || !keep || (nb && !boxes)) return DWG_E_ARG;
    DWG_LAUNCH("pc_outside_boxes", k_pc_outside_boxes, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, points, nb, boxes, keep);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
