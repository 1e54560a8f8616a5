// scan_common.h -- the deterministic device-wide exclusive scan of 32-bit counts of the NeRF stage, as three launches: block sums ->
// one workgroup over the sums -> scan down.  Integer adds in a fixed order: no atomics, no cross-workgroup flags.
//   raymarch.hip    scan_counts over rays[:,1] of the training march's count pass (offsets into rays[:,0], total added to the counter)
//   nerf_train.hip  scan_counts over max(live[n], 0) (the (offset, count) pairs of rays_live, total overwritten)
//   pointcloud.hip  k_scan_sums alone, between its own ballot count and write passes (count overwritten)
#pragma once
#include <stdint.h>

#include "dwg_common.h"
#include "dwg_prof_internal.h"

constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;                       // 1024 items per scan block
constexpr int kScanBlock = kScanThreads * kScanItems;
constexpr int kScanSumsThreads = 1024;              // the one workgroup of k_scan_sums

inline uint32_t scan_blocks(uint32_t N) { return (N + kScanBlock - 1) / kScanBlock; }
inline size_t scan_workspace_bytes(uint32_t N) { return (size_t)scan_blocks(N) * sizeof(uint32_t); }

__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
    const int lane = dwg_lane();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// exclusive scan over the block (NT threads); *total = block sum.  lds: NT/64 + 1 words.
template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = dwg_lane(), w = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_u32(v);
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int i = 0; i < NT / 64; ++i) { const uint32_t c = lds[i]; lds[i] = s; s += c; }
        lds[NT / 64] = s;
    }
    __syncthreads();
    const uint32_t res = lds[w] + incl - v;
    *total = lds[NT / 64];
    __syncthreads();
    return res;
}

namespace {

// Count: count(n) = the count of item n, called for n < N only.
template <typename Count>
__global__ __launch_bounds__(kScanThreads) void k_scan_block_sums(Count count, uint32_t N, uint32_t* __restrict__ sums) {
    __shared__ uint32_t lds[kScanThreads / 64 + 1];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < N) s += count(base + k);
    uint32_t total;
    block_excl_scan_u32<kScanThreads>(s, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive block offsets.  add_to_total: the offsets start from total[0] and total[0] += the sum;
// otherwise they start from 0 and total[0] = the sum.
__global__ __launch_bounds__(kScanSumsThreads) void k_scan_sums(uint32_t* __restrict__ sums, uint32_t nb, uint32_t* __restrict__ total,
                                                                uint32_t add_to_total) {
    __shared__ uint32_t lds[kScanSumsThreads / 64 + 1];
    uint32_t carry = add_to_total ? total[0] : 0u;
    for (uint32_t b0 = 0; b0 < nb; b0 += kScanSumsThreads) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < nb ? sums[i] : 0u;
        uint32_t t;
        const uint32_t ex = block_excl_scan_u32<kScanSumsThreads>(v, lds, &t);
        if (i < nb) sums[i] = carry + ex;
        carry += t;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// Write: write(n, offset, count) stores the result of item n, called for n < N only.
template <typename Count, typename Write>
__global__ __launch_bounds__(kScanThreads) void k_scan_down(Count count, Write write, uint32_t N, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t lds[kScanThreads / 64 + 1];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t c[kScanItems], s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        c[k] = base + k < N ? count(base + k) : 0u;
        s += c[k];
    }
    uint32_t total;
    uint32_t off = sums[blockIdx.x] + block_excl_scan_u32<kScanThreads>(s, lds, &total);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < N) write(base + k, off, c[k]);
        off += c[k];
    }
}

// The three launches over N > 0 items; sums: scan_workspace_bytes(N).  names: what the profiler records them under.
template <typename Count, typename Write>
void scan_counts(const char* const (&names)[3], Count count, Write write, uint32_t N, uint32_t* sums, uint32_t* total, bool add_to_total,
                 hipStream_t st) {
    const uint32_t nb = scan_blocks(N);
    const auto block_sums = k_scan_block_sums<Count>;
    const auto down = k_scan_down<Count, Write>;
    DWG_LAUNCH_W(names[0], "k_scan_block_sums", 0.0, block_sums, dim3(nb), dim3(kScanThreads), 0, st, count, N, sums);
    DWG_LAUNCH_W(names[1], "k_scan_sums", 0.0, k_scan_sums, dim3(1), dim3(kScanSumsThreads), 0, st, sums, nb, total, add_to_total ? 1u : 0u);
    DWG_LAUNCH_W(names[2], "k_scan_down", 0.0, down, dim3(nb), dim3(kScanThreads), 0, st, count, write, N, (const uint32_t*)sums);
}

}  // namespace
