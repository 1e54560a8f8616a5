// scan_common.h -- the workgroup exclusive scan of 32-bit counts behind the deterministic three-launch scans (block sums -> one
// workgroup over the sums -> scan down): raymarch.hip's sample offsets of the training march and nerf_train.hip's offsets of the live
// samples.  Integer adds in a fixed order: no atomics, no cross-workgroup flags.
#pragma once
#include <stdint.h>

#include "dwg_common.h"

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
