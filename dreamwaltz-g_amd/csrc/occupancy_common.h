// occupancy_common.h -- the jittered cell point of the occupancy update (boundary B13, include/dwg_occupancy.h), shared by the field
// kernel that evaluates the density there (nerf_field.hip, XOccupancy) and the kernel that materialises the points (occupancy.hip).
// FP contraction is off inside these functions: the reference's torch statements (nerf_renderer.py:119-133) round every product and
// every sum once.
#pragma once
#include <stdint.h>

struct OccLattice {
    const float* __restrict__ axis;         // [H]    2 i / (H - 1) - 1 as the caller's torch evaluates it
    const float* __restrict__ noise;        // [C, H^3, 3] uniform draws in [0, 1), meshgrid order
    const float* __restrict__ scale;        // [C]    bound_c - bound_c / H
    const float* __restrict__ half;         // [C]    bound_c / H
    uint32_t lg;                            // log2 H
};

// meshgrid index n = (ix H + iy) H + iz of a cascade -> (ix, iy, iz); H = 1 << lg
__device__ __forceinline__ void occ_decode(uint32_t lg, uint32_t n, uint32_t& ix, uint32_t& iy, uint32_t& iz) {
    const uint32_t m = (1u << lg) - 1u;
    iz = n & m; iy = (n >> lg) & m; ix = n >> (2u * lg);
}

// component k of the point of flat cell g = c H^3 + n:  axis[i] * scale[c] + (noise[c, n, k] * 2 - 1) * half[c]
__device__ __forceinline__ float occ_point(const OccLattice& l, uint32_t g, uint32_t k) {
#pragma clang fp contract(off)
    const uint32_t c = g >> (3u * l.lg), n = g & ((1u << (3u * l.lg)) - 1u);
    uint32_t i[3];
    occ_decode(l.lg, n, i[0], i[1], i[2]);
    const float a = l.axis[i[k]] * l.scale[c];
    const float r = l.noise[(uint64_t)g * 3u + k] * 2.f - 1.f;
    return a + r * l.half[c];
}

// the blob of random_sigmas (nerf_renderer.py:133): 1.0 * exp(-(x ** 2).sum(-1) / (2 * 0.2 ** 2)) as torch evaluates it on the device.
// Its reduction over a last dimension of 3 runs on two lanes: lane 0 adds elements 0 and 2, then lane 1's element is added, so the sum is
// (x^2 + z^2) + y^2; the division by the Python scalar is a product with its fp32 inverse (1 / 0.08f rounds to 12.5f).
__device__ __forceinline__ float occ_blob(float x, float y, float z) {
#pragma clang fp contract(off)
    const float d = (x * x + z * z) + y * y;
    return 1.0f * expf(-d * (1.0f / 0.08f));
}

// C H^3 within the limits of dwg_occupancy.h; lg <- log2 H
static inline bool occ_limits(uint32_t C, uint32_t H, uint32_t& lg) {
    if (C < 1 || C > 8 || H < 4 || H > 1024 || (H & (H - 1u))) return false;
    lg = 0;
    while ((1u << lg) < H) lg++;
    return ((uint64_t)C << (3u * lg)) < (1ull << 32);
}
