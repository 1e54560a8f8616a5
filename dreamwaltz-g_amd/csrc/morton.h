// morton.h -- the 3-D Morton code of the occupancy grid (raymarching.cu:92-117): a cell (x, y, z) of a cascade lives at morton3d(x, y, z)
// in density_grid / density_bitfield.  One copy for the marcher (raymarch.hip), the occupancy update (nerf_field.hip's k_nf_occupancy) and
// occupancy.hip: the three must agree bit for bit.  10 bits per axis (H <= 1024).
#pragma once
#include <stdint.h>

__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3d(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
__device__ __forceinline__ uint32_t morton3d_invert(uint32_t x) {
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}
