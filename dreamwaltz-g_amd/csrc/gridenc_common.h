// gridenc_common.h -- grid lookup of the multi-resolution encoder (D = 3, C = 2), shared by the kernels of gridenc.hip (B2) and the
// fused NeRF field of nerf_field.hip (B7): the level's cell, its interpolation weights and the table index of a corner, exactly as
// gridencoder.cu computes them (get_grid_index :66-84, kernel_grid :110-150).
#pragma once
#include "dwg_common.h"

namespace {

struct GridP {
    uint32_t B, L;
    float S;
    uint32_t H, gridtype, align_corners, interp, layout;  // layout 0: [L,B,C] (reference backend), 1: [B,L*C]
};

__device__ __forceinline__ uint32_t grid_index(uint32_t gridtype, bool align, uint32_t hashmap_size, uint32_t res,
                                               uint32_t x, uint32_t y, uint32_t z) {
    // gridencoder.cu:66-84 for D = 3
    uint32_t stride = 1, index = 0;
    const uint32_t step = align ? res : (res + 1);
    if (stride <= hashmap_size) { index += x * stride; stride *= step; }
    if (stride <= hashmap_size) { index += y * stride; stride *= step; }
    if (stride <= hashmap_size) { index += z * stride; stride *= step; }
    if (gridtype == 0 && stride > hashmap_size) index = (x * 1u) ^ (y * 2654435761u) ^ (z * 805459861u);
    return (index % hashmap_size) * 2u;
}

struct Cell {
    bool oob;
    float scale;
    uint32_t res, hsize;
    float w[3], dw[3];
    uint32_t g[3];
};

__device__ __forceinline__ Cell locate(const GridP& p, const int* __restrict__ offsets, uint32_t level, float x0, float x1,
                                       float x2) {
    Cell c;
    c.oob = (x0 < 0.f || x0 > 1.f || x1 < 0.f || x1 > 1.f || x2 < 0.f || x2 > 1.f);
    c.hsize = (uint32_t)(offsets[level + 1] - offsets[level]);
    c.scale = exp2f((float)level * p.S) * (float)p.H - 1.0f;
    c.res = (uint32_t)ceilf(c.scale) + 1u;
    const float xs[3] = {x0, x1, x2};
    // NB (bug-compatible with gridencoder.cu:137): pos_deriv is initialised {1, 0, 0}; smoothstep overwrites all three
    c.dw[0] = 1.f; c.dw[1] = 0.f; c.dw[2] = 0.f;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        float pos = xs[d] * c.scale + (p.align_corners ? 0.0f : 0.5f);
        float fl = floorf(pos);
        c.g[d] = (uint32_t)fl;
        pos -= fl;
        if (p.interp == 1) { c.dw[d] = 6.f * pos * (1.f - pos); pos = pos * pos * (3.f - 2.f * pos); }
        c.w[d] = pos;
    }
    return c;
}

}  // namespace
