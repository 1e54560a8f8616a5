// raymarch_common.h -- the per-ray marching rule of the occupancy-grid ray marcher (raymarching.cu:385-464, :751-827): where a ray's next
// sample lies.  One copy for the marcher (raymarch.hip: the training march and the inference loop's march_rays) and the one-launch
// inference render (nerf_field.hip's k_nf_render): the two must agree bit for bit, a one-ulp change of t moves a sample across a voxel
// boundary.  FP contraction is off inside every function here, whatever the including file compiles with: the float32 restatement
// (tests/raymarch_cases.py) rounds every operation separately.
#pragma once
#include <stdint.h>

#include "morton.h"

constexpr float kSqrt3 = 1.7320508075688772f;

__device__ __forceinline__ float clampf_(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }

// level from a magnitude: frexp exponent clamped to [0, C-1] ([0.5,1) -> 0, [1,2) -> 1, ...)
__device__ __forceinline__ int mip_level(float mx, float maxc) {
    int e;
    frexpf(mx, &e);
    return (int)fminf(maxc - 1.f, fmaxf(0.f, (float)e));
}

struct MarchP {
    const uint8_t* grid;
    float bound, dt_gamma, dt_min, dt_max, rH, Hf, maxc;
    uint32_t H, H3;
    bool contract;
};

inline MarchP make_march(const uint8_t* grid, float bound, uint32_t contract, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H) {
    MarchP p;
    p.grid = grid;
    p.bound = bound;
    p.dt_gamma = dt_gamma;
    p.dt_min = 2.f * kSqrt3 / (float)max_steps;
    p.dt_max = 2.f * kSqrt3 * bound / (float)H;
    p.rH = 1.f / (float)H;
    p.Hf = (float)H;
    p.maxc = (float)C;
    p.H = H;
    p.H3 = H * H * H;
    p.contract = contract != 0;
    return p;
}

inline bool march_args_ok(float bound, uint32_t max_steps, uint32_t C, uint32_t H) {
    // level * H^3 + morton < 2^32 and the bitfield index fits: C <= 8, H <= 1024 (morton of 10-bit coordinates)
    return bound > 0.f && max_steps > 0 && C >= 1 && C <= 8 && H >= 1 && H <= 1024 && (uint64_t)C * H * H * H < (1ull << 32);
}

struct Ray {
    float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz;
};

__device__ __forceinline__ Ray load_ray(const float* o, const float* d) {
    Ray r;
    r.ox = o[0]; r.oy = o[1]; r.oz = o[2];
    r.dx = d[0]; r.dy = d[1]; r.dz = d[2];
    r.rdx = 1.f / r.dx; r.rdy = 1.f / r.dy; r.rdz = 1.f / r.dz;
    return r;
}

// The slab test of near_far_from_aabb (raymarching.cu:92-138) for one ray: near clamped to min_near, both FLT_MAX on a miss.  One copy
// for raymarch.hip's k_near_far and nerf_view.hip's ray kernel, which computes the interval of the ray it has just stored.
__device__ __forceinline__ void near_far_ray(const Ray& r, const float* __restrict__ aabb, float min_near, float& near_out, float& far_out) {
#pragma clang fp contract(off)
    float near = (aabb[0] - r.ox) * r.rdx, far = (aabb[3] - r.ox) * r.rdx;
    if (near > far) { float c = near; near = far; far = c; }
    float ny = (aabb[1] - r.oy) * r.rdy, fy = (aabb[4] - r.oy) * r.rdy;
    if (ny > fy) { float c = ny; ny = fy; fy = c; }
    if (near > fy || ny > far) { near_out = far_out = 3.402823466e+38f; return; }
    if (ny > near) near = ny;
    if (fy < far) far = fy;
    float nz = (aabb[2] - r.oz) * r.rdz, fz = (aabb[5] - r.oz) * r.rdz;
    if (nz > fz) { float c = nz; nz = fz; fz = c; }
    if (near > fz || nz > far) { near_out = far_out = 3.402823466e+38f; return; }
    if (nz > near) near = nz;
    if (fz < far) far = fz;
    if (near < min_near) near = min_near;
    near_out = near;
    far_out = far;
}

__device__ __forceinline__ float start_t(const MarchP& p, float t0, float noise) {
#pragma clang fp contract(off)
    return t0 + clampf_(t0 * p.dt_gamma, p.dt_min, p.dt_max) * noise;
}

// One iteration of the marching loop at `t` (raymarching.cu:398-464).  Occupied cell: t += dt, returns true with the contracted
// position and dt of the sample.  Otherwise advances t (plain dt step under contraction outside the unit cube, else the do-while up
// to the next voxel boundary) and returns false.
__device__ __forceinline__ bool march_iter(const MarchP& p, const Ray& r, float& t, float& cx, float& cy, float& cz, float& dt) {
#pragma clang fp contract(off)
    const float x = clampf_(r.ox + t * r.dx, -p.bound, p.bound);
    const float y = clampf_(r.oy + t * r.dy, -p.bound, p.bound);
    const float z = clampf_(r.oz + t * r.dz, -p.bound, p.bound);
    dt = clampf_(t * p.dt_gamma, p.dt_min, p.dt_max);
    const float mag = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    const int level = max(mip_level(mag, p.maxc), mip_level(dt * p.Hf * 0.5f, p.maxc));
    const float mip_bound = fminf(scalbnf(1.f, level), p.bound);
    const float mip_rbound = 1.f / mip_bound;
    cx = x; cy = y; cz = z;
    const bool outside = p.contract && mag > 1.f;
    if (outside) {
        const float s = (2.f - 1.f / mag) / mag;
        cx = cx * s; cy = cy * s; cz = cz * s;
    }
    // 0.5 * (c/mip + 1) * H, each product rounded once as the reference's double-then-float conversion does
    const int nx = (int)clampf_(0.5f * (cx * mip_rbound + 1.f) * p.Hf, 0.f, p.Hf - 1.f);
    const int ny = (int)clampf_(0.5f * (cy * mip_rbound + 1.f) * p.Hf, 0.f, p.Hf - 1.f);
    const int nz = (int)clampf_(0.5f * (cz * mip_rbound + 1.f) * p.Hf, 0.f, p.Hf - 1.f);
    const uint32_t index = (uint32_t)level * p.H3 + morton3d((uint32_t)nx, (uint32_t)ny, (uint32_t)nz);
    if (p.grid[index >> 3] & (1u << (index & 7))) {
        t = t + dt;
        return true;
    }
    if (outside) {
        t = t + dt;
        return false;
    }
    const float tx = ((((float)nx + 0.5f) + 0.5f * copysignf(1.f, r.dx)) * p.rH * 2.f - 1.f) * mip_bound - cx;
    const float ty = ((((float)ny + 0.5f) + 0.5f * copysignf(1.f, r.dy)) * p.rH * 2.f - 1.f) * mip_bound - cy;
    const float tz = ((((float)nz + 0.5f) + 0.5f * copysignf(1.f, r.dz)) * p.rH * 2.f - 1.f) * mip_bound - cz;
    const float tt = t + fmaxf(0.f, fminf(tx * r.rdx, fminf(ty * r.rdy, tz * r.rdz)));
    do {
        dt = clampf_(t * p.dt_gamma, p.dt_min, p.dt_max);
        t = t + dt;
    } while (t < tt);
    return false;
}

// One sample of the inference composite (kernel_composite_rays, raymarching.cu:843-926), its statements in their order.  One copy for
// raymarch.hip's k_composite_rays and the one-launch renders (nerf_field.hip's nf_render).  Returns true when the transmittance before
// the sample was below T_thresh (the sample is composited all the same).
template <int NC>
__device__ __forceinline__ bool composite_sample(float sigma, const float (&rgb)[NC], float t, float dt, float T_thresh, bool binarize,
                                                 float& ws, float& d, float (&col)[NC]) {
#pragma clang fp contract(off)
    const float real_alpha = 1.f - expf(-sigma * dt);
    const float alpha = binarize ? (real_alpha > 0.5f ? 1.f : 0.f) : real_alpha;
    const float T = 1.f - ws;
    const float w = alpha * T;
    ws = ws + w;
    d = d + w * t;
#pragma unroll
    for (int k = 0; k < NC; ++k) col[k] = col[k] + w * rgb[k];
    return T < T_thresh;
}
