// fd_normal.h -- the finite-difference normal of the NeRF field (_NeRFNetwork.normal, core/nerf/nerf_model.py:146-169): the six shifted
// points and the normal from their densities.  One copy for the point-cloud export (pointcloud.hip: k_pc_fd_points, k_pc_finish) and the
// shaded inference render (nerf_field.hip's k_nf_render_shaded).  FP contraction is off inside every function here, whatever the
// including file compiles with: every product, sum and quotient is rounded on its own, as the torch statements these restate do.
#pragma once
#include <float.h>
#include <stdint.h>

// Component k (0 x, 1 y, 2 z) of the point's shift s (0 .. 5: +x, -x, +y, -y, +z, -z): (x + [0, .., +-eps, .., 0]).clamp(-bound, bound).
// The reference adds a full [1, 3] tensor, so the untouched components get + 0.f, and every component is clamped.
__device__ __forceinline__ float fd_shift(float v, uint32_t k, uint32_t s, float eps, float bound) {
#pragma clang fp contract(off)
    const float d = k == (s >> 1) ? ((s & 1u) ? -eps : eps) : 0.f;
    v = v + d;
    return v < -bound ? -bound : (v > bound ? bound : v);       // torch.clamp: NaN stays NaN
}

__device__ __forceinline__ float fd_nan_to_num(float v) {
    if (v != v) return 0.f;
    return v > FLT_MAX ? FLT_MAX : (v < -FLT_MAX ? -FLT_MAX : v);
}

// one component of -0.5 * stack(d_pos - d_neg) / epsilon
__device__ __forceinline__ float fd_gradient(float s_pos, float s_neg, float eps) {
#pragma clang fp contract(off)
    return (-0.5f * (s_pos - s_neg)) / eps;
}

// nan_to_num(safe_normalize(g))
__device__ __forceinline__ void fd_normalize(float g0, float g1, float g2, float& n0, float& n1, float& n2) {
#pragma clang fp contract(off)
    const float d = (g0 * g0 + g1 * g1) + g2 * g2;
    const float len = sqrtf(d < 1e-20f ? 1e-20f : d);           // torch.clamp(min): NaN stays NaN, and with it all three components
    n0 = fd_nan_to_num(g0 / len);
    n1 = fd_nan_to_num(g1 / len);
    n2 = fd_nan_to_num(g2 / len);
}
