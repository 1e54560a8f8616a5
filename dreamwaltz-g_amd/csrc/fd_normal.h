// fd_normal.h -- the finite-difference normal of the NeRF field (_NeRFNetwork.normal, core/nerf/nerf_model.py:146-169): the six shifted
// points here, the normal from their densities in shade_math.h (fd_gradient, fd_normalize, shade_normal).  One copy for the point-cloud
// export (pointcloud.hip: k_pc_fd_points, k_pc_finish) and the shaded inference render (nerf_field.hip's k_nf_render_shaded).
// FP contraction is off inside every function of both headers, whatever the including file
// compiles with: every product, sum and quotient is rounded on its own, as the torch statements these restate do.
#pragma once
#include <float.h>
#include <stdint.h>
#include "shade_math.h"       // the normal from the six densities and the shading, shared with the training kernels and the host build

// Component k (0 x, 1 y, 2 z) of the point's shift s (0 .. 5: +x, -x, +y, -y, +z, -z): (x + [0, .., +-eps, .., 0]).clamp(-bound, bound).
// The reference adds a full [1, 3] tensor, so the untouched components get + 0.f, and every component is clamped.
__device__ __forceinline__ float fd_shift(float v, uint32_t k, uint32_t s, float eps, float bound) {
#pragma clang fp contract(off)
    const float d = k == (s >> 1) ? ((s & 1u) ? -eps : eps) : 0.f;
    v = v + d;
    return v < -bound ? -bound : (v > bound ? bound : v);       // torch.clamp: NaN stays NaN
}
