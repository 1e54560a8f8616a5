// cull_math.h -- "may this scene Gaussian have a non-empty tile rectangle under this camera?" (include/dwg_scene_cull.h), written once for
// scene_cull.hip and compilable on the host (tests/hostmath/cull_math_host.cpp; a stand-alone program runs it under the host sanitizers).
//
// The contract is one-sided: the answer is never 0 for a Gaussian that raster.hip's k_preprocess gives radius > 0 (scale_modifier 1).  It
// may be 1 for one that k_preprocess then drops: that costs time, not correctness.  It is a BOUND with margins, not a copy of the kernel's
// statements -- raster.hip is compiled with FP contraction on, so its last bit cannot be restated; every margin below is orders of
// magnitude above fp32 rounding:
//   near plane   k_preprocess keeps pv.z > 0.2; pv is evaluated here exactly as xform43 does (contraction off there too); kept from
//                0.2 (1 - 1e-4)
//   extent       cov2D = J W Sigma W^T J^T + 0.3 I with Sigma = R diag(s^2) R^T.  The activated quaternion has norm 1 within fp32
//                rounding (the zero quaternion gives R = I in quat_to_R), W is a rotation, so lambda_max(cov2D) <= (1.001 max s)^2 |J|_F^2
//                + 0.3, with |J|_F^2 = (fx / z)^2 (1 + cx^2) + (fy / z)^2 (1 + cy^2) and cx = min(|pv.x / z|, 1.3 tanfovx) the clamp of
//                ewa_project.  k_preprocess's larger eigenvalue is mid + sqrt(max(0.1, mid^2 - det)) <= lambda_max + sqrt(0.1) < + 0.32.
//                rad = ceil(3 sqrt(lambda) 1.001) + 1 >= the kernel's integer radius.
//   rectangle    k_preprocess's tile rectangle of [px - rad, px + rad + RT - 1] is empty unless that interval meets [0, rtiles RT); here
//                the interval is widened by RT + m on the right, m on the left, m = 1 + 1e-5 |px| (the rounding of px under contraction),
//                and the image by one more tile.
// Anything that is not a number keeps the Gaussian (every drop is a comparison that a NaN fails).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DWG_CULLD __host__ __device__ __forceinline__
#else
#define DWG_CULLD static inline
#endif

#if defined(__clang__)
#define DWG_CULL_STRICT _Pragma("clang fp contract(off)")
#else
#define DWG_CULL_STRICT
#endif

#define DWG_CULL_RT 16                    /* the rasterizer's reference tile edge (raster.hip RT) */
#define DWG_CULL_NEAR 0.2f                /* k_preprocess: pv.z > 0.2 */
#define DWG_CULL_CAMERA_VIEW 0            /* offsets into a camera block: [viewmatrix 16 | projmatrix 16 | campos 3 | tanfovx | tanfovy] */
#define DWG_CULL_CAMERA_PROJ 16
#define DWG_CULL_CAMERA_TANFOV 35

// one axis: does [p - rad - m, p + rad + RT + m] meet [0, tiles RT + RT)?
DWG_CULLD int dwg_cull_axis(float p, float rad, int tiles) {
    DWG_CULL_STRICT
    const float m = 1.f + 1e-5f * fabsf(p);
    const float lo = (p - rad) - m, hi = ((p + rad) + (float)DWG_CULL_RT) + m;
    const float end = (float)(tiles * DWG_CULL_RT + DWG_CULL_RT);
    if (hi < 0.f) return 0;
    if (lo >= end) return 0;
    return 1;
}

// pos[3], scales[3] (activated), cam: one camera block (37 floats, row-major 4x4 matrices as the rasterizer reads them: element [4 c + k]
// multiplies coordinate c into output k), image W x H -> 1: may be visible, 0: certainly radius 0 in k_preprocess.
DWG_CULLD int dwg_cull_may_be_visible(const float* pos, const float* scales, const float* cam, int W, int H) {
    DWG_CULL_STRICT
    const float* v = cam + DWG_CULL_CAMERA_VIEW;
    const float* q = cam + DWG_CULL_CAMERA_PROJ;
    const float x = pos[0], y = pos[1], z = pos[2];
    const float pvx = ((v[0] * x + v[4] * y) + v[8] * z) + v[12];
    const float pvy = ((v[1] * x + v[5] * y) + v[9] * z) + v[13];
    const float pvz = ((v[2] * x + v[6] * y) + v[10] * z) + v[14];
    if (pvz <= DWG_CULL_NEAR * (1.f - 1e-4f)) return 0;
    const float zc = fmaxf(pvz, 0.19f);
    const float tanfovx = cam[DWG_CULL_CAMERA_TANFOV], tanfovy = cam[DWG_CULL_CAMERA_TANFOV + 1];
    const float fx = (float)W / (2.f * tanfovx), fy = (float)H / (2.f * tanfovy);
    const float s = 1.001f * fmaxf(scales[0], fmaxf(scales[1], scales[2]));
    const float cx = fminf(fabsf(pvx / zc), 1.3f * tanfovx), cy = fminf(fabsf(pvy / zc), 1.3f * tanfovy);
    const float jx = fx / zc, jy = fy / zc;
    const float j2 = (jx * jx) * (1.f + cx * cx) + (jy * jy) * (1.f + cy * cy);
    const float lambda = ((s * s) * j2 + 0.3f) + 0.32f;
    const float rad = ceilf((3.f * sqrtf(lambda)) * 1.001f) + 1.f;
    const float phx = ((q[0] * x + q[4] * y) + q[8] * z) + q[12];
    const float phy = ((q[1] * x + q[5] * y) + q[9] * z) + q[13];
    const float phw = ((q[3] * x + q[7] * y) + q[11] * z) + q[15];
    const float pw = 1.f / (phw + 1e-7f);
    const float px = ((phx * pw + 1.f) * (float)W - 1.f) * 0.5f, py = ((phy * pw + 1.f) * (float)H - 1.f) * 0.5f;
    const int tiles_x = (W + DWG_CULL_RT - 1) / DWG_CULL_RT, tiles_y = (H + DWG_CULL_RT - 1) / DWG_CULL_RT;
    return dwg_cull_axis(px, rad, tiles_x) && dwg_cull_axis(py, rad, tiles_y);
}
