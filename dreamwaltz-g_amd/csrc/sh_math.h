// sh_math.h -- the per-Gaussian statements of the static Gaussian scene (include/dwg_scene_gaussians.h), written once for
// scene_gaussians.hip and compilable on the host (a stand-alone program runs them under the host sanitizers).
//
// Follows what the reference computes through PyTorch, statement by statement and in its order of evaluation:
//   GaussianModel activations (sigmoid / exp / F.normalize)   core/gaussian/gaussian_model.py:35-56
//   get_colors: clamp_min(eval_sh(L - 1, sh, dir) + 0.5, 0)   core/gaussian/gaussian_utils.py:12-17
//   eval_sh, degree <= 3                                      core/gaussian/spherical_harmonics.py:117-172
//   compute_colors: dir = F.normalize(p - cam)                core/gaussian/gaussian_renderer.py:72-105
// Every operation is rounded on its own.  FP contraction is off inside every function (a host compiler is given -ffp-contract=off): HIP's
// __fmul_rn / __fadd_rn are plain operators that the compiler contracts all the same, and its __fsqrt_rn is the approximate square root,
// so the statements are plain C: `*`, `+`, `-`, `/` and sqrtf, which hipcc rounds correctly by default.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DWG_SHD __host__ __device__ __forceinline__
#else
#define DWG_SHD static inline
#endif

#if defined(__clang__)
#define DWG_SH_STRICT _Pragma("clang fp contract(off)")
#else
#define DWG_SH_STRICT
#endif

#define DWG_SH_C0 0.28209479177387814f
#define DWG_SH_C1 0.4886025119029199f
#define DWG_SH_EPS 1e-12f            /* F.normalize's eps */

DWG_SHD float dwg_scene_sigmoid(float x) {
    DWG_SH_STRICT
    return 1.f / (1.f + expf(-x));
}

// F.normalize over n <= 4 values: x / max(sqrt(((x0^2 + x1^2) + x2^2) + ...), eps)
DWG_SHD void dwg_scene_normalize(const float* x, int n, float* out) {
    DWG_SH_STRICT
    float s = x[0] * x[0];
    for (int c = 1; c < n; c++) {
        const float sq = x[c] * x[c];
        s = s + sq;
    }
    const float d = fmaxf(sqrtf(s), DWG_SH_EPS);
    for (int c = 0; c < n; c++) out[c] = x[c] / d;
}

// sh_levels = 1: max(C0 * dc + 0.5, 0)
DWG_SHD float dwg_scene_dc_color(float dc) {
    DWG_SH_STRICT
    const float t = DWG_SH_C0 * dc;
    return fmaxf(t + 0.5f, 0.f);
}

// One channel of eval_sh(levels - 1, sh, dir) + 0.5, clamped at 0.  sh[k]: coefficient k of the channel (k < levels^2), d: the unit direction.
DWG_SHD float dwg_scene_sh_color(int levels, const float* sh, const float d[3]) {
    DWG_SH_STRICT
    const float x = d[0], y = d[1], z = d[2];
    float r = DWG_SH_C0 * sh[0];
    if (levels > 1) {
        r = r - (DWG_SH_C1 * y) * sh[1];
        r = r + (DWG_SH_C1 * z) * sh[2];
        r = r - (DWG_SH_C1 * x) * sh[3];
    }
    if (levels > 2) {
        const float xx = x * x, yy = y * y, zz = z * z;
        const float xy = x * y, yz = y * z, xz = x * z;
        const float a = (2.0f * zz - xx) - yy;
        const float xmy = xx - yy;
        r = r + (1.0925484305920792f * xy) * sh[4];
        r = r + (-1.0925484305920792f * yz) * sh[5];
        r = r + (0.31539156525252005f * a) * sh[6];
        r = r + (-1.0925484305920792f * xz) * sh[7];
        r = r + (0.5462742152960396f * xmy) * sh[8];
        if (levels > 3) {
            const float b = (4.f * zz - xx) - yy;
            const float t9 = 3.f * xx - yy;
            const float t12 = (2.f * zz - 3.f * xx) - 3.f * yy;
            const float t15 = xx - 3.f * yy;
            r = r + ((-0.5900435899266435f * y) * t9) * sh[9];
            r = r + ((2.890611442640554f * xy) * z) * sh[10];
            r = r + ((-0.4570457994644658f * y) * b) * sh[11];
            r = r + ((0.3731763325901154f * z) * t12) * sh[12];
            r = r + ((-0.4570457994644658f * x) * b) * sh[13];
            r = r + ((1.445305721320277f * z) * xmy) * sh[14];
            r = r + ((-0.5900435899266435f * x) * t15) * sh[15];
        }
    }
    return fmaxf(r + 0.5f, 0.f);
}

// The three colour channels of one scene Gaussian at sh_levels in 1..4: dc [1, 3] and rest [15, 3] of that Gaussian (coefficient-major,
// channel fastest: the layout of the reference's _sh_features_dc / _sh_features_rest), its position and the camera's.
DWG_SHD void dwg_scene_view_color_at(const int levels, const float* dc, const float* rest, const float p[3], const float cam[3], float col[3]) {
    DWG_SH_STRICT
    const float v[3] = {p[0] - cam[0], p[1] - cam[1], p[2] - cam[2]};
    float d[3];
    dwg_scene_normalize(v, 3, d);
    for (int c = 0; c < 3; c++) {
        float sh[16];
        sh[0] = dc[c];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int k = 1; k < 16; k++) sh[k] = k < levels * levels ? rest[(k - 1) * 3 + c] : 0.f;
        col[c] = dwg_scene_sh_color(levels, sh, d);
    }
}

DWG_SHD void dwg_scene_view_color(int levels, const float* dc, const float* rest, const float p[3], const float cam[3], float col[3]) {
    switch (levels) {                       // a literal level per branch: the coefficient array stays in registers
        case 2: dwg_scene_view_color_at(2, dc, rest, p, cam, col); break;
        case 3: dwg_scene_view_color_at(3, dc, rest, p, cam, col); break;
        case 4: dwg_scene_view_color_at(4, dc, rest, p, cam, col); break;
        default:
            for (int c = 0; c < 3; c++) col[c] = dwg_scene_dc_color(dc[c]);
    }
}
