// shade_math.h -- per-sample arithmetic of the shaded NeRF views, written once for the HIP kernels (nerf_field.hip's shaded inference
// render, nerf_train.hip's training shade kernels, pointcloud.hip's k_pc_finish; the first and the last through fd_normal.h) and
// compilable by a C compiler for the host (tests/hostmath/shade_math_host.c checks the hand-derived backward against autograd on the
// CPU; the product runs it on the device).  The normalisation stands once: fd_unit, which the forward (fd_normalize, shade_normal) and
// the backward both call.  The three shading statements are shade_color; nerf_field.hip's inference render alone keeps a copy of
// them (shade_sample: why is written there).
//
// Forward: the statements of _NeRFNetwork.normal and forward (core/nerf/nerf_model.py:84-105, 155-168) for one sample, from the six
// densities at the shifted points:
//   g_a = (-0.5 (s+_a - s-_a)) / eps,   n = nan_to_num(g / sqrt(clamp(g.g, min=1e-20))),
//   'normal' (n + 1) / 2,   lam = ratio + (1 - ratio) clamp(n.(-l), min=0),   'textureless' lam,   'lambertian' albedo lam.
// Backward: what torch autograd does for those statements, node by node (div, clamp, sqrt, sum, mul, nan_to_num, matmul), so that
// non-finite intermediates travel as they do there: nan_to_num passes the gradient as a product with isfinite(input), clamp(min) as a
// select on input >= min.  Below the clamp the normalisation divides by 1e-10 and the gradient is dn / 1e-10: huge, and the reference's.
// FP contraction is off inside every function (a host compiler is given -ffp-contract=off): every product, sum and quotient is rounded
// on its own, as the torch statements are.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DWG_SHADE_HD __host__ __device__ __forceinline__
#else
#define DWG_SHADE_HD static inline
#endif
#if defined(__clang__)
#define DWG_SHADE_STRICT _Pragma("clang fp contract(off)")
#else
#define DWG_SHADE_STRICT
#endif

#define DWG_SHADE_NORMAL 1u
#define DWG_SHADE_TEXTURELESS 2u
#define DWG_SHADE_LAMBERTIAN 3u

DWG_SHADE_HD float fd_nan_to_num(float v) {
    if (v != v) return 0.f;
    return v > FLT_MAX ? FLT_MAX : (v < -FLT_MAX ? -FLT_MAX : v);
}

// one component of -0.5 * stack(d_pos - d_neg) / epsilon
DWG_SHADE_HD float fd_gradient(float s_pos, float s_neg, float eps) {
    DWG_SHADE_STRICT
    return (-0.5f * (s_pos - s_neg)) / eps;
}

// safe_normalize(g) before its nan_to_num: d = g.g, len = sqrt(clamp(d, min=1e-20)) (torch.clamp(min): NaN stays NaN, and with it all
// three components), u = g / len.  Returns len; *d is what the backward's clamp selects on.
DWG_SHADE_HD float fd_unit(float g0, float g1, float g2, float* u, float* d) {
    DWG_SHADE_STRICT
    *d = (g0 * g0 + g1 * g1) + g2 * g2;
    const float len = sqrtf(*d < 1e-20f ? 1e-20f : *d);
    u[0] = g0 / len; u[1] = g1 / len; u[2] = g2 / len;
    return len;
}

// n[3] = nan_to_num(safe_normalize(g))
DWG_SHADE_HD void fd_normalize(float g0, float g1, float g2, float* n) {
    float u[3], d;
    fd_unit(g0, g1, g2, u, &d);
    n[0] = fd_nan_to_num(u[0]); n[1] = fd_nan_to_num(u[1]); n[2] = fd_nan_to_num(u[2]);
}

// n[3] from the six densities s (+x, -x, +y, -y, +z, -z)
DWG_SHADE_HD void shade_normal(const float* s, float eps, float* n) {
    fd_normalize(fd_gradient(s[0], s[1], eps), fd_gradient(s[2], s[3], eps), fd_gradient(s[4], s[5], eps), n);
}

// The colour of a sample from its normal and albedo.  l = -light_d (read for 'textureless' and 'lambertian'); one_minus_ratio is the
// Python scalar 1 - ratio as torch hands it to its kernel.  rgb[nc]: channels the shading does not write (the fourth of a latent
// image, the reference's zero pad) are 0.  alb[nc] is read by 'lambertian' only.
DWG_SHADE_HD void shade_color(uint32_t shading, float ratio, float one_minus_ratio, float lx, float ly, float lz, float n0, float n1, float n2,
                              const float* alb, int nc, float* rgb) {
    DWG_SHADE_STRICT
    for (int k = 0; k < nc; ++k) rgb[k] = 0.f;
    if (shading == DWG_SHADE_NORMAL) {
        rgb[0] = (n0 + 1.f) / 2.f; rgb[1] = (n1 + 1.f) / 2.f; rgb[2] = (n2 + 1.f) / 2.f;
        return;
    }
    const float dot = (n0 * lx + n1 * ly) + n2 * lz;
    const float lam = ratio + one_minus_ratio * (dot < 0.f ? 0.f : dot);            // clamp(min=0): NaN stays NaN
    if (shading == DWG_SHADE_TEXTURELESS) { rgb[0] = lam; rgb[1] = lam; rgb[2] = lam; }
    else {
        for (int k = 0; k < nc; ++k) rgb[k] = alb[k] * lam;
    }
}

// Backward of shade_normal + shade_color for one sample: grgb[>= 3] (a latent image's fourth channel is the constant pad: its gradient is
// never read) -> ds[6], the gradient of the six shifted densities, and for 'lambertian' dalb[3] (not written otherwise).
//
// dlam, the one sum whose terms cancel, is taken in double: three exact products and two adds, rounded once.  Everything after it is a
// chain of products and quotients, and the projection du - u (u.du) whose terms are each at most |du|, so the result stays within a few
// ulps of |dn| 0.5 / (eps max(|g|, 1e-10)) per component.
DWG_SHADE_HD void shade_backward(uint32_t shading, float ratio, float one_minus_ratio, float lx, float ly, float lz, float eps, const float* s,
                                 const float* alb, const float* grgb, float* ds, float* dalb) {
    DWG_SHADE_STRICT
    // the forward again
    const float g[3] = {fd_gradient(s[0], s[1], eps), fd_gradient(s[2], s[3], eps), fd_gradient(s[4], s[5], eps)};
    float u[3], d;
    const float len = fd_unit(g[0], g[1], g[2], u, &d);
    float dn[3];
    if (shading == DWG_SHADE_NORMAL) {
        dn[0] = grgb[0] / 2.f; dn[1] = grgb[1] / 2.f; dn[2] = grgb[2] / 2.f;
    } else {
        const float n0 = fd_nan_to_num(u[0]), n1 = fd_nan_to_num(u[1]), n2 = fd_nan_to_num(u[2]);
        const float dot = (n0 * lx + n1 * ly) + n2 * lz;
        double dl;
        if (shading == DWG_SHADE_TEXTURELESS) dl = ((double)grgb[0] + (double)grgb[1]) + (double)grgb[2];
        else {
            const float lam = ratio + one_minus_ratio * (dot < 0.f ? 0.f : dot);
            dalb[0] = grgb[0] * lam; dalb[1] = grgb[1] * lam; dalb[2] = grgb[2] * lam;
            dl = ((double)grgb[0] * (double)alb[0] + (double)grgb[1] * (double)alb[1]) + (double)grgb[2] * (double)alb[2];
        }
        const float dclamp = (float)dl * one_minus_ratio;
        const float ddot = dot >= 0.f ? dclamp : 0.f;                               // clamp(min=0) passes where its input is >= 0: not at NaN
        dn[0] = ddot * lx; dn[1] = ddot * ly; dn[2] = ddot * lz;
    }
    // nan_to_num: grad * isfinite(input)
    float du[3];
    for (int k = 0; k < 3; ++k) du[k] = dn[k] * ((u[k] - u[k]) == 0.f ? 1.f : 0.f);
    // u = g / len: d/dg = du / len, d/dlen = sum_k -du_k ((g_k / len) / len)
    const float dlen = ((-du[0] * (u[0] / len)) + (-du[1] * (u[1] / len))) + (-du[2] * (u[2] / len));
    const float dc = dlen / (2.f * len);                                            // sqrt
    const float dd = d >= 1e-20f ? dc : 0.f;                                        // clamp(min=1e-20) passes where its input is >= min
    for (int k = 0; k < 3; ++k) {
        const float dg = du[k] / len + (dd * g[k] + dd * g[k]);                     // the quotient's and the square's (g * g: twice) shares
        const float t = -0.5f * (dg / eps);
        ds[2 * k] = t;
        ds[2 * k + 1] = -t;
    }
}
