// view_math.h -- per-pixel arithmetic of the NeRF stage's view around the render (nerf_view.hip, boundary B20), written once for the HIP
// kernels and compilable by a C compiler for the host (tests/hostmath/view_math_host.c).
//
//   view_ray            the statements of get_rays with N = -1 (core/nerf/nerf_utils.py:72-137) for one pixel: the centre (i + 0.5,
//                       j + 0.5), the direction ((i - cx) / fx, (j - cy) / fy, 1), safe_normalize with its clamp at 1e-20, and the
//                       product with c2w[:3, :3]^T
//   view_mix            image_fg + (1 - weights_sum) * image_bg, every operation rounded on its own (nerf_renderer.py:468-470)
//   sparsity_terms      the three per-element terms of SparsityLoss (core/nerf/nerf_loss.py:17-28) in double from the fp32 weights_sum
//   sparsity_loss       the loss from the three sums
//   sparsity_derivative d loss / d weights_sum of one element from the saved sum of the opacity term
// FP contraction is off inside every function (a host compiler is given -ffp-contract=off): the fp32 statements round as torch's do.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DWG_VIEW_HD __host__ __device__ __forceinline__
#else
#define DWG_VIEW_HD static inline
#endif
#if defined(__clang__)
#define DWG_VIEW_STRICT _Pragma("clang fp contract(off)")
#else
#define DWG_VIEW_STRICT
#endif

/* entropy_loss's clamp: alphas in [eps, 1 - eps].  torch clamps the fp32 tensor against the Python doubles 1e-6 and 1 - 1e-6 ROUNDED TO
 * FP32 (9.99999997e-7 and 0.99999899): those are the thresholds here, of the clamp and of its gradient gate alike, so that a
 * weights_sum equal to fp32(1e-6) passes its gradient as it does there. */
#define DWG_VIEW_ENTROPY_LO ((double)(float)1e-6)
#define DWG_VIEW_ENTROPY_HI ((double)(float)(1.0 - 1e-6))
#define DWG_VIEW_OPACITY_BIAS 0.01       /* opacity_loss: sqrt(mean(ws^2 + 0.01)) */
#define DWG_VIEW_EMPTINESS_WEIGHT 10000.0
#define DWG_VIEW_EMPTINESS_SCALE 10.0

// Pixel (row, col) of a camera c2w [16] row-major (the upper 3 x 4 is read) with intrinsics [9] row-major -> d[3], the unit direction
// in world space.  The origin of every ray is c2w[3], c2w[7], c2w[11].
DWG_VIEW_HD void view_ray(const float* c2w, const float* intrinsics, uint32_t row, uint32_t col, float* d) {
    DWG_VIEW_STRICT
    const float fx = intrinsics[0], fy = intrinsics[4], cx = intrinsics[2], cy = intrinsics[5];
    const float i = (float)col + 0.5f, j = (float)row + 0.5f;
    const float x = (i - cx) / fx, y = (j - cy) / fy, z = 1.f;
    const float s = (x * x + y * y) + z * z;
    const float len = sqrtf(s < 1e-20f ? 1e-20f : s);
    const float ux = x / len, uy = y / len, uz = z / len;
    d[0] = (ux * c2w[0] + uy * c2w[1]) + uz * c2w[2];
    d[1] = (ux * c2w[4] + uy * c2w[5]) + uz * c2w[6];
    d[2] = (ux * c2w[8] + uy * c2w[9]) + uz * c2w[10];
}

DWG_VIEW_HD float view_mix(float fg, float ws, float bg) {
    DWG_VIEW_STRICT
    const float t = 1.f - ws;
    const float u = t * bg;
    return fg + u;
}

// t[0] = ws^2 + 0.01, t[1] = the binary entropy (log2) of clamp(ws, fp32(1e-6), fp32(1 - 1e-6)), t[2] = log(1 + 10 ws)
DWG_VIEW_HD void sparsity_terms(float ws, double* t) {
    DWG_VIEW_STRICT
    const double w = (double)ws;
    const double a = w < DWG_VIEW_ENTROPY_LO ? DWG_VIEW_ENTROPY_LO : (w > DWG_VIEW_ENTROPY_HI ? DWG_VIEW_ENTROPY_HI : w);
    t[0] = w * w + DWG_VIEW_OPACITY_BIAS;
    t[1] = -a * log2(a) - (1.0 - a) * log2(1.0 - a);
    t[2] = log(1.0 + DWG_VIEW_EMPTINESS_SCALE * w);
}

// sums[3]: the sums of the three terms over n elements.  A term whose lambda is not positive is left out, as the reference does.
DWG_VIEW_HD double sparsity_loss(const double* sums, double n, double lambda_opacity, double lambda_entropy, double lambda_emptiness, double mult) {
    DWG_VIEW_STRICT
    double loss = 0.0;
    if (lambda_opacity > 0.0) loss += lambda_opacity * sqrt(sums[0] / n);
    if (lambda_entropy > 0.0) loss += lambda_entropy * (sums[1] / n);
    if (lambda_emptiness > 0.0) loss += lambda_emptiness * (DWG_VIEW_EMPTINESS_WEIGHT * (sums[2] / n));
    return mult * loss;
}

// d sparsity_loss / d ws of one element.  sum_opacity: sums[0] of the forward.  The entropy term passes no gradient where its clamp
// is active (torch's clamp: the gradient passes where min <= x <= max).
DWG_VIEW_HD double sparsity_derivative(float ws, double sum_opacity, double n, double lambda_opacity, double lambda_entropy, double lambda_emptiness,
                                       double mult) {
    DWG_VIEW_STRICT
    const double w = (double)ws;
    double g = 0.0;
    if (lambda_opacity > 0.0) g += lambda_opacity * (w / (n * sqrt(sum_opacity / n)));
    if (lambda_entropy > 0.0 && w >= DWG_VIEW_ENTROPY_LO && w <= DWG_VIEW_ENTROPY_HI)
        g += lambda_entropy * ((log2(1.0 - w) - log2(w)) / n);
    if (lambda_emptiness > 0.0)
        g += lambda_emptiness * (DWG_VIEW_EMPTINESS_WEIGHT * DWG_VIEW_EMPTINESS_SCALE / ((1.0 + DWG_VIEW_EMPTINESS_SCALE * w) * n));
    return mult * g;
}
