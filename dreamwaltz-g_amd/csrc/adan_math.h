// adan_math.h -- the Adan optimizer's arithmetic (adan.hip, boundary B23), written once for the HIP kernels and compilable by a C compiler
// for the host (tests/hostmath/adan_math_host.c).  Restated from the optimizer's statements (Xie et al., arXiv 2208.06677; the
// reference's core/optim/adan.py:110-129, 139-150, 221-256).
//
//   adan_clip        the global-norm clipping factor from the sum of squares of the whole gradient:
//                    min(max_grad_norm / (sqrt(total) * grad_scale + eps), 1), or 1 when max_grad_norm is 0 (no clipping)
//   adan_hyper_row   the per-step scalars of one group -> row [DWG_ADAN_ROW] fp32.  The hyper-parameters are doubles, as Python holds
//                    them; every scalar is formed in double and rounded ONCE.  (1 - beta formed from an fp32 beta would be off by 1e-6
//                    relative: the betas sit near 1.)
//   adan_update      the per-element statements, every fp32 operation rounded on its own (no contraction):
//                      g = gfac * grad                      gfac = clip * grad_scale
//                      d = g + neg_pre                      (neg_pre holds -previous g; first update of the group: d = 0)
//                      m = b1 m + (1 - b1) g
//                      v = b2 v + (1 - b2) d
//                      u = b2 d + g
//                      n = b3 n + (1 - b3) u u
//                      den = sqrt(n) / sqrt(1 - b3^t) + eps
//                      p = (p - step m / den - step_diff v / den) / (1 + lr wd)             (default)
//                      p = p (1 - lr wd) - step m / den - step_diff v / den                 (no_prox)
//                      neg_pre = -g
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DWG_ADAN_HD __host__ __device__ __forceinline__
#else
#define DWG_ADAN_HD static inline
#endif
#if defined(__clang__)
#define DWG_ADAN_STRICT _Pragma("clang fp contract(off)")
#else
#define DWG_ADAN_STRICT
#endif

/* the floats of a group's row of the device hyper table (include/dwg_adan.h: DWG_ADAN_ROW floats, 64 bytes) */
enum {
    ADAN_GFAC = 0,       /* clip * grad_scale */
    ADAN_STEP = 1,       /* lr / (1 - beta1^t) */
    ADAN_STEP_DIFF = 2,  /* lr * beta2 / (1 - beta2^t) */
    ADAN_BC3_SQRT = 3,   /* sqrt(1 - beta3^t) */
    ADAN_DECAY = 4,      /* 1 + lr * wd (divides), under no_prox 1 - lr * wd (multiplies) */
    ADAN_FIRST = 5,      /* 1: the group's first update (d = 0), else 0 */
    ADAN_B1 = 6, ADAN_OMB1 = 7, ADAN_B2 = 8, ADAN_OMB2 = 9, ADAN_B3 = 10, ADAN_OMB3 = 11,
    ADAN_EPS = 12,
    ADAN_NO_PROX = 13,   /* 1: no_prox, else 0 */
    ADAN_ROW_FLOATS = 16
};

DWG_ADAN_HD double adan_clip(double sumsq, double max_grad_norm, double grad_scale, double eps) {
    if (!(max_grad_norm > 0.0)) return 1.0;
    const double c = max_grad_norm / (sqrt(sumsq) * grad_scale + eps);
    return c < 1.0 ? c : 1.0;             /* torch.clamp(max=1): a NaN stays a NaN */
}

DWG_ADAN_HD void adan_hyper_row(double lr, double beta1, double beta2, double beta3, double eps, double weight_decay, int no_prox, int32_t t,
                                int first, double clip, double grad_scale, float* row) {
    row[ADAN_GFAC] = (float)(clip * grad_scale);
    row[ADAN_STEP] = (float)(lr / (1.0 - pow(beta1, (double)t)));
    row[ADAN_STEP_DIFF] = (float)(lr * beta2 / (1.0 - pow(beta2, (double)t)));
    row[ADAN_BC3_SQRT] = (float)sqrt(1.0 - pow(beta3, (double)t));
    row[ADAN_DECAY] = (float)(no_prox ? 1.0 - lr * weight_decay : 1.0 + lr * weight_decay);
    row[ADAN_FIRST] = first ? 1.f : 0.f;
    row[ADAN_B1] = (float)beta1; row[ADAN_OMB1] = (float)(1.0 - beta1);
    row[ADAN_B2] = (float)beta2; row[ADAN_OMB2] = (float)(1.0 - beta2);
    row[ADAN_B3] = (float)beta3; row[ADAN_OMB3] = (float)(1.0 - beta3);
    row[ADAN_EPS] = (float)eps;
    row[ADAN_NO_PROX] = no_prox ? 1.f : 0.f;
    row[14] = 0.f; row[15] = 0.f;
}

/* One element.  exp_avg_sq is the reference's name for n, exp_avg_diff for v. */
DWG_ADAN_HD void adan_update(const float* row, float grad, float* p, float* exp_avg, float* exp_avg_sq, float* exp_avg_diff, float* neg_pre_grad) {
    DWG_ADAN_STRICT
    const float g = grad * row[ADAN_GFAC];
    const float d = row[ADAN_FIRST] != 0.f ? 0.f : *neg_pre_grad + g;
    const float m1 = *exp_avg * row[ADAN_B1];
    const float m2 = g * row[ADAN_OMB1];
    const float m = m1 + m2;
    const float v1 = *exp_avg_diff * row[ADAN_B2];
    const float v2 = d * row[ADAN_OMB2];
    const float v = v1 + v2;
    const float u1 = d * row[ADAN_B2];
    const float u = u1 + g;
    const float n1 = *exp_avg_sq * row[ADAN_B3];
    const float uu = u * u;
    const float n2 = uu * row[ADAN_OMB3];
    const float n = n1 + n2;
    const float r = sqrtf(n) / row[ADAN_BC3_SQRT];
    const float den = r + row[ADAN_EPS];
    float q = *p;
    if (row[ADAN_NO_PROX] != 0.f) q = q * row[ADAN_DECAY];
    const float qm = m / den;
    const float sm = row[ADAN_STEP] * qm;
    q = q - sm;
    const float qv = v / den;
    const float sv = row[ADAN_STEP_DIFF] * qv;
    q = q - sv;
    if (row[ADAN_NO_PROX] == 0.f) q = q / row[ADAN_DECAY];
    *p = q;
    *exp_avg = m;
    *exp_avg_diff = v;
    *exp_avg_sq = n;
    *neg_pre_grad = -g;
}
