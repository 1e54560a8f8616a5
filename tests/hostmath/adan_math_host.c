/* Host build of csrc/adan_math.h for tests/test_adan_host.py: the clipping factor, a group's scalars and the update over an array. */
#include "../../dreamwaltz-g_amd/csrc/adan_math.h"

int host_adan_row_floats(void) { return ADAN_ROW_FLOATS; }

/* sum of squares of grad [n] in double, index order */
double host_adan_sumsq(int64_t n, const float* grad) {
    double t = 0.0;
    for (int64_t i = 0; i < n; ++i) t += (double)grad[i] * (double)grad[i];
    return t;
}

double host_adan_clip(double sumsq, double max_grad_norm, double grad_scale, double eps) { return adan_clip(sumsq, max_grad_norm, grad_scale, eps); }

void host_adan_hyper_row(double lr, double beta1, double beta2, double beta3, double eps, double weight_decay, int no_prox, int32_t t, int first,
                         double clip, double grad_scale, float* row) {
    adan_hyper_row(lr, beta1, beta2, beta3, eps, weight_decay, no_prox, t, first, clip, grad_scale, row);
}

void host_adan_update(int64_t n, const float* row, const float* grad, float* p, float* exp_avg, float* exp_avg_sq, float* exp_avg_diff,
                      float* neg_pre_grad) {
    for (int64_t i = 0; i < n; ++i) adan_update(row, grad[i], p + i, exp_avg + i, exp_avg_sq + i, exp_avg_diff + i, neg_pre_grad + i);
}
