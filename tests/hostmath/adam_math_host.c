/* Host build of csrc/adam_math.h for tests/test_adam_math_host.py: a group's scalars and the update over an array. */
#include "../../dreamwaltz-g_amd/csrc/adam_math.h"

void host_adam_row(float lr, float beta1, float beta2, int32_t t, float grad_scale, float scale, float* row) {
    adam_hyper_row(lr, beta1, beta2, t, grad_scale, scale, row);
}

/* row = {step, bc2_sqrt, grad_scale, skip}, as the kernels read it */
void host_adam_update(int64_t n, const float* row, float beta1, float beta2, float eps, const float* grad, float* p, float* exp_avg,
                      float* exp_avg_sq) {
    for (int64_t i = 0; i < n; ++i) adam_update(p + i, grad[i], exp_avg + i, exp_avg_sq + i, row[0], row[1], row[2], beta1, beta2, eps);
}
