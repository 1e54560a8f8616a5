/* Host build of csrc/scaler_math.h for tests/test_grad_scaler_host.py: the scale schedule over a scripted sequence and the Adam scalars. */
#include "../../dreamwaltz-g_amd/csrc/scaler_math.h"

/* found [steps] (0 / 1) -> scales, trackers [steps]: the state after each update, starting from (scale0, tracker0) */
void host_scaler_sequence(int steps, const int32_t* found, float scale0, int32_t tracker0, double growth_factor, double backoff_factor,
                          int32_t growth_interval, float* scales, int32_t* trackers) {
    float scale = scale0;
    int32_t tracker = tracker0;
    for (int i = 0; i < steps; ++i) {
        scaler_update(&scale, &tracker, found[i], growth_factor, backoff_factor, growth_interval);
        scales[i] = scale;
        trackers[i] = tracker;
    }
}

void host_adam_hyper_row(float lr, float beta1, float beta2, int32_t t, float grad_scale, float scale, float* row) {
    adam_hyper_row(lr, beta1, beta2, t, grad_scale, scale, row);
}

int host_scaler_nonfinite(float x) { return scaler_nonfinite(x); }
