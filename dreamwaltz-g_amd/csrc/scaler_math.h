// scaler_math.h -- scalar arithmetic of the device-resident loss scaler (grad_scaler.hip, boundary B21), written once for the HIP kernels
// and compilable by a C compiler for the host (tests/hostmath/scaler_math_host.c).
//
//   scaler_nonfinite    an fp32 value is Inf or NaN (all exponent bits set); FLT_MAX and denormals are finite
//   scaler_update       torch._amp_update_scale_ for one (scale, growth_tracker): backoff on a found Inf / NaN, growth after
//                       growth_interval clean steps unless the grown scale would not be finite
// The per-step scalars of an Adam group that k_scaler_prepare writes (adam_hyper_row) live with the optimizer's arithmetic in adam_math.h.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "adam_math.h"

#if defined(__HIPCC__)
#define DWG_SCALER_HD __host__ __device__ __forceinline__
#else
#define DWG_SCALER_HD static inline
#endif

DWG_SCALER_HD int scaler_nonfinite_bits(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

DWG_SCALER_HD int scaler_nonfinite(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return scaler_nonfinite_bits(b);
}

// The factors are doubles as torch passes them: the product is formed in double from the fp32 scale and rounded once.
DWG_SCALER_HD void scaler_update(float* scale, int32_t* growth_tracker, int found_inf, double growth_factor, double backoff_factor,
                                 int32_t growth_interval) {
    if (found_inf) {
        *scale = (float)((double)*scale * backoff_factor);
        *growth_tracker = 0;
        return;
    }
    const int32_t successful = *growth_tracker + 1;
    if (successful == growth_interval) {
        const float grown = (float)((double)*scale * growth_factor);
        if (!scaler_nonfinite(grown)) *scale = grown;
        *growth_tracker = 0;
    } else {
        *growth_tracker = successful;
    }
}
