// adam_math.h -- the fused Adam's arithmetic (adam.hip, boundary O2; the scalars also in grad_scaler.hip's k_scaler_prepare), written once
// for the HIP kernels and compilable by a C compiler for the host (tests/hostmath/adam_math_host.c, tests/hostmath/scaler_math_host.c).
// torch.optim.Adam semantics, amsgrad=False, weight_decay=0, maximize=False.
//
//   adam_hyper_row   the per-step scalars of one group -> row [4] fp32, the statements of FlatOptimizer.prepare_step: fp32
//                    hyper-parameters, double arithmetic, one rounding -- with the loss scaler's unscale folded into the gradient factor:
//                    {lr / (1 - b1^t), sqrt(1 - b2^t), grad_scale / scale, 0}.  The fourth float is the scaled step's skip flag.
//   adam_update      the per-element statements, with step = row[0], bc2_sqrt = row[1], grad_scale = row[2]:
//                      g = grad_scale * grad;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p = p - step m / (sqrt(v) / bc2_sqrt + eps)
//
// NO `fp contract(off)` pragma here, unlike adan_math.h: the Adam kernels have always been compiled with hipcc's default contraction
// (the moments' multiply-adds fuse), and every bit the project's determinism and parity tests were recorded against comes from that
// build.  Turning contraction off would change the device's results.  The host build (-ffp-contract=off) therefore does NOT reproduce the
// device's bits; the host test compares against float64 at the optimizer's tolerance instead.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DWG_ADAM_HD __host__ __device__ __forceinline__
#else
#define DWG_ADAM_HD static inline
#endif

DWG_ADAM_HD void adam_hyper_row(float lr, float beta1, float beta2, int32_t t, float grad_scale, float scale, float* row) {
    row[0] = (float)((double)lr / (1.0 - pow((double)beta1, (double)t)));
    row[1] = (float)sqrt(1.0 - pow((double)beta2, (double)t));
    row[2] = (float)((double)grad_scale / (double)scale);
    row[3] = 0.f;
}

/* One element.  p, m and v may point at registers (the components of a float4) or straight at memory (the n % 4 tail): both moments are
 * read before either is written and the parameter is read last, whatever the pointers alias. */
DWG_ADAM_HD void adam_update(float* p, float g, float* m, float* v, float step, float bc2_sqrt, float grad_scale, float b1, float b2,
                             float eps) {
    const float gr = g * grad_scale;
    const float mm = b1 * *m + (1.f - b1) * gr, vv = b2 * *v + (1.f - b2) * gr * gr;
    *m = mm; *v = vv;
    *p -= step * mm / (sqrtf(vv) / bc2_sqrt + eps);
}
