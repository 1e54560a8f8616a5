/*
 * include/dwg_grad_scaler.h -- C-ABI of the device-resident loss scaler of the stage-I step under optim.fp16 (boundary B21): what
 * torch.cuda.amp.GradScaler's scale / step / update do around the optimizers (the reference's loop, core/trainer.py:840-896), with the
 * decision to skip a step, the unscale, the per-group Adam step counts and the scale schedule kept on the device.
 *
 *   dwg_grads_nonfinite               scan a range of the flat fp32 gradient buffer for Inf / NaN: one 0 / 1 slot per workgroup
 *   dwg_scaler_prepare                one workgroup: OR the slots into the optimizer's `found` and the scaler's found_inf; on a clean
 *                                     step bump the step count of every participating group and write its row of the hyper table
 *   dwg_adam_step_groups_scaled_dev   dwg_adam_step_groups_dev whose rows carry grad_scale / scale and a skip flag
 *   dwg_scaler_update                 torch._amp_update_scale_ on the state, then found_inf = 0
 *
 * All pointers are device pointers unless said otherwise; nothing is allocated inside and nothing is read back; every launch goes to
 * `stream` and can be captured.  No atomics: two calls on the same inputs give the same bits.  Every entry point returns DWG_E_ARG before
 * any launch on a bad argument.
 */
#ifndef DWG_GRAD_SCALER_H
#define DWG_GRAD_SCALER_H
#include "dwg_elementwise.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The scaler's device block (16 bytes, 16-byte aligned). */
typedef struct dwg_scaler_state {
    float scale;            /* the loss scale */
    int32_t growth_tracker; /* consecutive steps without Inf / NaN since the scale last moved */
    float found_inf;        /* 1 when some optimizer of this step found Inf / NaN, else 0 */
    int32_t reserved;
} dwg_scaler_state;

#define DWG_SCALER_MAX_SLOTS 2048 /* the scan's grid cap: slots [DWG_SCALER_MAX_SLOTS] int32 is always enough */

/* Number of slots (workgroups) the scan of n floats writes: min(ceil((n / 4) / 256), DWG_SCALER_MAX_SLOTS), at least 1; 0 for n <= 0. */
int32_t dwg_grads_nonfinite_slots(int64_t n);

/* grad [n] fp32, 16-byte aligned.  slots[b] <- 1 when workgroup b met an Inf or NaN in its share, else 0, for every
 * b < dwg_grads_nonfinite_slots(n): every slot is written by every call (no clearing launch). */
int dwg_grads_nonfinite(int64_t n, const float* grad, int32_t* slots, dwg_stream_t stream);

/* f = OR of slots[0 .. nslots).  found[0] <- f (fp32 0 / 1); state->found_inf <- 1 when f (left as it is otherwise: several optimizers
 * share one state).  groups <= DWG_ADAM_MAX_GROUPS; mask bit g: group g takes part in this step; beta1 / beta2 are HOST arrays [groups];
 * lr [groups], steps [groups] int32 and hyper [groups][4] are device arrays.
 *   f == 0: for every g in mask, t = ++steps[g] and hyper[g] <- {lr[g] / (1 - beta1[g]^t), sqrt(1 - beta2[g]^t), grad_scale / state->scale, 0}
 *           formed in double from the fp32 values and rounded once; the rows of the other groups get a 0 in their fourth float.
 *   f != 0: steps stay; hyper[g] <- {0, 1, 0, 1} for every g (the fourth float is the skip flag). */
int dwg_scaler_prepare(int32_t nslots, const int32_t* slots, dwg_scaler_state* state, float* found, int32_t groups, uint32_t mask,
                       const float* lr, const float* beta1, const float* beta2, float grad_scale, int32_t* steps, float* hyper,
                       dwg_stream_t stream);

/* dwg_adam_step_groups_dev (dwg_elementwise.h) with two differences: a group whose row has a non-zero fourth float is left untouched
 * (param, exp_avg, exp_avg_sq are neither read nor written), and the gradient factor hyper[row][2] carries the unscale. */
int dwg_adam_step_groups_scaled_dev(int32_t count, const dwg_adam_group* groups, const float* hyper, dwg_stream_t stream);

/* torch._amp_update_scale_: found_inf != 0: scale *= backoff_factor, growth_tracker = 0; else growth_tracker + 1, and when that equals
 * growth_interval: scale *= growth_factor unless the product is not finite, growth_tracker = 0.  Then found_inf = 0. */
int dwg_scaler_update(dwg_scaler_state* state, double growth_factor, double backoff_factor, int32_t growth_interval, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
