/*
 * include/dwg_adan.h -- C-ABI of the fused Adan optimizer on flat fp32 buffers (boundary B23): the optimizer of the stage-II learned
 * MLP background (the reference's MLPBackground.get_optimizer, core/system/background.py:86-89: Adan(lr=1e-3, eps=1e-8,
 * weight_decay=2e-5, max_grad_norm=5.0), core/optim/adan.py).  The statements are restated in csrc/adan_math.h.
 *
 * The reference reads the clipping factor back to the host every step (adan.py:125-127).  Here a step is three launches and nothing is
 * read back:
 *
 *   dwg_adan_sumsq             one fp64 partial sum of squares of the gradient per workgroup, each written to its own slot
 *   dwg_adan_prepare           one workgroup: the slots summed in slot order, the clipping factor, every group's step count + 1, every
 *                              group's row of the hyper table
 *   dwg_adan_step_groups_dev   the update of the participating groups in one launch
 *
 * No hand-off between workgroups inside a launch and no float atomics: two runs on the same inputs give the same bits.  All pointers are
 * device pointers unless said otherwise; nothing is allocated inside; every launch goes to `stream` and can be captured.  Every entry
 * point returns DWG_E_ARG before any launch on a bad argument.  The gradient buffer is only read: the clipped gradient is not written
 * back.
 */
#ifndef DWG_ADAN_H
#define DWG_ADAN_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_ADAN_MAX_GROUPS 16  /* param groups per optimizer */
#define DWG_ADAN_MAX_SLOTS 1024 /* the grid cap of dwg_adan_sumsq: partials [DWG_ADAN_MAX_SLOTS] fp64 is always enough */
#define DWG_ADAN_ROW 16         /* floats per group in the hyper table (64 bytes) */

/* Number of slots (workgroups) the scan of n floats writes: min(ceil((n / 4) / 256), DWG_ADAN_MAX_SLOTS), at least 1; 0 for n <= 0.
 * Beyond DWG_ADAN_MAX_SLOTS * 1024 elements every workgroup strides over the buffer. */
int32_t dwg_adan_sumsq_slots(int64_t n);

/* grad [n] fp32, 16-byte aligned -> partials[b] = the sum of grad[i]^2 over workgroup b's share, in fp64 (each square is exact in
 * fp64), for every b < dwg_adan_sumsq_slots(n); partials 8-byte aligned.  Every slot is written by every call. */
int dwg_adan_sumsq(int64_t n, const float* grad, double* partials, dwg_stream_t stream);

/* The hyper-parameters of one group, as Python holds them. */
typedef struct dwg_adan_hyper {
    double lr, beta1, beta2, beta3, eps, weight_decay;
    int32_t no_prox, reserved;
} dwg_adan_hyper;

/* One workgroup.  hyper is a HOST array [groups], groups in 1..DWG_ADAN_MAX_GROUPS.
 *   total = partials[0] + partials[1] + ... in slot order (nslots in 1..DWG_ADAN_MAX_SLOTS), or nslots == 0 and partials NULL when
 *           max_grad_norm == 0: the scan is skipped
 *   clip  = min(max_grad_norm / (sqrt(total) * grad_scale + eps), 1) with the LAST group's eps (adan.py:126), 1 without clipping
 *   for every group g: t = ++steps[g] (int32 [groups]: a group ages whether or not it takes part, adan.py:143-146) and
 *   rows[g] <- {clip * grad_scale, lr / (1 - beta1^t), lr * beta2 / (1 - beta2^t), sqrt(1 - beta3^t), the decay factor (1 + lr * wd, or
 *   1 - lr * wd under no_prox), the first-update flag (t == 1 or bit g of first_mask), beta1, 1 - beta1, beta2, 1 - beta2, beta3,
 *   1 - beta3, eps, no_prox, 0, 0}, each formed in double and rounded once.  rows [groups][DWG_ADAN_ROW] fp32, 16-byte aligned. */
int dwg_adan_prepare(int32_t nslots, const double* partials, int32_t groups, const dwg_adan_hyper* hyper, uint32_t first_mask,
                     double max_grad_norm, double grad_scale, int32_t* steps, float* rows, dwg_stream_t stream);

/* One group of the update: its slices of the flat buffers (16-byte aligned), its element count and its row of the hyper table.
 * neg_pre_grad holds MINUS the previous clipped gradient, the reference's sign. */
typedef struct dwg_adan_group {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq; float* exp_avg_diff; float* neg_pre_grad;
    int64_t n;
    int32_t hyper_row, reserved;
} dwg_adan_group;

/* The statements of csrc/adan_math.h on every element of `count` groups (0..DWG_ADAN_MAX_GROUPS; groups is a HOST array) in one launch:
 * 16-byte loads and stores, the n % 4 tail element by element.  rows as dwg_adan_prepare wrote them.  A group with n == 0 is skipped. */
int dwg_adan_step_groups_dev(int32_t count, const dwg_adan_group* groups, const float* rows, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
