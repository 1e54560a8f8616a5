/*
 * include/dwg_nerf_train.h -- C-ABI of the training render of the NeRF stage (boundary B18): the pieces that turn the training branch of
 * the reference's _NeRFRenderer.run_cuda (core/nerf/nerf_renderer.py:334-349: march_rays_train -> the field network ->
 * composite_rays_train, and their backward) into one chain that keeps, for the backward, only the samples the composite used.
 *
 * composite_rays_train stops a ray at the first sample after which T < T_thresh (raymarching.cu:541-569); that sample is composited,
 * nothing after it is, and the backward (raymarching.cu:652-694) writes no gradient there.  The field backward over those rows adds
 * zeros.  The chain is
 *   dwg_raymarch_march_rays_train (count, write)  ->  dwg_nerf_field_forward  ->  dwg_raymarch_composite_rays_train_forward_live
 *   ->  dwg_nerf_train_compact_offsets  ->  dwg_nerf_train_gather_live
 * and, in the backward, dwg_raymarch_composite_rays_train_backward and dwg_nerf_field_backward on the gathered rows with rays_live in
 * the place of rays and M_live in the place of M.  A ray's live samples are the leading ones, so the composite of the gathered rows
 * is the composite of the full rows, bit for bit.
 *
 * All pointers are device pointers; buffers are caller-allocated.  Every function checks its arguments before any launch (DWG_E_ARG,
 * DWG_E_CAPACITY) and runs on `stream`.  No atomics, no cross-workgroup flags: integer adds in a fixed order, bit-for-bit copies and,
 * in the two shade kernels, per-sample float arithmetic.
 */
#ifndef DWG_NERF_TRAIN_H
#define DWG_NERF_TRAIN_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

size_t dwg_nerf_train_workspace_bytes(uint32_t N);

/* rays_live[n] = (exclusive prefix sum of live[0..n), live[n]) in ray order, total[0] = the sum (M_live); a negative live[n] counts
 * as 0.  The three-launch scan of dwg_raymarch_march_rays_train's count pass.  workspace: dwg_nerf_train_workspace_bytes(N) bytes.
 * N == 0 launches nothing and writes nothing, total included. */
int dwg_nerf_train_compact_offsets(const int32_t* live /*[N]*/, uint32_t N, int32_t* rays_live /*[N,2]*/, int32_t* total /*[1]*/,
                                   void* workspace, size_t workspace_bytes, dwg_stream_t stream);

/* Row r < rays_live[n,1] of ray n goes from row rays[n,0] + r of every source to row rays_live[n,0] + r of its destination, bit for
 * bit, in one launch: xyzs [M,3], ts [M,2], sigmas [M] fp32 and rgbs [M,channels] fp32 (rgbs_f16 == 0) or fp16 (rgbs_f16 == 1), into
 * buffers of M_live rows.  A source and its destination are given together or both NULL (that array is not moved).  A ray whose source
 * range leaves [0, M), whose destination range leaves [0, M_live) or whose rays_live[n,1] exceeds rays[n,1] is skipped.  A wave walks
 * one ray's rows; offsets are 64-bit.  Buffers are 4-byte aligned (fp16 rgbs of 3 channels: 2-byte; of 4 channels the rows go as
 * words).  N == 0, M == 0 or M_live == 0 launch nothing. */
int dwg_nerf_train_gather_live(const int32_t* rays /*[N,2]*/, const int32_t* rays_live /*[N,2]*/, uint32_t N, uint32_t M, uint32_t M_live,
                               const float* xyzs, float* xyzs_live, const float* ts, float* ts_live, const float* sigmas,
                               float* sigmas_live, const void* rgbs, void* rgbs_live, uint32_t channels /*3 or 4*/, uint32_t rgbs_f16,
                               dwg_stream_t stream);

/* dwg_nerf_train_gather_live's rule for one more per-sample array of fp32 rows (boundary B19: the six shifted densities): src
 * [M, floats_per_row] -> dst [M_live, floats_per_row], bit for bit, the same rays skipped.  1 <= floats_per_row <= 64. */
int dwg_nerf_train_gather_live_rows(const int32_t* rays /*[N,2]*/, const int32_t* rays_live /*[N,2]*/, uint32_t N, uint32_t M, uint32_t M_live,
                                    const float* src, float* dst, uint32_t floats_per_row, dwg_stream_t stream);

/* The shaded training render (boundary B19) puts two per-sample kernels between the field and the composite:
 *   dwg_raymarch_march_rays_train -> dwg_nerf_field_forward_fd (dwg_nerf.h) -> dwg_nerf_train_shade_forward -> composite ... and back:
 *   composite backward -> dwg_nerf_train_shade_backward -> dwg_nerf_field_backward_fd, on the live rows.
 * shade_forward: the colour of forward() (nerf_model.py:86-103) from sigma_fd [M, 6] (the densities at the six shifted points), the
 * normal n = nan_to_num(safe_normalize(-0.5 (s+ - s-) / epsilon)): shading 1 'normal' (n + 1) / 2; 2 'textureless' and 3 'lambertian'
 * from lam = ratio + (1 - ratio) clamp(n . -light_d, min=0).  albedo [M, channels] fp32 (albedo_f16 == 0) or fp16 is read by 'lambertian'
 * only (NULL otherwise), which takes channels == 3.  light_d: device [3], NULL for 'normal'.  rgbs [M, channels] fp32; with channels ==
 * 4 the fourth is the reference's zero pad.
 * shade_backward: grad_rgbs [M, channels] fp32 -> dsigma_fd [M, 6] fp32 and, when dalbedo is given ('lambertian' must), dalbedo
 * [M, channels] in the albedo dtype (zero for the other shadings).  It restates torch autograd for those statements: clamp(min) passes
 * the gradient where its input is >= min, nan_to_num where its input is finite; the pad's gradient is dropped.
 * sigma_fd and dsigma_fd are 8-byte aligned.  M == 0 launches nothing. */
int dwg_nerf_train_shade_forward(uint32_t shading, const float* sigma_fd, const void* albedo, uint32_t albedo_f16, const float* light_d,
                                 float ambient_ratio, float epsilon, uint32_t M, uint32_t channels /*3 or 4*/, float* rgbs,
                                 dwg_stream_t stream);
int dwg_nerf_train_shade_backward(uint32_t shading, const float* sigma_fd, const void* albedo, uint32_t albedo_f16, const float* light_d,
                                  float ambient_ratio, float epsilon, uint32_t M, uint32_t channels, const float* grad_rgbs,
                                  float* dsigma_fd, void* dalbedo, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
