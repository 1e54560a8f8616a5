/*
 * include/dwg_nerf_view.h -- C-ABI of the view around the NeRF stage's training render (boundary B20): what the reference's
 * _NeRFRenderer.render (core/nerf/nerf_renderer.py:404-472) does before and after run_cuda, and SparsityLoss
 * (core/nerf/nerf_loss.py:17-56).
 *
 *   dwg_nerf_view_rays               one launch: get_rays with N = -1 for one camera read from device memory, and the slab test of
 *                                    dwg_raymarch_near_far_from_aabb on the rays it stores
 *   dwg_nerf_view_compose_forward    image = image_fg + (1 - weights_sum) * image_bg written planar ([1, channels_out, H, W]), and the
 *                                    sparsity loss of weights_sum as one fp32 scalar (per-workgroup fp64 partial sums + one finishing launch)
 *   dwg_nerf_view_compose_backward   one launch: d image_fg, d weights_sum (mix term + sparsity terms), optionally d image_bg
 *
 * All tensors are fp32 and contiguous.  N = H * W pixels in row-major order; C = 3 (rgb) or 4 (latent) channels; 1 <= channels_out <= C.
 * The fp32 statements round every operation on its own (no contraction), the sparsity terms are evaluated in fp64 from the fp32
 * weights_sum and summed in a fixed order: no atomics, two calls give the same bits.  All pointers are device pointers; nothing is
 * allocated inside and nothing is read back; every launch goes to `stream` and can be captured.  Every entry point returns DWG_E_ARG
 * before any launch on a bad argument.
 */
#ifndef DWG_NERF_VIEW_H
#define DWG_NERF_VIEW_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_VIEW_BG_NONE 0u     /* image = the first channels_out channels of image_fg */
#define DWG_VIEW_BG_CONSTANT 1u /* bg [C]: one colour */
#define DWG_VIEW_BG_IMAGE 2u    /* bg [N, C]: one colour per pixel */
#define DWG_VIEW_MAX_SIZE 32768 /* H and W at most; H * W < 2^31 */

/* c2w [16] row-major (rows 0..2 are read), intrinsics [9] row-major (fx, fy, cx, cy are read), aabb [6].
 * rays_o, rays_d [H * W, 3], nears, fars [H * W] <- pixel p = row * W + col: the direction of the pixel centre (col + 0.5, row + 0.5),
 * ((i - cx) / fx, (j - cy) / fy, 1) normalised (clamp of the squared length at 1e-20) and rotated by c2w[:3, :3]; the origin
 * c2w[:3, 3]; nears / fars are bit for bit what dwg_raymarch_near_far_from_aabb gives on the stored rays. */
int dwg_nerf_view_rays(const float* c2w, const float* intrinsics, const float* aabb, uint32_t H, uint32_t W, float min_near,
                       float* rays_o, float* rays_d, float* nears, float* fars, dwg_stream_t stream);

/* Bytes of the workspace the two compose calls share: three fp64 partial sums per workgroup of 256 pixels and the three totals. */
size_t dwg_nerf_view_compose_workspace_bytes(uint32_t N);

/* image_fg [N, C], weights_sum [N], bg: NULL / [C] / [N, C] by bg_mode.  image [channels_out, N] <- the mix (or the channel slice).
 * sparsity_loss (NULL: not computed, workspace not touched) [1] fp32 <-
 *     mult * (lambda_opacity * sqrt(mean(ws^2 + 0.01)) + lambda_entropy * mean H2(clamp(ws, fp32(1e-6), fp32(1 - 1e-6)))
 *             + lambda_emptiness * 10000 * mean log(1 + 10 ws)),       a term whose lambda is not positive is left out.
 * image_fg == image == NULL (then bg == NULL too): only the sparsity loss is computed.
 * workspace: 16-byte aligned, dwg_nerf_view_compose_workspace_bytes(N) bytes; it keeps the sums the backward reads. */
int dwg_nerf_view_compose_forward(uint32_t N, uint32_t C, uint32_t channels_out, const float* image_fg, const float* weights_sum,
                                  const float* bg, uint32_t bg_mode, double lambda_opacity, double lambda_entropy, double lambda_emptiness,
                                  double mult, float* image, float* sparsity_loss, void* workspace, size_t workspace_bytes,
                                  dwg_stream_t stream);

/* d_image [channels_out, N] (NULL: zero), d_sparsity [1] on the device (NULL: the sparsity loss got no gradient; then workspace may be
 * NULL), weights_sum / bg / workspace: the forward's.
 * d_image_fg [N, C] (NULL: skipped) <- d_image transposed, zeros in the channels beyond channels_out.
 * d_weights_sum [N] <- fp32 of (-sum_c bg_c d_image_c, 0 with detach_ws or without a background) + d_sparsity * d loss / d ws, the sum
 *     formed in fp64; the entropy term passes no gradient where its clamp is active.
 * d_image_bg [N, C] (NULL: skipped; only with DWG_VIEW_BG_IMAGE) <- (1 - ws) * d_image. */
int dwg_nerf_view_compose_backward(uint32_t N, uint32_t C, uint32_t channels_out, const float* d_image, const float* d_sparsity,
                                   const float* weights_sum, const float* bg, uint32_t bg_mode, uint32_t detach_ws, double lambda_opacity,
                                   double lambda_entropy, double lambda_emptiness, double mult, const void* workspace,
                                   size_t workspace_bytes, float* d_image_fg, float* d_weights_sum, float* d_image_bg, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
