/*
 * include/dwg_image_loss.h -- C-ABI of the image reconstruction loss of the nerf2gs loop (boundary B17): the reference's
 * ImageReconstructionLoss (core/gaussian/gaussian_loss.py:9-60,131-138),
 *
 *     loss = (1 - lambda) * mean|x - y| + lambda * (1 - mean(SSIM(x, y))),
 *
 * SSIM with an 11 x 11 Gaussian window (sigma 1.5), zero padding, C1 = 0.01^2, C2 = 0.03^2, sigma = E[..] - mu * mu -- the standard
 * L1 + D-SSIM loss of image-fitted 3D Gaussian splatting.
 *
 *   dwg_image_loss_forward     per-workgroup partial sums + one finishing launch -> loss, l1, ssim (and one ssim mean per batch item)
 *   dwg_image_loss_backward    dL/dx in one launch, scaled by an upstream gradient read from device memory; y gets no gradient
 *
 * Images are fp32, B x C planes of H x W, each described by FOUR element strides (batch, channel, row, pixel): a plane index b * C + c
 * is not linear in memory for a [B, H, W, C] tensor with B > 1, so the plane stride is given as its two parts.  NCHW tensors and
 * [B, H, W, C] renders are both read in place; the gradient is written with x's strides.
 *
 * The window is the reference's eleven fp32 weights (exp(-(i - 5)^2 / (2 * 1.5^2)) rounded to fp32, divided by their fp32 sum); the
 * filter is applied separably and, like the SSIM map, accumulated in fp64; every sum runs in a fixed order.  No float atomics: two
 * calls give the same bits.  All pointers are device pointers; nothing is allocated inside and nothing is read back; every launch
 * goes to `stream` and can be captured.  Every entry point returns DWG_E_ARG before any launch on a bad argument.
 */
#ifndef DWG_IMAGE_LOSS_H
#define DWG_IMAGE_LOSS_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_IMAGE_LOSS_WINDOW 11    /* the only window size */
#define DWG_IMAGE_LOSS_TILE 16      /* pixels per workgroup edge */
#define DWG_IMAGE_LOSS_MAX_SIZE 32768 /* H and W at most */
#define DWG_IMAGE_LOSS_MAX_PLANES 65535 /* B * C at most */

/* Bytes of workspace of dwg_image_loss_forward: two fp64 partial sums per (16 x 16 tile, plane).  0 on a size that the forward
 * refuses. */
size_t dwg_image_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W);

/* window_size is DWG_IMAGE_LOSS_WINDOW and lambda_dssim lies in [0, 1]; anything else is DWG_E_ARG.
 * x, y: fp32 images with element strides (batch, channel, row, pixel).  A stride of x over a dimension longer than 1 is >= 1 (the
 * gradient is written in that layout); a stride of y is >= 0.
 * scalars [3] fp32 <- loss, l1 = mean|x - y|, ssim = mean of the SSIM map.  ssim_batch [B] fp32 (NULL: not written) <- the SSIM mean of
 * every batch item (the reference's size_average=False).
 * maps [3, B, C, H, W] fp32 (NULL: not stored) <- what dwg_image_loss_backward needs: with S the SSIM map as a function of
 * mu1 = F[x], e11 = F[x x], e12 = F[x y] (F the filter), a = dS/dmu1, b = dS/de11 and c + 2 b where c = dS/de12.
 * workspace: 16-byte aligned, dwg_image_loss_workspace_bytes(B, C, H, W) bytes. */
int dwg_image_loss_forward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t window_size, float lambda_dssim,
                           const float* x, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                           const float* y, int64_t y_batch_stride, int64_t y_channel_stride, int64_t y_row_stride, int64_t y_pixel_stride,
                           float* scalars, float* ssim_batch, float* maps, void* workspace, size_t workspace_bytes, dwg_stream_t stream);

/* grad_x (x's strides) <- g * fp32(coef_ssim * (F[a] + 2 (x - y) F[b] + y F[c + 2 b]) + coef_l1 * sign(x - y)), sign(0) = 0;
 * F[a] + 2 (x - y) F[b] + y F[c + 2 b] = F[a] + 2 x F[b] + y F[c] is the derivative of the SUM of the SSIM map.  g = grad_out[0], or
 * grad_out[b] when grad_per_batch != 0 (grad_out is then [B]); it is read on the device.  The image loss has
 * coef_ssim = -lambda / N and coef_l1 = (1 - lambda) / N with N = B C H W.  maps: the forward's, for the same x and y; NULL is
 * allowed only with coef_ssim == 0 (the L1 term alone). */
int dwg_image_loss_backward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t window_size, double coef_ssim, double coef_l1,
                            const float* x, int64_t x_batch_stride, int64_t x_channel_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                            const float* y, int64_t y_batch_stride, int64_t y_channel_stride, int64_t y_row_stride, int64_t y_pixel_stride,
                            const float* maps, const float* grad_out, int32_t grad_per_batch, float* grad_x, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
