/*
 * include/dwg_depthmap.h -- C-ABI of the SMPL-X depth-map condition and of the NeRF pretrain loss that consumes it (boundary B9).
 *
 * What the reference's loader does on the CPU at every step of scripts/pretrain_nerf.sh (condition type 'depth_raw'): one pinhole ray per
 * pixel against the posed body mesh (core/human/smpl_condition.py:237-249,264-269 over utils/open3d.py:21-45: an open3d BVH build over
 * 20 908 triangles plus H x W rays), and what Trainer.pretrain_forward (core/trainer.py:1242-1279) does with the map: two MSE terms.
 *
 *   dwg_depthmap_cast            t_hit [H,W] (+ primitive normals [H,W,3]) of the mesh as it lies in device memory; no BVH is built
 *   dwg_depthmap_image           export_depth's inverse + normalise + uint8 image from a t_hit map
 *   dwg_pretrain_loss_forward    mean((ws - mask)^2) + mean((depth - sd)^2), sd = nan_to_num(smpl_depth), mask = sd > 1e-6
 *   dwg_pretrain_loss_backward   the two gradients, scaled by an upstream gradient read from device memory
 *
 * Ray and hit convention -- PARITY UNPINNED: open3d 0.17 is not on this stack, so create_rays_pinhole / cast_rays are restated from
 * their published behaviour (as oracle/condition.py does for the keypoint rays):
 *   - pixel (x, y) has the camera-space direction ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1), NOT normalised; it is rotated to world
 *     space by R^T; the origin is -R^T T; so t_hit counts units of that direction and IS the camera-space z of the hit; a miss is +inf;
 *   - directions are computed in fp64 and rounded to fp32 (open3d's rays are float32 tensors);
 *   - the intersection is Moeller-Trumbore in fp64 with |det| > 1e-12, u >= 0, w >= 0, u + w <= 1, t > 0 (the statements of
 *     oracle.condition.ray_cast; the keypoint rays of dwg_condition_keypoints make the same choice); equal t: the lower triangle index;
 *   - primitive_normals = normalize(cross(v1 - v0, v2 - v0)) of the hit triangle, not flipped towards the camera; a miss gives zero.
 *
 * All pointers are device pointers; nothing is allocated inside and nothing is read back; every launch goes to `stream` and can be
 * captured.  No float atomics and no data-dependent list sizes: two calls give the same bits.  Every entry point returns DWG_E_ARG
 * before any launch on a bad argument.  Triangles with an index outside [0, V) are never read and never hit.
 */
#ifndef DWG_DEPTHMAP_H
#define DWG_DEPTHMAP_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_DEPTHMAP_MAX_SIZE 16384 /* H and W at most (the triangle boxes are stored as 16-bit pixel indices) */

/* Bytes of workspace of dwg_depthmap_cast / dwg_depthmap_image: a fixed function of the sizes (per-triangle records and boxes, and the
 * two words of the image's minimum / maximum).  0 when H <= 0, W <= 0 or F < 0. */
size_t dwg_depthmap_workspace_bytes(int32_t H, int32_t W, int32_t F);

/* extrinsic [4,4] row-major world -> camera, intrinsics [3,3] already adjusted to H x W, vertices [V,3] fp32, triangles [F,3] int32
 * (F == 0: every pixel misses) -> t_hit [H,W] fp32, normals [H,W,3] fp32 (NULL: not written).  want_minmax != 0 also leaves the minimum
 * and maximum of 1 / t_hit in the workspace for dwg_depthmap_image(..., minmax_from_cast = 1).  workspace: 16-byte aligned,
 * dwg_depthmap_workspace_bytes(H, W, F) bytes. */
int dwg_depthmap_cast(int32_t H, int32_t W, const float* extrinsic, const float* intrinsics, int32_t V, const float* vertices, int32_t F,
                      const int32_t* triangles, float* t_hit, float* normals, int32_t want_minmax, void* workspace, size_t workspace_bytes,
                      dwg_stream_t stream);

/* export_depth(inverse=True, normalize=True) in fp32 as numpy does it: d = 1 / t; d -= min(d); d /= max(d); uint8(d * 255) truncating,
 * replicated to three channels.  Either output may be NULL: out_u8 [H,W,3], out_chw [3,H,W] fp32 = byte / 255.  An image whose maximum
 * is 0 after the subtraction (all misses) is all zero; the reference's 0 / 0 is not reproduced.  minmax_from_cast = 0: the minimum and
 * maximum are taken here (one more launch); 1: they are the ones dwg_depthmap_cast left in the SAME workspace for the SAME map. */
int dwg_depthmap_image(int32_t H, int32_t W, const float* t_hit, int32_t minmax_from_cast, uint8_t* out_u8, float* out_chw,
                       void* workspace, size_t workspace_bytes, dwg_stream_t stream);

/* Bytes of workspace of dwg_pretrain_loss_forward (per-workgroup partial sums).  0 when N <= 0. */
size_t dwg_pretrain_loss_workspace_bytes(int64_t N);

/* render_depth, render_ws [N] of `dtype` (DWG_DTYPE_F32 or DWG_DTYPE_F16), smpl_depth [N] fp32 (NaN and +-inf count as 0) ->
 * loss [1] fp32 = mean((ws - mask)^2) + mean((depth - sd)^2).  Differences and squares in fp32; the sums run in a fixed order
 * (per-workgroup partials, then one finishing launch). */
int dwg_pretrain_loss_forward(int32_t dtype, int64_t N, const void* render_depth, const void* render_ws, const float* smpl_depth,
                              float* loss, void* workspace, size_t workspace_bytes, dwg_stream_t stream);

/* grad_loss [1] fp32 in device memory (a GradScaler's scale arrives there) -> grad_depth = 2 (depth - sd) / N * g and
 * grad_ws = 2 (ws - mask) / N * g, [N] of `dtype`; either may be NULL. */
int dwg_pretrain_loss_backward(int32_t dtype, int64_t N, const void* render_depth, const void* render_ws, const float* smpl_depth,
                               const float* grad_loss, void* grad_depth, void* grad_ws, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
