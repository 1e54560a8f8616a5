/*
 * include/dwg_scene_gaussians.h -- C-ABI of the static 3D-Gaussian scene behind the avatars (boundary B24: the reference's
 * `--render.use_gs_background PATH`, a GaussianModel loaded from a .ply and merged into every frame, core/system/scene.py:123-132 and
 * core/gaussian/gaussian_model.py:35-94).
 *
 * The reference re-runs five activations over all scene Gaussians per frame, concatenates the 48-float SH tensor to read its first
 * coefficient, and merges with one torch.cat per attribute.  Here:
 *
 *   dwg_scene_gaussians_activate   once per parameter change: opacity = 1 / (1 + exp(-logit)); scales = exp(log scales);
 *                                  quaternion = q / max(sqrt(((q0^2 + q1^2) + q2^2) + q3^2), 1e-12) (F.normalize; a zero row gives 0);
 *                                  DC colour = max(C0 * dc + 0.5, 0) (gaussian_utils.py:12-17 at sh_levels = 1).  Positions are not copied.
 *   dwg_scene_gaussians_colors     the view-dependent colour of sh_levels 2..4 on its own (what dwg_scene_merge evaluates in place)
 *   dwg_scene_merge                once per rendered frame: rows of up to DWG_SCENE_MAX_PARTS parts (the avatars, then the scene block)
 *                                  go to rows [0, sum of counts) of the five buffers the rasterizer reads, in the order of the reference's
 *                                  merge_gaussians(avatars..., background).
 *
 * View-dependent colour (sh_levels L in 2..4): dir = (p - cam) / max(sqrt((dx^2 + dy^2) + dz^2), 1e-12), eval_sh of degree L - 1 over
 * coefficient 0 from sh_dc and coefficients 1 .. L^2 - 1 from sh_rest, in the statement order of core/gaussian/spherical_harmonics.py
 * (csrc/sh_math.h), + 0.5, max(., 0).  The camera position is read from device memory: a captured frame follows a moving camera.
 *
 * All pointers are device pointers to fp32, 4-byte aligned.  The merge is a streaming copy: per segment the destination is walked in
 * 16-byte aligned chunks (scalar stores up to the first aligned address and after the last), and the source is read 16 bytes at a time
 * only when it is aligned at the same chunks -- no wide access ever touches an unaligned address.  No atomics; every float operation
 * is rounded on its own (FP contraction off inside every function of csrc/sh_math.h, correctly rounded division and sqrt); two runs are
 * bit-identical.  Every entry point returns DWG_E_ARG before any launch on a bad argument; an empty call (no rows) returns DWG_OK
 * without a launch.
 */
#ifndef DWG_SCENE_GAUSSIANS_H
#define DWG_SCENE_GAUSSIANS_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_SCENE_MAX_PARTS 17          /* 16 avatars (DWG_CONDITION_MAX_PEOPLE) and the scene block */
#define DWG_SCENE_SH_REST 15            /* coefficients 1..15 of a degree-3 file: sh_rest is [n, 15, 3] */

/* opacity_logits [n] or [n, 1], log_scales [n, 3], quaternions [n, 4], sh_dc [n, 1, 3] -> opacities [n, 1], scales [n, 3],
 * quaternions_out [n, 4], colors [n, 3].  Inputs are read in place; an output may not alias an input. */
int dwg_scene_gaussians_activate(int64_t n, const float* opacity_logits, const float* log_scales, const float* quaternions,
                                 const float* sh_dc, float* opacities, float* scales, float* quaternions_out, float* colors,
                                 dwg_stream_t stream);

/* positions [n, 3], sh_dc [n, 1, 3], sh_rest [n, 15, 3], sh_levels in 1..4, camera_position: 3 floats `camera_stride` elements apart
 * (1: dense; 4: the translation column of a row-major c2w) -> colors [n, 3]. */
int dwg_scene_gaussians_colors(int64_t n, const float* positions, const float* sh_dc, const float* sh_rest, int32_t sh_levels,
                               const float* camera_position, int64_t camera_stride, float* colors, dwg_stream_t stream);

/* One part of a frame: `count` rows of positions [count, 3], opacities [count, 1], colors [count, 3], scales [count, 3] and
 * quaternions [count, 4], each dense. */
typedef struct dwg_scene_part {
    const float* positions;
    const float* opacities;
    const float* colors;
    const float* scales;
    const float* quaternions;
    int64_t count;
} dwg_scene_part;

/* parts[0 .. n_parts) in order -> rows [0, sum of counts) of positions / opacities / colors / scales / quaternions, each with room for
 * `capacity` rows (a larger sum is DWG_E_ARG).  sh_levels = 1: every part's colours are copied.  sh_levels in 2..4: the LAST part is the
 * scene block -- its `colors` may be NULL -- and its colour rows are evaluated in the same launch from sh_dc / sh_rest (that part's
 * rows), its `positions` and the camera position.  sh_dc, sh_rest and camera_position are ignored at sh_levels = 1. */
int dwg_scene_merge(int32_t n_parts, const dwg_scene_part* parts, int32_t sh_levels, const float* sh_dc, const float* sh_rest,
                    const float* camera_position, int64_t camera_stride, int64_t capacity, float* positions, float* opacities,
                    float* colors, float* scales, float* quaternions, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
