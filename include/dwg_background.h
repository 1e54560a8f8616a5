/*
 * include/dwg_background.h -- C-ABI of the video background compositing (boundary B5, the reference's VideoBackground:
 * core/system/background.py:92-160 and core/system/scene.py:157-160).
 *
 * The reference takes the decoded BGR uint8 frame, converts it to RGB, resizes it to the render size with cv2.resize (INTER_LINEAR)
 * when the sizes differ, divides by 255 on the host and composites `image + image_bg * (1 - alpha)`.  Here the frames live on the
 * device as the decoder wrote them (uint8 [T, h, w, 3], BGR) and one launch covers F frames whose indices are read from device memory,
 * so that a captured graph can replay with another index.
 *
 *   dwg_video_composite_forward    image = fg + bg * (1 - alpha), and the background itself (image_bg)
 *   dwg_video_composite_backward   d_alpha = -(d_image_r * bg_r + d_image_g * bg_g + d_image_b * bg_b), summed in that order.
 *                                  d_fg = d_image: the caller uses d_image itself.
 *
 * Per output pixel: the source pixel, BGR -> RGB; the resample below when (h, w) != (H, W); bg = v / 255.0f as an IEEE division;
 * then 1 - alpha, bg * that, fg + that, each rounded on its own (no contraction).  With equal sizes the result is bit-identical to the
 * reference's statements.
 *
 * Resampling (OpenCV's INTER_LINEAR rule for 8-bit images; restated in tests/video_background_cases.py):
 *   scale_x = 1 / ((double)W / w), scale_y = 1 / ((double)H / h)
 *   exact 2x downscale (scale_x == scale_y == 2): OpenCV's fast area path, dst = (s00 + s01 + s10 + s11 + 2) >> 2
 *   otherwise, per output column dx (rows alike):
 *     fx = (float)((dx + 0.5) * scale_x - 0.5); sx = floor(fx); fx -= sx
 *     columns only: sx < 0 -> sx = 0, fx = 0;  sx >= w - 1 -> sx = w - 1, fx = 0
 *     rows: the two source rows sy, sy + 1 are clamped to [0, h - 1]; fy itself is not
 *     11-bit coefficients (INTER_RESIZE_COEF_SCALE = 2048), rounded half to even: a0 = rint((1 - fx) * 2048), a1 = rint(fx * 2048)
 *     horizontal pass into integers: S = src[sx] * a0 + src[min(sx + 1, w - 1)] * a1
 *     vertical pass with rounding:   dst = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
 *   Against cv2.resize itself this is UNVERIFIED (cv2 is not available where this was written, and its SIMD / IPP code paths may round
 *   differently): the claim is +-1 on the uint8 value.
 *
 * Frame indices: a negative index counts from the end (t + T); an index still outside [0, T) is clamped for memory safety.  Range
 * checks that raise belong to the host API (dreamwaltz_g_amd.background).  All pointers are device pointers; float buffers must be
 * 4-byte aligned and strides non-negative.  Every entry point returns DWG_E_ARG before any launch on a bad argument.  No atomics: two
 * runs are bit-identical.
 */
#ifndef DWG_BACKGROUND_H
#define DWG_BACKGROUND_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fg [F, H, W, 3] fp32 at element strides (sf, sp, sc) per frame, pixel (y * W + x) and channel -- the renderer's image is a
 * channel-planar view: (3 H W, 1, H W) --, alpha [F, H, W, 1] fp32 contiguous, frames [T, h, w, 3] uint8 BGR contiguous, frame_index [F]
 * int32 -> image [F, H, W, 3] fp32 at fg's strides, image_bg [F, H, W, 3] fp32 RGB in [0, 1] contiguous (NULL: not written).
 * fg, alpha and image all NULL: only the background is written (image_bg required then; the strides are ignored). */
int dwg_video_composite_forward(int32_t F, int32_t H, int32_t W, const float* fg, const float* alpha, int64_t sf, int64_t sp, int64_t sc,
                                const uint8_t* frames, int32_t T, int32_t h, int32_t w, const int32_t* frame_index, float* image,
                                float* image_bg, dwg_stream_t stream);

/* d_image [F, H, W, 3] fp32 at element strides (sf, sp, sc) -> d_alpha [F, H, W, 1] fp32 contiguous (the background is recomputed
 * from the frames). */
int dwg_video_composite_backward(int32_t F, int32_t H, int32_t W, const float* d_image, int64_t sf, int64_t sp, int64_t sc,
                                 const uint8_t* frames, int32_t T, int32_t h, int32_t w, const int32_t* frame_index, float* d_alpha,
                                 dwg_stream_t stream);

/*
 * The learned (MLP) background of stage II (boundary B23, the reference's MLPBackground: core/system/background.py:55-89 and
 * core/system/scene.py:161-164).  The network itself is include/dwg_nerf_background.h's, unchanged; here are the two steps around it.
 *
 *   dwg_background_dirs           the unit view direction of every pixel of F cameras
 *   dwg_mlp_composite_forward     image = fg + bg * (1 - alpha), bg read from memory
 *   dwg_mlp_composite_backward    d_alpha = -((d_r bg_r + d_g bg_g) + d_b bg_b) and d_bg = d_image * (1 - alpha);
 *                                 d_fg = d_image: the caller uses d_image itself.
 * Every float operation is rounded on its own; no atomics.
 */
#define DWG_BACKGROUND_CAMERA_FLOATS 16

/* cameras [F][DWG_BACKGROUND_CAMERA_FLOATS] fp32: rows 0..2 of c2w (12 floats, row-major; the translation column is not read), then fx,
 * fy, cx, cy -> dirs [F * H * W, 3] fp32, pixel (row, col) of camera f at f * H * W + row * W + col.  Per pixel, in fp32: get_rays'
 * direction with N = -1 (core/nerf/nerf_utils.py:124-129) -- ((col + 0.5 - cx) / fx, (row + 0.5 - cy) / fy, 1), safe_normalize with its
 * clamp at 1e-20, times c2w[:3, :3]^T -- then d / sqrt((d_x^2 + d_y^2) + d_z^2), a plain division (background.py:78).  No origins. */
int dwg_background_dirs(int32_t F, const float* cameras, int32_t H, int32_t W, float* dirs, dwg_stream_t stream);

/* fg [F, H, W, 3] fp32 at element strides (sf, sp, sc) as in dwg_video_composite_forward, alpha [F, H, W, 1] fp32 contiguous, bg
 * [F, H, W, 3] fp32 contiguous (bg_frame_stride = H * W * 3) or one [H, W, 3] background shared by all frames (bg_frame_stride = 0)
 * -> image [F, H, W, 3] fp32 at fg's strides. */
int dwg_mlp_composite_forward(int32_t F, int32_t H, int32_t W, const float* fg, const float* alpha, int64_t sf, int64_t sp, int64_t sc,
                              const float* bg, int64_t bg_frame_stride, float* image, dwg_stream_t stream);

/* d_image [F, H, W, 3] fp32 at element strides (sf, sp, sc), alpha [F, H, W, 1] and bg [F, H, W, 3] fp32 contiguous -> d_alpha
 * [F, H, W, 1] and d_bg [F, H, W, 3] fp32 contiguous.  Either output may be NULL (not wanted; alpha is read for d_bg only, bg for
 * d_alpha only), not both. */
int dwg_mlp_composite_backward(int32_t F, int32_t H, int32_t W, const float* d_image, int64_t sf, int64_t sp, int64_t sc, const float* alpha,
                               const float* bg, float* d_alpha, float* d_bg, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
