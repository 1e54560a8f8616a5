/*
 * include/dwg_scene_cull.h -- C-ABI of the per-camera cull of the static 3D-Gaussian scene (boundary B25; the scene itself:
 * dwg_scene_gaussians.h).  The scene does not change between playback frames and the camera is pinned or on a track, yet every frame
 * pushes every scene Gaussian through the merge and the rasterizer's per-Gaussian stages, which then give most of them radius 0.  These
 * three entries run in front of the rasterizer, once per (scene, cameras, image size):
 *
 *   dwg_scene_cull_flags     one lane per scene Gaussian: flag = 1 if the Gaussian MAY have a non-empty tile rectangle under any of the
 *                            n_cameras cameras (the union: one culled block serves every frame of a batch with per-frame cameras).
 *                            The test is csrc/cull_math.h: conservative -- never 0 for a Gaussian the rasterizer gives radius > 0 at
 *                            scale_modifier 1 -- and evaluated with every operation rounded on its own (FP contraction off, correctly
 *                            rounded division and sqrt): a host build gives the same flags bit for bit.
 *   dwg_scene_cull_compact   the indices of the flagged Gaussians, ascending, as int32, and their count in a device word: a deterministic
 *                            three-launch scan (csrc/scan_common.h).  No atomics: the order never depends on timing.
 *   dwg_scene_cull_gather    rows index[0 .. kept) of up to DWG_SCENE_CULL_MAX_ROWS dense fp32 tables into compact tables, one launch.
 *
 * Cameras are read from device memory: blocks of DWG_SCENE_CULL_CAMERA_FLOATS floats in the layout dwg_raster_camera_block writes
 * ([viewmatrix 16 | projmatrix 16 | campos 3 | tanfovx | tanfovy]), `camera_stride` floats apart.
 *
 * All pointers are device pointers, 4-byte aligned (flags: any alignment).  The gather moves one float per lane and access: rows of 4,
 * 12, 16 or 180 bytes start at arbitrary 4-byte aligned offsets, and no wide access ever touches an unaligned address.  An index outside
 * [0, n_total) is skipped, never dereferenced.  Two runs are bit-identical.  Every entry returns DWG_E_ARG before any launch on a bad
 * argument; an empty call (no Gaussians, no kept rows, no tables) returns DWG_OK without a launch (compact: after zeroing the count).
 */
#ifndef DWG_SCENE_CULL_H
#define DWG_SCENE_CULL_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_SCENE_CULL_MAX_CAMERAS 64
#define DWG_SCENE_CULL_CAMERA_FLOATS 37
#define DWG_SCENE_CULL_MAX_ROWS 8

/* positions [n, 3], scales [n, 3] (activated), cameras: n_cameras blocks in 1 .. DWG_SCENE_CULL_MAX_CAMERAS, camera_stride >=
 * DWG_SCENE_CULL_CAMERA_FLOATS floats apart, image_height x image_width pixels -> flags [n] bytes, 0 or 1.  n < 2^31. */
int dwg_scene_cull_flags(int64_t n, const float* positions, const float* scales, int32_t n_cameras, const float* cameras,
                         int64_t camera_stride, int32_t image_height, int32_t image_width, uint8_t* flags, dwg_stream_t stream);

/* bytes of `workspace` for dwg_scene_cull_compact over n flags (0 for a bad n) */
size_t dwg_scene_cull_workspace_bytes(int64_t n);

/* flags [n] -> index: the i with flags[i] != 0, ascending, in index[0 .. count) (room for n entries); count[0] = their number. */
int dwg_scene_cull_compact(int64_t n, const uint8_t* flags, int32_t* index, uint32_t* count, void* workspace, dwg_stream_t stream);

/* One table of a gather: dst[k, :] = src[index[k], :] for rows of `width` floats, both dense. */
typedef struct dwg_scene_cull_rows {
    const float* src;
    float* dst;
    int32_t width;
} dwg_scene_cull_rows;

/* index [kept] with values in [0, n_total); tables[0 .. n_tables): src [n_total, width] -> dst [kept, width], width in 1 .. 64.  A dst
 * may not alias a src. */
int dwg_scene_cull_gather(int64_t kept, const int32_t* index, int64_t n_total, int32_t n_tables, const dwg_scene_cull_rows* tables,
                          dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
