// scene_cull_args.h -- the argument checks of include/dwg_scene_cull.h's entries: plain host code with no HIP call, so that a stand-alone
// program can run them (and csrc/cull_math.h) under the host sanitizers.  1 = good, 0 = DWG_E_ARG.
#pragma once
#include <stdint.h>

#include "../../include/dwg_scene_cull.h"

#define DWG_SCENE_CULL_MAX_WIDTH 64            /* floats per row of a gathered table */
#define DWG_SCENE_CULL_MAX_IMAGE 0x7fff0       /* pixels per image edge: rtiles * RT + RT stays far inside int and exact in fp32 */

static inline int dwg_scene_cull_ok4(const void* p) { return p && ((uintptr_t)p & 3u) == 0; }

// the scan counts in 32 bits and the indices are int32
static inline int dwg_scene_cull_ok_n(int64_t n) { return n >= 0 && n <= 0x7fffffffLL; }

static inline int dwg_scene_cull_check_flags(int64_t n, const void* positions, const void* scales, int32_t n_cameras, const void* cameras,
                                             int64_t camera_stride, int32_t image_height, int32_t image_width, const void* flags) {
    if (!dwg_scene_cull_ok_n(n)) return 0;
    if (n_cameras < 1 || n_cameras > DWG_SCENE_CULL_MAX_CAMERAS || camera_stride < DWG_SCENE_CULL_CAMERA_FLOATS) return 0;
    if (image_height < 1 || image_width < 1 || image_height > DWG_SCENE_CULL_MAX_IMAGE || image_width > DWG_SCENE_CULL_MAX_IMAGE) return 0;
    if (n == 0) return 1;
    return dwg_scene_cull_ok4(positions) && dwg_scene_cull_ok4(scales) && dwg_scene_cull_ok4(cameras) && flags != 0;
}

static inline int dwg_scene_cull_check_compact(int64_t n, const void* flags, const void* index, const void* count, const void* workspace) {
    if (!dwg_scene_cull_ok_n(n) || !dwg_scene_cull_ok4(count)) return 0;
    if (n == 0) return 1;
    return flags != 0 && dwg_scene_cull_ok4(index) && dwg_scene_cull_ok4(workspace);
}

// -> 1 and *widest = the largest row width of the tables
static inline int dwg_scene_cull_check_gather(int64_t kept, const void* index, int64_t n_total, int32_t n_tables,
                                              const dwg_scene_cull_rows* tables, int32_t* widest) {
    *widest = 0;
    if (!dwg_scene_cull_ok_n(n_total) || kept < 0 || kept > n_total) return 0;
    if (n_tables < 0 || n_tables > DWG_SCENE_CULL_MAX_ROWS) return 0;
    if (kept == 0 || n_tables == 0) return 1;
    if (!dwg_scene_cull_ok4(index) || !tables) return 0;
    for (int i = 0; i < n_tables; i++) {
        const dwg_scene_cull_rows* t = &tables[i];
        if (t->width < 1 || t->width > DWG_SCENE_CULL_MAX_WIDTH) return 0;
        if (!dwg_scene_cull_ok4(t->src) || !dwg_scene_cull_ok4(t->dst) || (const void*)t->src == (const void*)t->dst) return 0;
        if (t->width > *widest) *widest = t->width;
    }
    return 1;
}
