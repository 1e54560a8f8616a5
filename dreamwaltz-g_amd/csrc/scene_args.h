// scene_args.h -- the argument checks of include/dwg_scene_gaussians.h's entries: plain host code with no HIP call, so that a
// stand-alone program can run them (and csrc/sh_math.h) under the host sanitizers.  1 = good, 0 = DWG_E_ARG.
#pragma once
#include <stdint.h>

#include "../../include/dwg_scene_gaussians.h"

static inline int dwg_scene_ok4(const void* p) { return p && ((uintptr_t)p & 3u) == 0; }

static inline int dwg_scene_check_activate(int64_t n, const void* logits, const void* log_scales, const void* quats, const void* sh_dc,
                                           const void* opac, const void* scales, const void* quats_out, const void* colors) {
    if (n < 0) return 0;
    if (n == 0) return 1;
    const void* all[8] = {logits, log_scales, quats, sh_dc, opac, scales, quats_out, colors};
    for (int i = 0; i < 8; i++)
        if (!dwg_scene_ok4(all[i])) return 0;
    for (int i = 0; i < 4; i++)
        for (int o = 4; o < 8; o++)
            if (all[i] == all[o]) return 0;
    return 1;
}

static inline int dwg_scene_check_view(int32_t levels, const void* positions, const void* sh_dc, const void* sh_rest, const void* cam,
                                       int64_t cam_stride) {
    if (levels < 1 || levels > 4) return 0;
    if (levels == 1) return 1;
    return dwg_scene_ok4(positions) && dwg_scene_ok4(sh_dc) && dwg_scene_ok4(sh_rest) && dwg_scene_ok4(cam) && cam_stride >= 1;
}

static inline int dwg_scene_check_colors(int64_t n, const void* positions, const void* sh_dc, const void* sh_rest, int32_t levels,
                                         const void* cam, int64_t cam_stride, const void* colors) {
    if (n < 0 || levels < 1 || levels > 4) return 0;
    if (n == 0) return 1;
    if (!dwg_scene_ok4(sh_dc) || !dwg_scene_ok4(colors)) return 0;
    return dwg_scene_check_view(levels, positions, sh_dc, sh_rest, cam, cam_stride);
}

// -> 1 and *total = the sum of the counts; the last part's colours may be NULL when they are evaluated (levels > 1)
static inline int dwg_scene_check_merge(int32_t n_parts, const dwg_scene_part* parts, int32_t levels, const void* sh_dc, const void* sh_rest,
                                        const void* cam, int64_t cam_stride, int64_t capacity, const void* positions, const void* opacities,
                                        const void* colors, const void* scales, const void* quaternions, int64_t* total) {
    *total = 0;
    if (n_parts < 0 || n_parts > DWG_SCENE_MAX_PARTS || levels < 1 || levels > 4 || capacity < 0) return 0;
    if (n_parts == 0) return 1;
    if (!parts) return 0;
    int64_t sum = 0;
    for (int i = 0; i < n_parts; i++) {
        const dwg_scene_part* p = &parts[i];
        if (p->count < 0 || p->count > capacity - sum) return 0;
        sum += p->count;
        if (p->count == 0) continue;
        const int evaluated = levels > 1 && i == n_parts - 1;
        if (!dwg_scene_ok4(p->positions) || !dwg_scene_ok4(p->opacities) || !dwg_scene_ok4(p->scales) || !dwg_scene_ok4(p->quaternions)) return 0;
        if (evaluated ? ((uintptr_t)p->colors & 3u) != 0 : !dwg_scene_ok4(p->colors)) return 0;
        if (evaluated && !dwg_scene_check_view(levels, p->positions, sh_dc, sh_rest, cam, cam_stride)) return 0;
    }
    if (sum == 0) return 1;
    if (!dwg_scene_ok4(positions) || !dwg_scene_ok4(opacities) || !dwg_scene_ok4(colors) || !dwg_scene_ok4(scales) || !dwg_scene_ok4(quaternions))
        return 0;
    *total = sum;
    return 1;
}
