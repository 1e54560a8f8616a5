/* Host build of csrc/sh_math.h and csrc/scene_args.h for tests/test_gs_background_host.py: the scene Gaussians' activations, the colour
 * of sh_levels 1..4 over arrays, and the merge's argument check. */
#include "../../dreamwaltz-g_amd/csrc/sh_math.h"
#include "../../dreamwaltz-g_amd/csrc/scene_args.h"

void host_scene_activate(int64_t n, const float* logits, const float* quats, const float* dc, float* opac, float* quats_out, float* colors) {
    for (int64_t i = 0; i < n; ++i) {
        opac[i] = dwg_scene_sigmoid(logits[i]);
        dwg_scene_normalize(quats + 4 * i, 4, quats_out + 4 * i);
        for (int c = 0; c < 3; ++c) colors[3 * i + c] = dwg_scene_dc_color(dc[3 * i + c]);
    }
}

void host_scene_colors(int64_t n, int levels, const float* positions, const float* dc, const float* rest, const float* cam, float* colors) {
    for (int64_t i = 0; i < n; ++i) dwg_scene_view_color(levels, dc + 3 * i, rest + 45 * i, positions + 3 * i, cam, colors + 3 * i);
}

int host_scene_check_merge(int32_t n_parts, const dwg_scene_part* parts, int32_t levels, int64_t capacity, const void* any, int64_t* total) {
    return dwg_scene_check_merge(n_parts, parts, levels, any, any, any, 4, capacity, any, any, any, any, any, total);
}
