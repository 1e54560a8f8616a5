/* Host build (g++) of csrc/cull_math.h and csrc/scene_cull_args.h for tests/test_scene_cull_host.py and tests/test_scene_cull_gpu.py: the
 * visibility flags of dwg_scene_cull_flags over arrays (the union over the cameras, as the kernel takes it) and the three argument checks.
 * With -DCULL_SELFCHECK_MAIN the same file is a stand-alone program (its own main, no Python) that walks the checks and the test over
 * edge inputs: what runs under -fsanitize=address,undefined. */
#include "../../dreamwaltz-g_amd/csrc/cull_math.h"
#include "../../dreamwaltz-g_amd/csrc/scene_cull_args.h"

extern "C" {

void host_cull_flags(int64_t n, const float* positions, const float* scales, int32_t n_cameras, const float* cameras, int64_t camera_stride,
                     int32_t H, int32_t W, uint8_t* flags) {
    for (int64_t i = 0; i < n; ++i) {
        int keep = 0;
        for (int c = 0; c < n_cameras && !keep; ++c) keep = dwg_cull_may_be_visible(positions + 3 * i, scales + 3 * i, cameras + c * camera_stride, W, H);
        flags[i] = (uint8_t)keep;
    }
}

int host_cull_check_flags(int64_t n, const void* positions, const void* scales, int32_t n_cameras, const void* cameras, int64_t camera_stride,
                          int32_t H, int32_t W, const void* flags) {
    return dwg_scene_cull_check_flags(n, positions, scales, n_cameras, cameras, camera_stride, H, W, flags);
}

int host_cull_check_compact(int64_t n, const void* flags, const void* index, const void* count, const void* workspace) {
    return dwg_scene_cull_check_compact(n, flags, index, count, workspace);
}

int host_cull_check_gather(int64_t kept, const void* index, int64_t n_total, int32_t n_tables, const dwg_scene_cull_rows* tables) {
    int32_t widest = 0;
    return dwg_scene_cull_check_gather(kept, index, n_total, n_tables, tables, &widest);
}

}  // extern "C"

#ifdef CULL_SELFCHECK_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

/* a pinhole camera at the origin looking down +z: view = identity, proj rows as the rasterizer reads them (element [4 c + k]) */
static void make_camera(float* cam, float tanfov) {
    for (int i = 0; i < DWG_SCENE_CULL_CAMERA_FLOATS; ++i) cam[i] = 0.f;
    for (int i = 0; i < 4; ++i) cam[5 * i] = 1.f;
    cam[16 + 0] = 1.f / tanfov; cam[16 + 5] = -1.f / tanfov; cam[16 + 10] = 1.f; cam[16 + 11] = 1.f; cam[16 + 14] = -0.02f;
    cam[35] = tanfov; cam[36] = tanfov;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float edge[] = {0.f, -0.f, 1e-30f, -1e-30f, 0.2f, 0.19998f, 0.2000001f, 1.f, -1.f, 3.4e38f, -3.4e38f, inf, -inf, nan};
    const int E = (int)(sizeof(edge) / sizeof(edge[0]));
    std::vector<float> cams(3 * DWG_SCENE_CULL_CAMERA_FLOATS);
    make_camera(cams.data(), 0.45f); make_camera(cams.data() + 37, 1e-3f); make_camera(cams.data() + 74, 50.f);
    cams[74 + 14] = nan;                                              /* a camera with a NaN translation */
    std::vector<float> pos, sc;
    for (int a = 0; a < E; ++a)
        for (int b = 0; b < E; ++b)
            for (int c = 0; c < E; ++c) {
                pos.push_back(edge[a]); pos.push_back(edge[b]); pos.push_back(edge[c]);
                sc.push_back(edge[c]); sc.push_back(edge[a]); sc.push_back(edge[b]);
            }
    const int64_t n = (int64_t)pos.size() / 3;
    std::vector<uint8_t> flags(n);
    long kept = 0;
    const int sizes[][2] = {{1, 1}, {64, 64}, {35, 67}, {1024, 1024}, {DWG_SCENE_CULL_MAX_IMAGE, DWG_SCENE_CULL_MAX_IMAGE}};
    for (const auto& hw : sizes)
        for (int C = 1; C <= 3; ++C) {
            host_cull_flags(n, pos.data(), sc.data(), C, cams.data(), 37, hw[0], hw[1], flags.data());
            for (uint8_t f : flags) kept += f;
        }
    /* a Gaussian in front of the camera is kept, one behind it is dropped */
    const float front[3] = {0.f, 0.f, 2.f}, behind[3] = {0.f, 0.f, -2.f}, s[3] = {0.01f, 0.01f, 0.01f};
    if (!dwg_cull_may_be_visible(front, s, cams.data(), 64, 64) || dwg_cull_may_be_visible(behind, s, cams.data(), 64, 64)) {
        printf("cull self-check: wrong answer for the plain cases\n");
        return 1;
    }
    /* the argument checks over good and bad arguments */
    float buf[8] = {0};
    int bad = 0;
    bad += host_cull_check_flags(4, buf, buf, 1, buf, 37, 64, 64, buf) != 1;
    bad += host_cull_check_flags(-1, buf, buf, 1, buf, 37, 64, 64, buf) != 0;
    bad += host_cull_check_flags(4, buf, buf, 0, buf, 37, 64, 64, buf) != 0;
    bad += host_cull_check_flags(4, buf, buf, 65, buf, 37, 64, 64, buf) != 0;
    bad += host_cull_check_flags(4, buf, buf, 1, buf, 36, 64, 64, buf) != 0;
    bad += host_cull_check_flags(4, (const char*)buf + 1, buf, 1, buf, 37, 64, 64, buf) != 0;
    bad += host_cull_check_flags(0, 0, 0, 1, 0, 37, 64, 64, 0) != 1;
    bad += host_cull_check_compact(4, buf, buf, buf, buf) != 1;
    bad += host_cull_check_compact(4, buf, buf, 0, buf) != 0;
    bad += host_cull_check_compact(0, 0, 0, buf, 0) != 1;
    bad += host_cull_check_compact((int64_t)1 << 31, buf, buf, buf, buf) != 0;
    dwg_scene_cull_rows rows[DWG_SCENE_CULL_MAX_ROWS] = {};
    for (int i = 0; i < DWG_SCENE_CULL_MAX_ROWS; ++i) { rows[i].src = buf; rows[i].dst = buf + 4; rows[i].width = 1 + i; }
    bad += host_cull_check_gather(2, buf, 4, DWG_SCENE_CULL_MAX_ROWS, rows) != 1;
    bad += host_cull_check_gather(5, buf, 4, 1, rows) != 0;
    bad += host_cull_check_gather(2, buf, 4, DWG_SCENE_CULL_MAX_ROWS + 1, rows) != 0;
    bad += host_cull_check_gather(0, 0, 4, 1, 0) != 1;
    rows[1].width = 65;
    bad += host_cull_check_gather(2, buf, 4, 2, rows) != 0;
    rows[1].width = 2; rows[1].dst = buf;
    bad += host_cull_check_gather(2, buf, 4, 2, rows) != 0;
    printf("cull self-check: %ld of %ld edge cases kept, %d wrong argument checks\n", kept, (long)(n * 15), bad);
    return bad ? 1 : 0;
}
#endif
