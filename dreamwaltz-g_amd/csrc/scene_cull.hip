// scene_cull.hip -- the per-camera cull of the static 3D-Gaussian scene (include/dwg_scene_cull.h, boundary B25): conservative visibility
// flags (csrc/cull_math.h, one lane per scene Gaussian, the union over up to 64 cameras read from device memory), an order-preserving
// compaction of the flagged indices (scan_common.h's deterministic three-launch scan: no atomics decide an order) and one gather launch
// that copies the kept rows of the scene's tables into a compact block.  All of it runs once per (scene, cameras, image size), in front
// of the merge and the rasterizer, which then see only the rows that can reach the image.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "scan_common.h"
#include "cull_math.h"
#include "scene_cull_args.h"

namespace {

constexpr int kCam = DWG_SCENE_CULL_CAMERA_FLOATS;

__global__ __launch_bounds__(256) void k_cull_flags(long long n, const float* __restrict__ positions, const float* __restrict__ scales,
                                                    int n_cameras, const float* __restrict__ cameras, long long camera_stride, int H, int W,
                                                    uint8_t* __restrict__ flags) {
    __shared__ float cams[DWG_SCENE_CULL_MAX_CAMERAS * kCam];
    for (int t = threadIdx.x; t < n_cameras * kCam; t += 256) cams[t] = cameras[(long long)(t / kCam) * camera_stride + t % kCam];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]};
    const float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
    int keep = 0;
    for (int c = 0; c < n_cameras && !keep; c++) keep = dwg_cull_may_be_visible(p, s, cams + c * kCam, W, H);
    flags[i] = (uint8_t)keep;
}

// the scan's callbacks: item n counts 1 when it is flagged; a flagged item writes its own index at its offset
struct FlagCount {
    const uint8_t* flags;
    __device__ __forceinline__ uint32_t operator()(uint32_t n) const { return flags[n] ? 1u : 0u; }
};
struct IndexWrite {
    int32_t* index;
    __device__ __forceinline__ void operator()(uint32_t n, uint32_t offset, uint32_t count) const {
        if (count) index[offset] = (int32_t)n;
    }
};

struct GatherTables {
    const float* src[DWG_SCENE_CULL_MAX_ROWS];
    float* dst[DWG_SCENE_CULL_MAX_ROWS];
    int width[DWG_SCENE_CULL_MAX_ROWS];
};

// blockIdx.y = table; one float per lane and pass: consecutive lanes write consecutive floats of dst and read consecutive floats of a row
__global__ __launch_bounds__(256) void k_cull_gather(GatherTables T, long long kept, const int32_t* __restrict__ index, long long n_total) {
    const int t = blockIdx.y;
    const float* __restrict__ src = T.src[t];
    float* __restrict__ dst = T.dst[t];
    const int w = T.width[t];
    const long long floats = kept * w;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < floats; e += (long long)gridDim.x * 256) {
        const long long k = e / w;
        const int c = (int)(e - k * w);
        const long long row = index[k];
        if ((unsigned long long)row < (unsigned long long)n_total) dst[e] = src[row * w + c];
    }
}

}  // namespace

extern "C" {

int dwg_scene_cull_flags(int64_t n, const float* positions, const float* scales, int32_t n_cameras, const float* cameras,
                         int64_t camera_stride, int32_t image_height, int32_t image_width, uint8_t* flags, dwg_stream_t stream) {
    if (!dwg_scene_cull_check_flags(n, positions, scales, n_cameras, cameras, camera_stride, image_height, image_width, flags)) return DWG_E_ARG;
    if (n == 0) return DWG_OK;
    DWG_LAUNCH("scene_cull_flags", k_cull_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n, positions,
               scales, (int)n_cameras, cameras, (long long)camera_stride, (int)image_height, (int)image_width, flags);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_scene_cull_workspace_bytes(int64_t n) {
    if (!dwg_scene_cull_ok_n(n) || n == 0) return 0;
    return scan_workspace_bytes((uint32_t)n);
}

int dwg_scene_cull_compact(int64_t n, const uint8_t* flags, int32_t* index, uint32_t* count, void* workspace, dwg_stream_t stream) {
    if (!dwg_scene_cull_check_compact(n, flags, index, count, workspace)) return DWG_E_ARG;
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return DWG_E_LAUNCH;
        return DWG_OK;
    }
    scan_counts({"scene_cull_block_sums", "scene_cull_scan_sums", "scene_cull_scan_down"}, FlagCount{flags}, IndexWrite{index}, (uint32_t)n,
                (uint32_t*)workspace, count, false, (hipStream_t)stream);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_scene_cull_gather(int64_t kept, const int32_t* index, int64_t n_total, int32_t n_tables, const dwg_scene_cull_rows* tables,
                          dwg_stream_t stream) {
    int32_t widest = 0;
    if (!dwg_scene_cull_check_gather(kept, index, n_total, n_tables, tables, &widest)) return DWG_E_ARG;
    if (kept == 0 || n_tables == 0) return DWG_OK;
    GatherTables T = {};
    for (int i = 0; i < n_tables; i++) { T.src[i] = tables[i].src; T.dst[i] = tables[i].dst; T.width[i] = tables[i].width; }
    long long blocks = (kept * widest + 1023) / 1024;                 // four passes per lane on the widest table
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    DWG_LAUNCH("scene_cull_gather", k_cull_gather, dim3((unsigned)blocks, (unsigned)n_tables), dim3(256), 0, (hipStream_t)stream, T, (long long)kept,
               index, (long long)n_total);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
