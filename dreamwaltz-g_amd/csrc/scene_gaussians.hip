// scene_gaussians.hip -- the static 3D-Gaussian scene behind the avatars (include/dwg_scene_gaussians.h; reference scene.py:123-132,
// gaussian_model.py:35-94): the activations once per parameter change, and ONE streaming launch per frame that writes the avatars' rows and
// the scene's rows into the buffers the rasterizer reads (the reference: five activations, a 48-float cat and five torch.cat per frame).
// 112 B moved per Gaussian (28 floats read, 28 written); at sh_levels > 1 the scene rows read 192 B more (dc + 45 floats of the higher bands).
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "sh_math.h"
#include "scene_args.h"

namespace {

constexpr int kAttrs = 5;
constexpr int kMaxJobs = DWG_SCENE_MAX_PARTS * kAttrs;

__global__ __launch_bounds__(256) void k_scene_activate(long long n, const float* __restrict__ logits, const float* __restrict__ log_scales,
                                                        const float* __restrict__ quats, const float* __restrict__ dc,
                                                        float* __restrict__ opac, float* __restrict__ scales, float* __restrict__ quats_out,
                                                        float* __restrict__ colors) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    opac[i] = dwg_scene_sigmoid(logits[i]);
    float q[4], qn[4];
    for (int c = 0; c < 4; c++) q[c] = quats[4 * i + c];
    dwg_scene_normalize(q, 4, qn);
    for (int c = 0; c < 4; c++) quats_out[4 * i + c] = qn[c];
    for (int c = 0; c < 3; c++) {
        scales[3 * i + c] = expf(log_scales[3 * i + c]);
        colors[3 * i + c] = dwg_scene_dc_color(dc[3 * i + c]);
    }
}

// the view-dependent colour rows of the scene block: one lane per Gaussian
struct ViewJob {
    const float* positions; const float* dc; const float* rest; const float* cam; float* colors;
    long long rows, cam_stride; int levels;
};

__device__ __forceinline__ void view_rows(const ViewJob& v) {
    const float cam[3] = {v.cam[0], v.cam[v.cam_stride], v.cam[2 * v.cam_stride]};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < v.rows; i += (long long)gridDim.x * 256) {
        const float p[3] = {v.positions[3 * i], v.positions[3 * i + 1], v.positions[3 * i + 2]};
        float col[3];
        dwg_scene_view_color(v.levels, v.dc + 3 * i, v.rest + 3 * DWG_SCENE_SH_REST * i, p, cam, col);
        for (int c = 0; c < 3; c++) v.colors[3 * i + c] = col[c];
    }
}

__global__ __launch_bounds__(256) void k_scene_colors(ViewJob v) { view_rows(v); }

struct MergeJobs {
    const float* src[kMaxJobs];
    float* dst[kMaxJobs];
    long long count[kMaxJobs];          // floats
    int n;
    ViewJob view;                       // rows > 0: job `n` of the grid
};

// count floats from src to dst.  The destination is written 16 bytes at a time at 16-byte aligned addresses only: scalar stores up to the
// first such address and behind the last.  The source is read 16 bytes at a time when it is aligned at those chunks too, else float by float.
__device__ __forceinline__ void copy_floats(const float* __restrict__ src, float* __restrict__ dst, long long count) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, threads = (long long)gridDim.x * 256;
    long long head = (long long)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
    if (head > count) head = count;
    if (tid < head) dst[tid] = src[tid];
    const float* __restrict__ s = src + head;
    float* __restrict__ d = dst + head;
    const long long chunks = (count - head) >> 2;
    if (((uintptr_t)s & 15u) == 0) {
        for (long long i = tid; i < chunks; i += threads) reinterpret_cast<float4*>(d)[i] = reinterpret_cast<const float4*>(s)[i];
    } else {
        for (long long i = tid; i < chunks; i += threads)
            reinterpret_cast<float4*>(d)[i] = make_float4(s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]);
    }
    const long long done = head + 4 * chunks;
    if (tid < count - done) dst[done + tid] = src[done + tid];
}

__global__ __launch_bounds__(256) void k_scene_merge(MergeJobs J) {
    const int j = blockIdx.y;
    if (j < J.n) copy_floats(J.src[j], J.dst[j], J.count[j]);
    else view_rows(J.view);
}

int grid_x(long long longest, long long per_block) {
    long long b = (longest + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

extern "C" {

int dwg_scene_gaussians_activate(int64_t n, const float* opacity_logits, const float* log_scales, const float* quaternions,
                                 const float* sh_dc, float* opacities, float* scales, float* quaternions_out, float* colors,
                                 dwg_stream_t stream) {
    if (!dwg_scene_check_activate(n, opacity_logits, log_scales, quaternions, sh_dc, opacities, scales, quaternions_out, colors)) return DWG_E_ARG;
    if (n == 0) return DWG_OK;
    if ((n + 255) / 256 > 0x7fffffffLL) return DWG_E_ARG;
    DWG_LAUNCH("scene_gaussians_activate", k_scene_activate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n,
               opacity_logits, log_scales, quaternions, sh_dc, opacities, scales, quaternions_out, colors);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_scene_gaussians_colors(int64_t n, const float* positions, const float* sh_dc, const float* sh_rest, int32_t sh_levels,
                               const float* camera_position, int64_t camera_stride, float* colors, dwg_stream_t stream) {
    if (!dwg_scene_check_colors(n, positions, sh_dc, sh_rest, sh_levels, camera_position, camera_stride, colors)) return DWG_E_ARG;
    if (n == 0) return DWG_OK;
    ViewJob v = {};
    v.positions = positions; v.dc = sh_dc; v.rest = sh_rest; v.cam = sh_levels > 1 ? camera_position : sh_dc; v.colors = colors;
    v.rows = n; v.cam_stride = sh_levels > 1 ? camera_stride : 0; v.levels = sh_levels;
    if (sh_levels == 1) v.positions = sh_dc;            // not used by the level-1 statement; any readable address
    DWG_LAUNCH("scene_gaussians_colors", k_scene_colors, dim3(grid_x(n, 256)), dim3(256), 0, (hipStream_t)stream, v);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_scene_merge(int32_t n_parts, const dwg_scene_part* parts, int32_t sh_levels, const float* sh_dc, const float* sh_rest,
                    const float* camera_position, int64_t camera_stride, int64_t capacity, float* positions, float* opacities,
                    float* colors, float* scales, float* quaternions, dwg_stream_t stream) {
    int64_t total = 0;
    if (!dwg_scene_check_merge(n_parts, parts, sh_levels, sh_dc, sh_rest, camera_position, camera_stride, capacity, positions, opacities, colors,
                               scales, quaternions, &total))
        return DWG_E_ARG;
    if (total == 0) return DWG_OK;
    MergeJobs J = {};
    float* const out[kAttrs] = {positions, opacities, colors, scales, quaternions};
    const int width[kAttrs] = {3, 1, 3, 3, 4};
    long long row = 0, longest = 0, view_blocks = 0;
    for (int i = 0; i < n_parts; i++) {
        const dwg_scene_part& p = parts[i];
        if (p.count == 0) continue;
        const float* const in[kAttrs] = {p.positions, p.opacities, p.colors, p.scales, p.quaternions};
        for (int a = 0; a < kAttrs; a++) {
            if (a == 2 && sh_levels > 1 && i == n_parts - 1) {
                ViewJob& v = J.view;
                v.positions = p.positions; v.dc = sh_dc; v.rest = sh_rest; v.cam = camera_position; v.colors = colors + row * 3;
                v.rows = p.count; v.cam_stride = camera_stride; v.levels = sh_levels;
                view_blocks = grid_x(p.count, 256);
                continue;
            }
            J.src[J.n] = in[a]; J.dst[J.n] = out[a] + row * width[a]; J.count[J.n] = (long long)p.count * width[a];
            if (J.count[J.n] > longest) longest = J.count[J.n];
            J.n++;
        }
        row += p.count;
    }
    long long gx = grid_x(longest, 2048);               // 256 lanes, two 16-byte chunks each per pass
    if (view_blocks > gx) gx = view_blocks;
    DWG_LAUNCH("scene_merge", k_scene_merge, dim3((unsigned)gx, (unsigned)(J.n + (J.view.rows > 0 ? 1 : 0))), dim3(256), 0, (hipStream_t)stream, J);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
