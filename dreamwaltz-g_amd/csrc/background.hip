// background.hip -- video background compositing (include/dwg_background.h, boundary B5): one lane per output pixel of F frames, the
// source pixel fetched from a device-resident uint8 BGR frame store, resampled with OpenCV's 8-bit INTER_LINEAR rule when the sizes
// differ, divided by 255 and composited as `fg + bg * (1 - alpha)`.
//
// Also here (boundary B23, the stage-II learned MLP background): the view directions of every pixel of F cameras, and the composite of a
// background image read from memory with its backward to alpha and to that image -- the same `Layout` and the same statements.
//
// Traffic per 512^2 frame: 12 B fg + 4 B alpha read, 12 B image + 12 B image_bg written per pixel (~10.5 MB) plus the source bytes;
// a few microseconds at HBM rates.  fg / image / d_image take the caller's strides: the renderer's image is a channel-planar view
// ([F, 3, H, W] permuted), and the composite keeps that layout as torch's elementwise ops would.  The backward recomputes the
// background instead of reading a saved fp32 copy (3 source bytes against 12).  Every float operation is rounded on its own: with equal sizes the result is the reference's statements bit for bit.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_background.h"
#include "view_math.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kCoefScale = 2048;          // OpenCV INTER_RESIZE_COEF_SCALE (11 bits)

enum Mode : int { kEqual = 0, kLinear = 1, kArea2x = 2 };

struct Src {
    const uint8_t* frames;
    int T, h, w;
    const int* frame_index;
    int mode;
    double scale_x, scale_y;
};

__device__ __forceinline__ int frame_of(const Src& s, int f) {
    int t = s.frame_index[f];
    if (t < 0) t += s.T;
    return min(max(t, 0), s.T - 1);
}

// the source value of output pixel (dy, dx), channel order of the store (BGR), as OpenCV's cv2.resize leaves it in uint8
__device__ __forceinline__ void fetch(const Src& s, const uint8_t* img, int dy, int dx, int v[3]) {
    const int w = s.w, h = s.h;
    if (s.mode == kEqual) {
        const uint8_t* p = img + ((size_t)dy * w + dx) * 3;
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
        return;
    }
    if (s.mode == kArea2x) {
        const uint8_t* p0 = img + ((size_t)(2 * dy) * w + 2 * dx) * 3;
        const uint8_t* p1 = p0 + (size_t)w * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = (p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
        return;
    }
    // columns: clamped coefficients
    float fx = (float)(((double)dx + 0.5) * s.scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx = fx - (float)sx;
    if (sx < 0) { fx = 0.f; sx = 0; }
    if (sx >= w - 1) { fx = 0.f; sx = w - 1; }
    const int a0 = (int)rintf((1.f - fx) * (float)kCoefScale), a1 = (int)rintf(fx * (float)kCoefScale);
    const int sx1 = min(sx + 1, w - 1);
    // rows: clamped row indices, unclamped coefficients
    float fy = (float)(((double)dy + 0.5) * s.scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy = fy - (float)sy;
    const int b0 = (int)rintf((1.f - fy) * (float)kCoefScale), b1 = (int)rintf(fy * (float)kCoefScale);
    const int y0 = min(max(sy, 0), h - 1), y1 = min(max(sy + 1, 0), h - 1);
    const uint8_t* r0 = img + (size_t)y0 * w * 3;
    const uint8_t* r1 = img + (size_t)y1 * w * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int S0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
        const int S1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
        v[c] = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    }
}

// RGB background of output pixel p of frame f, v / 255 as an IEEE division (the reference divides on the host)
__device__ __forceinline__ void background(const Src& s, int f, int dy, int dx, float bg[3]) {
    const uint8_t* img = s.frames + (size_t)frame_of(s, f) * s.h * s.w * 3;
    int v[3];
    fetch(s, img, dy, dx, v);
    bg[0] = (float)v[2] / 255.0f;
    bg[1] = (float)v[1] / 255.0f;
    bg[2] = (float)v[0] / 255.0f;
}

struct Layout {
    int64_t sf, sp, sc;           // element strides of fg / image / d_image: frame, pixel (y * W + x), channel
};

__global__ __launch_bounds__(kBlock) void k_video_composite(int W, int HW, const float* __restrict__ fg, const float* __restrict__ alpha,
                                                            Layout L, Src s, float* __restrict__ image, float* __restrict__ image_bg) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const int f = blockIdx.y;
    const int dy = p / W, dx = p - dy * W;
    float bg[3];
    background(s, f, dy, dx, bg);
    const size_t px = (size_t)f * HW + p;
    if (image_bg) {
#pragma unroll
        for (int c = 0; c < 3; c++) image_bg[px * 3 + c] = bg[c];
    }
    if (image) {
        const float om = 1.0f - alpha[px];
        const int64_t q = (int64_t)f * L.sf + (int64_t)p * L.sp;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float t = bg[c] * om;
            image[q + c * L.sc] = fg[q + c * L.sc] + t;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_video_composite_bwd(int W, int HW, const float* __restrict__ d_image, Layout L, Src s,
                                                                float* __restrict__ d_alpha) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const int f = blockIdx.y;
    const int dy = p / W, dx = p - dy * W;
    float bg[3];
    background(s, f, dy, dx, bg);
    const size_t px = (size_t)f * HW + p;
    const float* g = d_image + (int64_t)f * L.sf + (int64_t)p * L.sp;
    float acc = g[0] * bg[0];
    acc = acc + g[L.sc] * bg[1];
    acc = acc + g[2 * L.sc] * bg[2];
    d_alpha[px] = -acc;
}

// ---- the learned (MLP) background of stage II (boundary B23) -----------------------------------------------------------------------
// One lane per pixel of F cameras: get_rays' direction (view_math.h view_ray: pixel centre, safe_normalize, rotation), then the
// reference's second normalisation d / ||d|| as a plain division (core/system/background.py:78).
__global__ __launch_bounds__(kBlock) void k_background_dirs(int W, int HW, const float* __restrict__ cameras, float* __restrict__ dirs) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const int f = blockIdx.y;
    const float* cam = cameras + (size_t)f * DWG_BACKGROUND_CAMERA_FLOATS;
    const float K[9] = {cam[12], 0.f, cam[14], 0.f, cam[13], cam[15], 0.f, 0.f, 1.f};
    const int row = p / W, col = p - row * W;
    float d[3];
    view_ray(cam, K, (uint32_t)row, (uint32_t)col, d);
    const float s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float len = sqrtf(s);
    float* o = dirs + ((size_t)f * HW + p) * 3;
    o[0] = d[0] / len; o[1] = d[1] / len; o[2] = d[2] / len;
}

// image = fg + bg * (1 - alpha): the statements of k_video_composite with the background read from memory (bg_sf: its frame stride in
// elements, 0 when all frames share one background).
__global__ __launch_bounds__(kBlock) void k_mlp_composite(int HW, const float* __restrict__ fg, const float* __restrict__ alpha, Layout L,
                                                          const float* __restrict__ bg, int64_t bg_sf, float* __restrict__ image) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const int f = blockIdx.y;
    const size_t px = (size_t)f * HW + p;
    const float* b = bg + (int64_t)f * bg_sf + (int64_t)p * 3;
    const float om = 1.0f - alpha[px];
    const int64_t q = (int64_t)f * L.sf + (int64_t)p * L.sp;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float t = b[c] * om;
        image[q + c * L.sc] = fg[q + c * L.sc] + t;
    }
}

// d_alpha = -((d_r bg_r + d_g bg_g) + d_b bg_b), d_bg = d * (1 - alpha); either output may be NULL.
__global__ __launch_bounds__(kBlock) void k_mlp_composite_bwd(int HW, const float* __restrict__ d_image, Layout L, const float* __restrict__ alpha,
                                                              const float* __restrict__ bg, float* __restrict__ d_alpha,
                                                              float* __restrict__ d_bg) {
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const int f = blockIdx.y;
    const size_t px = (size_t)f * HW + p;
    const float* g = d_image + (int64_t)f * L.sf + (int64_t)p * L.sp;
    const float g0 = g[0], g1 = g[L.sc], g2 = g[2 * L.sc];
    if (d_alpha) {
        const float* b = bg + px * 3;
        float acc = g0 * b[0];
        acc = acc + g1 * b[1];
        acc = acc + g2 * b[2];
        d_alpha[px] = -acc;
    }
    if (d_bg) {
        const float om = 1.0f - alpha[px];
        d_bg[px * 3] = g0 * om; d_bg[px * 3 + 1] = g1 * om; d_bg[px * 3 + 2] = g2 * om;
    }
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// the resample mode and scales of cv2.resize(frame, (W, H)) for an (h, w) frame; false on sizes the kernels do not take
bool plan(int32_t F, int32_t H, int32_t W, const uint8_t* frames, int32_t T, int32_t h, int32_t w, const int32_t* frame_index, Src& s) {
    if (F <= 0 || H <= 0 || W <= 0 || T <= 0 || h <= 0 || w <= 0) return false;
    if (F > 65535 || (int64_t)H * W > (int64_t)0x7fffffff - kBlock) return false;
    if ((int64_t)h * w * 3 > (int64_t)0x7fffffff) return false;     // per-frame offsets inside a row block stay in int
    if (!frames || !frame_index || !aligned4(frame_index)) return false;
    s.frames = frames; s.T = T; s.h = h; s.w = w; s.frame_index = frame_index;
    s.scale_x = 1.0 / ((double)W / (double)w);
    s.scale_y = 1.0 / ((double)H / (double)h);
    if (h == H && w == W) {
        s.mode = kEqual;
    } else {
        // OpenCV: INTER_LINEAR with integer scales of exactly 2 in both directions runs its fast area path
        const int ix = (int)lrint(s.scale_x), iy = (int)lrint(s.scale_y);
        const bool area_fast = fabs(s.scale_x - ix) < 2.220446049250313e-16 && fabs(s.scale_y - iy) < 2.220446049250313e-16;
        s.mode = (area_fast && ix == 2 && iy == 2 && h == 2 * H && w == 2 * W) ? kArea2x : kLinear;   // (the sizes: a guard)
    }
    return true;
}

}  // namespace

extern "C" {

int dwg_video_composite_forward(int32_t F, int32_t H, int32_t W, const float* fg, const float* alpha, int64_t sf, int64_t sp, int64_t sc,
                                const uint8_t* frames, int32_t T, int32_t h, int32_t w, const int32_t* frame_index, float* image,
                                float* image_bg, dwg_stream_t stream_) {
    Src s;
    if (!plan(F, H, W, frames, T, h, w, frame_index, s)) return DWG_E_ARG;
    const bool composite = fg || alpha || image;
    if (composite && (!fg || !alpha || !image)) return DWG_E_ARG;
    if (!composite && !image_bg) return DWG_E_ARG;
    if (!aligned4(fg) || !aligned4(alpha) || !aligned4(image) || !aligned4(image_bg)) return DWG_E_ARG;
    if (composite && (sf < 0 || sp < 0 || sc < 0)) return DWG_E_ARG;
    const Layout L{sf, sp, sc};
    const int HW = H * W;
    DWG_LAUNCH("video_composite", k_video_composite, dim3(dwg_cdiv(HW, kBlock), F), dim3(kBlock), 0, (hipStream_t)stream_, W, HW, fg,
               alpha, L, s, image, image_bg);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_video_composite_backward(int32_t F, int32_t H, int32_t W, const float* d_image, int64_t sf, int64_t sp, int64_t sc,
                                 const uint8_t* frames, int32_t T, int32_t h, int32_t w, const int32_t* frame_index, float* d_alpha,
                                 dwg_stream_t stream_) {
    Src s;
    if (!plan(F, H, W, frames, T, h, w, frame_index, s)) return DWG_E_ARG;
    if (!d_image || !d_alpha || !aligned4(d_image) || !aligned4(d_alpha) || sf < 0 || sp < 0 || sc < 0) return DWG_E_ARG;
    const Layout L{sf, sp, sc};
    const int HW = H * W;
    DWG_LAUNCH("video_composite_bwd", k_video_composite_bwd, dim3(dwg_cdiv(HW, kBlock), F), dim3(kBlock), 0, (hipStream_t)stream_, W, HW,
               d_image, L, s, d_alpha);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

static bool image_dims(int32_t F, int32_t H, int32_t W) {
    return F > 0 && H > 0 && W > 0 && F <= 65535 && (int64_t)H * W <= (int64_t)0x7fffffff - kBlock;
}

int dwg_background_dirs(int32_t F, const float* cameras, int32_t H, int32_t W, float* dirs, dwg_stream_t stream_) {
    if (!image_dims(F, H, W) || !cameras || !dirs || !aligned4(cameras) || !aligned4(dirs)) return DWG_E_ARG;
    const int HW = H * W;
    DWG_LAUNCH("background_dirs", k_background_dirs, dim3(dwg_cdiv(HW, kBlock), F), dim3(kBlock), 0, (hipStream_t)stream_, W, HW, cameras, dirs);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_mlp_composite_forward(int32_t F, int32_t H, int32_t W, const float* fg, const float* alpha, int64_t sf, int64_t sp, int64_t sc,
                              const float* bg, int64_t bg_frame_stride, float* image, dwg_stream_t stream_) {
    if (!image_dims(F, H, W) || !fg || !alpha || !bg || !image) return DWG_E_ARG;
    if (!aligned4(fg) || !aligned4(alpha) || !aligned4(bg) || !aligned4(image) || sf < 0 || sp < 0 || sc < 0) return DWG_E_ARG;
    const int HW = H * W;
    if (bg_frame_stride != 0 && bg_frame_stride != (int64_t)HW * 3) return DWG_E_ARG;
    const Layout L{sf, sp, sc};
    DWG_LAUNCH("mlp_composite", k_mlp_composite, dim3(dwg_cdiv(HW, kBlock), F), dim3(kBlock), 0, (hipStream_t)stream_, HW, fg, alpha, L, bg,
               bg_frame_stride, image);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_mlp_composite_backward(int32_t F, int32_t H, int32_t W, const float* d_image, int64_t sf, int64_t sp, int64_t sc, const float* alpha,
                               const float* bg, float* d_alpha, float* d_bg, dwg_stream_t stream_) {
    if (!image_dims(F, H, W) || !d_image || !aligned4(d_image) || sf < 0 || sp < 0 || sc < 0) return DWG_E_ARG;
    if ((!d_alpha && !d_bg) || (d_alpha && !bg) || (d_bg && !alpha)) return DWG_E_ARG;
    if (!aligned4(alpha) || !aligned4(bg) || !aligned4(d_alpha) || !aligned4(d_bg)) return DWG_E_ARG;
    const Layout L{sf, sp, sc};
    const int HW = H * W;
    DWG_LAUNCH("mlp_composite_bwd", k_mlp_composite_bwd, dim3(dwg_cdiv(HW, kBlock), F), dim3(kBlock), 0, (hipStream_t)stream_, HW, d_image, L,
               alpha, bg, d_alpha, d_bg);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
