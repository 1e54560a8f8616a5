// adam.hip -- the fused Adam on flat fp32 buffers (boundary O2; include/dwg_elementwise.h, include/dwg_grad_scaler.h): one group with the
// step's scalars as kernel arguments (dwg_adam_step) or read from a device table (dwg_adam_step_dev), up to DWG_ADAM_MAX_GROUPS groups in
// one launch (dwg_adam_step_groups_dev), and that launch under the loss scaler, whose skip flag leaves a group untouched (.._scaled_dev).
// One statement (adam_math.h adam_update) and one loop (adam_span): all four entry points write the same bits from the same scalars.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_elementwise.h"
#include "../../include/dwg_grad_scaler.h"
#include "adam_math.h"

namespace {

// One group's n floats: grid-stride over the float4s (16-byte accesses), then the n % 4 tail one float per lane.  The pointers are not
// __restrict__ here: k_adam's are, as kernel arguments, and the grouped kernels' (loaded from the group table) have never been to the
// compiler -- qualifying them here would reorder the grouped kernels' tail loads and change their register count.
__device__ __forceinline__ void adam_span(size_t n, float* p, const float* g, float* m, float* v, float step, float bc2_sqrt,
                                          float grad_scale, float b1, float b2, float eps) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256, n4 = n / 4;
    float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m); float4* v4 = reinterpret_cast<float4*>(v);
    for (size_t k = i; k < n4; k += stride) {
        float4 pp = p4[k], gg = g4[k], mm = m4[k], vv = v4[k];
        adam_update(&pp.x, gg.x, &mm.x, &vv.x, step, bc2_sqrt, grad_scale, b1, b2, eps);
        adam_update(&pp.y, gg.y, &mm.y, &vv.y, step, bc2_sqrt, grad_scale, b1, b2, eps);
        adam_update(&pp.z, gg.z, &mm.z, &vv.z, step, bc2_sqrt, grad_scale, b1, b2, eps);
        adam_update(&pp.w, gg.w, &mm.w, &vv.w, step, bc2_sqrt, grad_scale, b1, b2, eps);
        p4[k] = pp; m4[k] = mm; v4[k] = vv;
    }
    for (size_t k = n4 * 4 + i; k < n; k += stride) adam_update(p + k, g[k], m + k, v + k, step, bc2_sqrt, grad_scale, b1, b2, eps);
}

// `hyper` != nullptr: the per-step scalars come from DEVICE memory -- hyper[0] = lr / (1 - b1^t), hyper[1] = sqrt(1 - b2^t), hyper[2] =
// grad_scale -- so that the launch can sit inside a captured graph whose replays see the learning-rate schedule and the step count move.
__global__ __launch_bounds__(256) void k_adam(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                              float grad_scale, const float* __restrict__ hyper) {
    float step = lr / bc1;
    if (hyper) { step = hyper[0]; bc2_sqrt = hyper[1]; grad_scale = hyper[2]; }
    adam_span(n, p, g, m, v, step, bc2_sqrt, grad_scale, b1, b2, eps);
}

struct AdamGroups { dwg_adam_group g[DWG_ADAM_MAX_GROUPS]; };

// k_adam for several parameter groups: blockIdx.y = group (groups shorter than the grid's x extent leave their surplus workgroups idle).
// SKIP (the step under the loss scaler): the row's fourth float is read first, and a non-zero one returns before p, m or v is touched; the
// unscale rides in the row's gradient factor, so a taken step differs from the unscaled kernel's only through the value of grad_scale.
// Without SKIP the fourth float is not read at all.
template <bool SKIP>
__global__ __launch_bounds__(256) void k_adam_groups(AdamGroups G, const float* __restrict__ hyper) {
    const dwg_adam_group a = G.g[blockIdx.y];
    const float* h = hyper + 4 * (size_t)a.hyper_row;
    if (SKIP && h[3] != 0.f) return;
    const size_t n = (size_t)a.n, n4 = n / 4, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4 && n4 * 4 + i >= n) return;
    adam_span(n, a.param, a.grad, a.exp_avg, a.exp_avg_sq, h[0], h[1], h[2], a.beta1, a.beta2, a.eps);
}

// Workgroups of 256 lanes, one float4 per lane per pass, at most 2048 of them (the grid-stride loop takes the rest).
unsigned adam_blocks(int64_t n) {
    const size_t blocks = ((size_t)n / 4 + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > 2048 ? 2048 : blocks);
}

bool adam_buffers_ok(const float* p, const float* g, const float* m, const float* v) {
    return p && g && m && v && !(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16);
}

// Validates `groups`, copies the non-empty ones into G (`used` of them); returns the grid's x extent (the widest group's), 0 on a bad argument.
unsigned adam_compact_groups(int32_t count, const dwg_adam_group* groups, const float* hyper, AdamGroups& G, int& used) {
    used = 0;
    if (count < 0 || count > DWG_ADAM_MAX_GROUPS || !hyper || (count > 0 && !groups)) return 0;
    unsigned blocks = 1;
    for (int i = 0; i < count; i++) {
        const dwg_adam_group& a = groups[i];
        if (a.n < 0 || a.hyper_row < 0) return 0;
        if (a.n == 0) continue;
        if (!adam_buffers_ok(a.param, a.grad, a.exp_avg, a.exp_avg_sq)) return 0;
        G.g[used++] = a;
        blocks = adam_blocks(a.n) > blocks ? adam_blocks(a.n) : blocks;
    }
    return blocks;
}

// The single-group launch: k_adam's scalar arguments as the caller states them.
int adam_launch(int64_t n, float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, float bc2_sqrt,
                float grad_scale, const float* hyper, dwg_stream_t stream) {
    if (n == 0) return DWG_OK;
    if (!adam_buffers_ok(p, g, m, v)) return DWG_E_ARG;
    DWG_LAUNCH("adam_step", k_adam, dim3(adam_blocks(n)), dim3(256), 0, (hipStream_t)stream, (size_t)n, p, g, m, v, lr, b1, b2, eps, 1.f,
               bc2_sqrt, grad_scale, hyper);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

template <bool SKIP>
int adam_launch_groups(const char* name, int32_t count, const dwg_adam_group* groups, const float* hyper, dwg_stream_t stream) {
    AdamGroups G;
    int used;
    const unsigned blocks = adam_compact_groups(count, groups, hyper, G, used);
    if (!blocks) return DWG_E_ARG;
    if (used == 0) return DWG_OK;
    DWG_LAUNCH_W(name, SKIP ? "k_adam_groups<true>" : "k_adam_groups<false>", 0.0, k_adam_groups<SKIP>, dim3(blocks, used), dim3(256), 0,
                 (hipStream_t)stream, G, hyper);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // namespace

extern "C" {

int dwg_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                  float beta2, float eps, int32_t step, float grad_scale, dwg_stream_t stream) {
    if (n < 0 || step < 1) return DWG_E_ARG;
    // The step's two scalars by the statements that fill the device table of a captured step (FlatOptimizer.prepare_step for
    // dwg_adam_step_dev) and of a scaled one (k_scaler_prepare): an eager step and a replay of the captured one run k_adam on identical bits.
    // row[2] = (float)((double)grad_scale / 1.0) is grad_scale itself (fp32 -> double and / 1.0 are exact), so it goes through as it came.
    float row[4];
    adam_hyper_row(lr, beta1, beta2, step, grad_scale, 1.f, row);
    return adam_launch(n, param, grad, exp_avg, exp_avg_sq, row[0], beta1, beta2, eps, row[1], grad_scale, nullptr, stream);
}

int dwg_adam_step_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* hyper, float beta1,
                      float beta2, float eps, dwg_stream_t stream) {
    if (n < 0 || !hyper) return DWG_E_ARG;
    return adam_launch(n, param, grad, exp_avg, exp_avg_sq, 0.f, beta1, beta2, eps, 1.f, 1.f, hyper, stream);
}

int dwg_adam_step_groups_dev(int32_t count, const dwg_adam_group* groups, const float* hyper, dwg_stream_t stream) {
    return adam_launch_groups<false>("adam_step", count, groups, hyper, stream);
}

int dwg_adam_step_groups_scaled_dev(int32_t count, const dwg_adam_group* groups, const float* hyper, dwg_stream_t stream) {
    return adam_launch_groups<true>("adam_step_scaled", count, groups, hyper, stream);
}

}  // extern "C"
