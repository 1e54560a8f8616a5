// grad_scaler.hip -- the device-resident loss scaler of the stage-I step under optim.fp16 (boundary B21, include/dwg_grad_scaler.h):
// the Inf / NaN scan of the flat gradient, the one-workgroup decision (skip flag, step counts, this step's Adam scalars with the unscale
// folded in) and the scale schedule.  The fused Adam that honours the skip flag (dwg_adam_step_groups_scaled_dev) is adam.hip's, with the
// other Adam launches.  Nothing here reads back to the host.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_grad_scaler.h"
#include "scaler_math.h"

namespace {

// A pure stream: 16-byte loads, grid-stride over the float4s (grid capped at DWG_SCALER_MAX_SLOTS workgroups), the n % 4 tail by
// workgroup 0.  Every workgroup writes its own slot on every call -- no atomics, no clearing launch.
__global__ __launch_bounds__(256) void k_grads_nonfinite(size_t n, const float* __restrict__ g, int32_t* __restrict__ slots) {
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * 256;
    const uint4* g4 = reinterpret_cast<const uint4*>(g);
    int bad = 0;
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n4; k += stride) {
        const uint4 v = g4[k];
        bad |= scaler_nonfinite_bits(v.x) | scaler_nonfinite_bits(v.y) | scaler_nonfinite_bits(v.z) | scaler_nonfinite_bits(v.w);
    }
    if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) bad |= scaler_nonfinite(g[n4 * 4 + threadIdx.x]);
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) slots[blockIdx.x] = any ? 1 : 0;
}

struct ScalerBetas { float beta1[DWG_ADAM_MAX_GROUPS], beta2[DWG_ADAM_MAX_GROUPS]; };

// One workgroup.  The decision is global (any slot of any workgroup of the scan), which is why it cannot ride in the Adam launch: a
// skipped step must leave p, m and v untouched everywhere, and no workgroup of that launch knows the answer before all slots exist.
__global__ __launch_bounds__(256) void k_scaler_prepare(int nslots, const int32_t* __restrict__ slots, dwg_scaler_state* __restrict__ state,
                                                        float* __restrict__ found, int groups, uint32_t mask, const float* __restrict__ lr,
                                                        ScalerBetas B, float grad_scale, int32_t* __restrict__ steps,
                                                        float* __restrict__ hyper) {
    int bad = 0;
    for (int i = threadIdx.x; i < nslots; i += 256) bad |= slots[i];
    const int f = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        found[0] = f ? 1.f : 0.f;
        if (f) state->found_inf = 1.f;
    }
    const int g = threadIdx.x;
    if (g >= groups) return;
    float4 row = make_float4(0.f, 1.f, 0.f, 1.f);
    if (!f) {
        if (!((mask >> g) & 1u)) { hyper[4 * g + 3] = 0.f; return; }
        const int32_t t = steps[g] + 1;
        steps[g] = t;
        float r[4];
        adam_hyper_row(lr[g], B.beta1[g], B.beta2[g], t, grad_scale, state->scale, r);
        row = make_float4(r[0], r[1], r[2], r[3]);
    }
    reinterpret_cast<float4*>(hyper)[g] = row;
}

__global__ void k_scaler_update(dwg_scaler_state* __restrict__ state, double growth_factor, double backoff_factor, int32_t growth_interval) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float scale = state->scale;
    int32_t tracker = state->growth_tracker;
    scaler_update(&scale, &tracker, state->found_inf != 0.f, growth_factor, backoff_factor, growth_interval);
    state->scale = scale;
    state->growth_tracker = tracker;
    state->found_inf = 0.f;
}

}  // namespace

extern "C" {

int32_t dwg_grads_nonfinite_slots(int64_t n) {
    if (n <= 0) return 0;
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > DWG_SCALER_MAX_SLOTS) blocks = DWG_SCALER_MAX_SLOTS;
    return (int32_t)blocks;
}

int dwg_grads_nonfinite(int64_t n, const float* grad, int32_t* slots, dwg_stream_t stream) {
    if (n <= 0 || !grad || !slots || (uintptr_t)grad % 16 || (uintptr_t)slots % 4) return DWG_E_ARG;
    DWG_LAUNCH("grads_nonfinite", k_grads_nonfinite, dim3((unsigned)dwg_grads_nonfinite_slots(n)), dim3(256), 0, (hipStream_t)stream,
               (size_t)n, grad, slots);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_scaler_prepare(int32_t nslots, const int32_t* slots, dwg_scaler_state* state, float* found, int32_t groups, uint32_t mask,
                       const float* lr, const float* beta1, const float* beta2, float grad_scale, int32_t* steps, float* hyper,
                       dwg_stream_t stream) {
    if (nslots < 1 || nslots > DWG_SCALER_MAX_SLOTS || !slots || !state || !found || groups < 0 || groups > DWG_ADAM_MAX_GROUPS) return DWG_E_ARG;
    if (groups > 0 && (!lr || !beta1 || !beta2 || !steps || !hyper)) return DWG_E_ARG;
    if ((uintptr_t)state % 16 || (uintptr_t)hyper % 16 || (groups < 32 && (mask >> groups))) return DWG_E_ARG;
    ScalerBetas B = {};
    for (int g = 0; g < groups; g++) { B.beta1[g] = beta1[g]; B.beta2[g] = beta2[g]; }
    DWG_LAUNCH("scaler_prepare", k_scaler_prepare, dim3(1), dim3(256), 0, (hipStream_t)stream, (int)nslots, slots, state, found, (int)groups,
               mask, lr, B, grad_scale, steps, hyper);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_scaler_update(dwg_scaler_state* state, double growth_factor, double backoff_factor, int32_t growth_interval, dwg_stream_t stream) {
    if (!state || (uintptr_t)state % 16 || growth_interval < 1) return DWG_E_ARG;
    DWG_LAUNCH("scaler_update", k_scaler_update, dim3(1), dim3(1), 0, (hipStream_t)stream, state, growth_factor, backoff_factor, growth_interval);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
