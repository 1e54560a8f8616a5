// adan.hip -- the fused Adan optimizer on flat fp32 buffers (boundary B23, include/dwg_adan.h): the sum of squares of the gradient in
// per-workgroup fp64 partials, the one-workgroup preparation (clipping factor, step counts, every group's scalars) and the update of
// all participating groups in one launch.  The arithmetic is csrc/adan_math.h's, shared with the host test.  Nothing reads back.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_adan.h"
#include "adan_math.h"

namespace {

constexpr int kBlock = 256;

// A pure stream: 16-byte loads, grid-stride over the float4s (grid capped at DWG_ADAN_MAX_SLOTS workgroups), the n % 4 tail by workgroup
// 0.  The squares are exact in fp64; a lane adds its own in index order, the workgroup's 256 lane sums are added by a fixed tree.  Every
// workgroup writes its own slot on every call -- no atomics, no clearing launch.
__global__ __launch_bounds__(kBlock) void k_adan_sumsq(size_t n, const float* __restrict__ g, double* __restrict__ partials) {
    __shared__ double red[kBlock];
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * kBlock;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    double acc = 0.0;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < n4; k += stride) {
        const float4 v = g4[k];
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    if (blockIdx.x == 0 && n4 * 4 + threadIdx.x < n) {
        const double t = (double)g[n4 * 4 + threadIdx.x];
        acc += t * t;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

struct AdanHypers { dwg_adan_hyper h[DWG_ADAN_MAX_GROUPS]; };

// One workgroup.  The clipping factor is global (every slot of the scan), which is why it cannot ride in the update launch: no workgroup
// of that launch knows the total before all slots exist.
__global__ __launch_bounds__(kBlock) void k_adan_prepare(int nslots, const double* __restrict__ partials, int groups, AdanHypers H,
                                                         uint32_t first_mask, double max_grad_norm, double grad_scale,
                                                         int32_t* __restrict__ steps, float* __restrict__ rows) {
    __shared__ double slot[DWG_ADAN_MAX_SLOTS];
    __shared__ double total;
    for (int i = threadIdx.x; i < nslots; i += kBlock) slot[i] = partials[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < nslots; i++) t += slot[i];          // slot order
        total = t;
    }
    __syncthreads();
    const int g = threadIdx.x;
    if (g >= groups) return;
    const double clip = nslots > 0 ? adan_clip(total, max_grad_norm, grad_scale, H.h[groups - 1].eps) : 1.0;
    const int32_t t = steps[g] + 1;
    steps[g] = t;
    const dwg_adan_hyper& h = H.h[g];
    float r[ADAN_ROW_FLOATS];
    adan_hyper_row(h.lr, h.beta1, h.beta2, h.beta3, h.eps, h.weight_decay, h.no_prox, t, t == 1 || ((first_mask >> g) & 1u), clip, grad_scale, r);
    float4* out = reinterpret_cast<float4*>(rows + (size_t)g * DWG_ADAN_ROW);
    out[0] = make_float4(r[0], r[1], r[2], r[3]);
    out[1] = make_float4(r[4], r[5], r[6], r[7]);
    out[2] = make_float4(r[8], r[9], r[10], r[11]);
    out[3] = make_float4(r[12], r[13], r[14], r[15]);
}

struct AdanGroups { dwg_adan_group g[DWG_ADAN_MAX_GROUPS]; };

// grid (workgroups, groups): a pure stream of five reads and five writes of 16 bytes per four elements.
__global__ __launch_bounds__(kBlock) void k_adan_groups(AdanGroups G, const float* __restrict__ rows) {
    const dwg_adan_group a = G.g[blockIdx.y];
    float row[ADAN_ROW_FLOATS];
    {
        const float4* h4 = reinterpret_cast<const float4*>(rows + (size_t)a.hyper_row * DWG_ADAN_ROW);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float4 v = h4[k];
            row[4 * k] = v.x; row[4 * k + 1] = v.y; row[4 * k + 2] = v.z; row[4 * k + 3] = v.w;
        }
    }
    const size_t n = (size_t)a.n, n4 = n / 4;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * kBlock;
    float* __restrict__ p = a.param; const float* __restrict__ g = a.grad; float* __restrict__ m = a.exp_avg;
    float* __restrict__ s = a.exp_avg_sq; float* __restrict__ v = a.exp_avg_diff; float* __restrict__ q = a.neg_pre_grad;
    float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m); float4* s4 = reinterpret_cast<float4*>(s);
    float4* v4 = reinterpret_cast<float4*>(v); float4* q4 = reinterpret_cast<float4*>(q);
    for (size_t k = i; k < n4; k += stride) {
        float4 pp = p4[k], mm = m4[k], ss = s4[k], vv = v4[k], qq = q4[k];
        const float4 gg = g4[k];
        adan_update(row, gg.x, &pp.x, &mm.x, &ss.x, &vv.x, &qq.x);
        adan_update(row, gg.y, &pp.y, &mm.y, &ss.y, &vv.y, &qq.y);
        adan_update(row, gg.z, &pp.z, &mm.z, &ss.z, &vv.z, &qq.z);
        adan_update(row, gg.w, &pp.w, &mm.w, &ss.w, &vv.w, &qq.w);
        p4[k] = pp; m4[k] = mm; s4[k] = ss; v4[k] = vv; q4[k] = qq;
    }
    for (size_t k = n4 * 4 + i; k < n; k += stride) {
        float pp = p[k], mm = m[k], ss = s[k], vv = v[k], qq = q[k];
        adan_update(row, g[k], &pp, &mm, &ss, &vv, &qq);
        p[k] = pp; m[k] = mm; s[k] = ss; v[k] = vv; q[k] = qq;
    }
}

}  // namespace

extern "C" {

int32_t dwg_adan_sumsq_slots(int64_t n) {
    if (n <= 0) return 0;
    int64_t blocks = (n / 4 + kBlock - 1) / kBlock;
    if (blocks < 1) blocks = 1;
    if (blocks > DWG_ADAN_MAX_SLOTS) blocks = DWG_ADAN_MAX_SLOTS;
    return (int32_t)blocks;
}

int dwg_adan_sumsq(int64_t n, const float* grad, double* partials, dwg_stream_t stream) {
    if (n <= 0 || !grad || !partials || (uintptr_t)grad % 16 || (uintptr_t)partials % 8) return DWG_E_ARG;
    DWG_LAUNCH("adan_sumsq", k_adan_sumsq, dim3((unsigned)dwg_adan_sumsq_slots(n)), dim3(kBlock), 0, (hipStream_t)stream, (size_t)n, grad,
               partials);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_adan_prepare(int32_t nslots, const double* partials, int32_t groups, const dwg_adan_hyper* hyper, uint32_t first_mask,
                     double max_grad_norm, double grad_scale, int32_t* steps, float* rows, dwg_stream_t stream) {
    if (groups < 1 || groups > DWG_ADAN_MAX_GROUPS || !hyper || !steps || !rows || (uintptr_t)steps % 4 || (uintptr_t)rows % 16) return DWG_E_ARG;
    if (nslots < 0 || nslots > DWG_ADAN_MAX_SLOTS || (nslots > 0 && (!partials || (uintptr_t)partials % 8))) return DWG_E_ARG;
    if (!(max_grad_norm >= 0.0) || (max_grad_norm > 0.0 && nslots == 0) || (max_grad_norm == 0.0 && nslots != 0)) return DWG_E_ARG;
    if (groups < 32 && (first_mask >> groups)) return DWG_E_ARG;
    AdanHypers H = {};
    for (int g = 0; g < groups; g++) {
        const dwg_adan_hyper& h = hyper[g];
        if (!(h.lr >= 0.0) || !(h.eps >= 0.0) || !(h.beta1 >= 0.0 && h.beta1 < 1.0) || !(h.beta2 >= 0.0 && h.beta2 < 1.0) ||
            !(h.beta3 >= 0.0 && h.beta3 < 1.0))
            return DWG_E_ARG;
        H.h[g] = h;
    }
    DWG_LAUNCH("adan_prepare", k_adan_prepare, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, (int)nslots, partials, (int)groups, H,
               first_mask, max_grad_norm, grad_scale, steps, rows);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_adan_step_groups_dev(int32_t count, const dwg_adan_group* groups, const float* rows, dwg_stream_t stream) {
    if (count < 0 || count > DWG_ADAN_MAX_GROUPS || !rows || (uintptr_t)rows % 16 || (count > 0 && !groups)) return DWG_E_ARG;
    AdanGroups G;
    size_t blocks = 0;
    int used = 0;
    for (int i = 0; i < count; i++) {
        const dwg_adan_group& a = groups[i];
        if (a.n < 0 || a.hyper_row < 0 || a.hyper_row >= DWG_ADAN_MAX_GROUPS) return DWG_E_ARG;
        if (a.n == 0) continue;
        if (!a.param || !a.grad || !a.exp_avg || !a.exp_avg_sq || !a.exp_avg_diff || !a.neg_pre_grad) return DWG_E_ARG;
        if (((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq | (uintptr_t)a.exp_avg_diff |
             (uintptr_t)a.neg_pre_grad) % 16)
            return DWG_E_ARG;
        G.g[used++] = a;
        size_t b = ((size_t)a.n / 4 + kBlock - 1) / kBlock;
        if (b < 1) b = 1;
        blocks = b > blocks ? b : blocks;
    }
    if (used == 0) return DWG_OK;
    if (blocks > 2048) blocks = 2048;
    DWG_LAUNCH("adan_step", k_adan_groups, dim3((unsigned)blocks, used), dim3(kBlock), 0, (hipStream_t)stream, G, rows);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
