// avatar_init.hip -- the avatar constructor's geometry (include/dwg_avatar_init.h, boundary B11): barycentric coordinates of the closest
// points, interpolation of the per-vertex LBS weights, exact K nearest neighbours within the point cloud, the smoothing weights and the
// Jacobi sweeps of the LBS-weight smoothing.
//
// Sizes: N = 1e5 .. 3e5 points, V ~ 1e4 vertices, J = 55 joints, K = 30 neighbours, up to 5000 sweeps.  The one-lane-per-point kernels
// (barycentric, interp, weights) run once and cost microseconds.  The two that matter:
//   k_knn     brute force, one query per lane.  The reference points stream through a 256-point LDS tile that every lane reads as a
//             broadcast; the running K-list of a lane is a column of LDS ([K][lanes]: lane-consecutive, conflict-free), unsorted, with the
//             current worst entry's distance and slot in registers.  A candidate is a compare against that register; only an accepted one
//             touches LDS (overwrite the worst slot, rescan the column for the new worst: K independent reads).  References arrive in
//             index order, so "strictly closer than the worst" is exactly the (distance, index) order.  The column is emitted in order by
//             K selection passes at the end.
//   k_smooth  one sweep, one wave per point, lane j = column j: K coalesced 4 J-byte row reads from the previous sweep's buffer (the
//             neighbour ids and weights sit in lanes 0..K-1 and are broadcast by readlane), then the blend.  A point whose update weight
//             is 0 copies its row and reads nothing else.  The kernel boundary is the only hand-off between sweeps.
// No atomics anywhere: the result does not depend on scheduling.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_avatar_init.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kKnnLanes = 128;             // queries per k_knn workgroup: 2 x 64 x 128 x 4 B = 64 KB of lists at K = 64
constexpr int kKnnTile = 256;              // reference points staged per round (4 KB)
constexpr int kSmoothWaves = 4;            // points per k_smooth workgroup

__device__ __forceinline__ bool vert_ok(int v, int V) { return v >= 0 && v < V; }

__global__ __launch_bounds__(256) void k_barycentric(int N, const float* __restrict__ cp, const int* __restrict__ cf, int V,
                                                     const float* __restrict__ verts, int F, const int* __restrict__ faces,
                                                     float* __restrict__ bary, int* __restrict__ vidx, int* __restrict__ nearest) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int f = cf[i];
    float b[3] = {0.f, 0.f, 0.f};
    int t[3] = {-1, -1, -1}, nv = -1;
    if (f >= 0 && f < F) {
        const int* tf = faces + 3 * (size_t)f;
        const int t0 = tf[0], t1 = tf[1], t2 = tf[2];
        if (vert_ok(t0, V) && vert_ok(t1, V) && vert_ok(t2, V)) {
            t[0] = t0; t[1] = t1; t[2] = t2;
            double e0[3], e1[3], r[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double a = verts[3 * (size_t)t0 + k];
                e0[k] = (double)verts[3 * (size_t)t1 + k] - a;
                e1[k] = (double)verts[3 * (size_t)t2 + k] - a;
                r[k] = (double)cp[3 * (size_t)i + k] - a;
            }
            const double d00 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2], d01 = e0[0] * e1[0] + e0[1] * e1[1] + e0[2] * e1[2];
            const double d11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
            const double d20 = r[0] * e0[0] + r[1] * e0[1] + r[2] * e0[2], d21 = r[0] * e1[0] + r[1] * e1[1] + r[2] * e1[2];
            const double den = d00 * d11 - d01 * d01;
            const double b1 = (d11 * d20 - d01 * d21) / den, b2 = (d00 * d21 - d01 * d20) / den;
            b[0] = (float)(1.0 - b1 - b2); b[1] = (float)b1; b[2] = (float)b2;
            nv = t0;                                            // argmin, the first minimum winning
            float m = b[0];
            if (b[1] < m) { m = b[1]; nv = t1; }
            if (b[2] < m) { m = b[2]; nv = t2; }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        bary[3 * (size_t)i + k] = b[k];
        vidx[3 * (size_t)i + k] = t[k];
    }
    nearest[i] = nv;
}

__global__ __launch_bounds__(256) void k_lbs_interp(long long total, int J, int V, const float* __restrict__ table, const int* __restrict__ vidx,
                                                    const float* __restrict__ bary, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long n = e / J;
    const int j = (int)(e - n * J);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int v = vidx[3 * n + c];
        if (vert_ok(v, V)) {
            const float term = table[(size_t)v * J + j] * bary[3 * n + c];
            acc = c == 0 ? term : acc + term;
        }
    }
    out[e] = acc;
}

// LDS: tile [kKnnTile] float4 | list distances [K][kKnnLanes] | list indices [K][kKnnLanes]
__global__ __launch_bounds__(kKnnLanes) void k_knn(int Nq, const float* __restrict__ query, int Nr, const float* __restrict__ ref, int K,
                                                   int* __restrict__ idx, float* __restrict__ d2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* tile = reinterpret_cast<float4*>(smem);
    float* ld = reinterpret_cast<float*>(smem + sizeof(float4) * kKnnTile);
    int* li = reinterpret_cast<int*>(ld + (size_t)K * kKnnLanes);
    const int tid = threadIdx.x;
    const int q = blockIdx.x * kKnnLanes + tid;
    const bool valid = q < Nq;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (valid) { qx = query[3 * (size_t)q]; qy = query[3 * (size_t)q + 1]; qz = query[3 * (size_t)q + 2]; }
    for (int k = 0; k < K; k++) { ld[k * kKnnLanes + tid] = INFINITY; li[k * kKnnLanes + tid] = -1; }
    float thr = INFINITY;                  // (distance, slot) of the list's worst entry by (distance, index)
    int slot = 0;
    for (int base = 0; base < Nr; base += kKnnTile) {
        __syncthreads();
        for (int t = tid; t < kKnnTile; t += kKnnLanes) {
            const int r = base + t;
            tile[t] = r < Nr ? make_float4(ref[3 * (size_t)r], ref[3 * (size_t)r + 1], ref[3 * (size_t)r + 2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        if (!valid) continue;
        const int cnt = min(kKnnTile, Nr - base);
#pragma unroll 4
        for (int t = 0; t < cnt; t++) {
            const float4 p = tile[t];
            const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
            const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (d < thr) {                 // equal distance: the earlier (lower) index stays
                ld[slot * kKnnLanes + tid] = d;
                li[slot * kKnnLanes + tid] = base + t;
                float md = -INFINITY;
                int mi = INT_MIN, ms = 0;
                for (int k = 0; k < K; k++) {
                    const float pd = ld[k * kKnnLanes + tid];
                    const int pi = li[k * kKnnLanes + tid];
                    if (pd > md || (pd == md && pi > mi)) { md = pd; mi = pi; ms = k; }
                }
                thr = md; slot = ms;
            }
        }
    }
    if (!valid) return;
    float last_d = -INFINITY;
    int last_i = INT_MIN;
    for (int o = 0; o < K; o++) {          // emit in (distance, index) order: the smallest entry above the last one written
        float bd = INFINITY;
        int bi = INT_MAX;
        bool found = false;
        for (int k = 0; k < K; k++) {
            const float pd = ld[k * kKnnLanes + tid];
            const int pi = li[k * kKnnLanes + tid];
            const bool above = pd > last_d || (pd == last_d && pi > last_i);
            const bool below = pd < bd || (pd == bd && pi < bi);
            if (above && below) { bd = pd; bi = pi; found = true; }
        }
        if (found) { last_d = bd; last_i = bi; } else { bd = INFINITY; bi = -1; }
        idx[(size_t)q * K + o] = bi;
        d2[(size_t)q * K + o] = bd;
    }
}

__global__ __launch_bounds__(256) void k_knn_weights(int N, int K, const int* __restrict__ idx, const float* __restrict__ d2,
                                                     const float* __restrict__ mesh_d2, int use_sqrt, float low, float high,
                                                     float* __restrict__ knn_w, float* __restrict__ update_w) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float sum = 0.f;
    for (int k = 0; k < K; k++) {
        const int id = idx[(size_t)n * K + k];
        float md = (id >= 0 && id < N) ? mesh_d2[id] : NAN;
        float kd = d2[(size_t)n * K + k];
        if (use_sqrt) { md = sqrtf(md); kd = sqrtf(kd); }
        const float raw = 1.0f / (md * kd);
        knn_w[(size_t)n * K + k] = raw;
        sum = k == 0 ? raw : sum + raw;
    }
    for (int k = 0; k < K; k++) knn_w[(size_t)n * K + k] = knn_w[(size_t)n * K + k] / sum;
    float m = mesh_d2[n];
    if (use_sqrt) m = sqrtf(m);
    float u = m;
    if (m <= low) u = 0.f;
    if (m >= high) u = 1.f;
    if (m > low && m < high) u = (m - low) / (high - low);
    update_w[n] = u;
}

__global__ __launch_bounds__(256) void k_copy_f32(size_t total, const float* __restrict__ src, float* __restrict__ dst) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) dst[e] = src[e];
}

__global__ __launch_bounds__(64 * kSmoothWaves) void k_smooth(int N, int J, int K, const int* __restrict__ idx, const float* __restrict__ knn_w,
                                                              const float* __restrict__ update_w, const float* __restrict__ src,
                                                              float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int n = __builtin_amdgcn_readfirstlane(blockIdx.x * kSmoothWaves + (threadIdx.x >> 6));
    if (n >= N) return;
    const float u = update_w[n];
    const float* own = src + (size_t)n * J;
    float* o = dst + (size_t)n * J;
    if (u == 0.f) {
        for (int j = lane; j < J; j += 64) o[j] = own[j];
        return;
    }
    int my_i = -1;
    float my_w = 0.f;
    if (lane < K) {
        my_i = idx[(size_t)n * K + lane];
        my_w = knn_w[(size_t)n * K + lane];
        if (my_i < 0 || my_i >= N) { my_i = -1; }
    }
    for (int j0 = 0; j0 < J; j0 += 64) {
        const int j = j0 + lane;
        const int jl = min(j, J - 1);      // lanes past the row end read its last element and write nothing
        float acc = 0.f;
#pragma unroll 6
        for (int k = 0; k < K; k++) {
            const int id = __builtin_amdgcn_readlane(my_i, k);
            const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_w), k));
            const float v = src[(size_t)(id < 0 ? n : id) * J + jl];
            acc = fmaf(w, id < 0 ? 0.f : v, acc);
        }
        if (j < J) o[j] = (1.0f - u) * own[j] + u * acc;
    }
}

size_t knn_lds_bytes(int K) { return sizeof(float4) * kKnnTile + (size_t)2 * K * kKnnLanes * 4; }

bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" {

int dwg_avinit_barycentric(int32_t N, const float* closest_point, const int32_t* closest_face, int32_t V, const float* verts, int32_t F,
                           const int32_t* faces, float* bary, int32_t* vertex_indices, int32_t* nearest_vertex, dwg_stream_t stream_) {
    if (N < 0 || V < 0 || F < 0) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (!closest_point || !closest_face || !bary || !vertex_indices || !nearest_vertex) return DWG_E_ARG;
    if ((V > 0 && !verts) || (F > 0 && !faces)) return DWG_E_ARG;
    DWG_LAUNCH("avinit_barycentric", k_barycentric, dim3(dwg_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream_, N, closest_point,
               closest_face, V, verts, F, faces, bary, vertex_indices, nearest_vertex);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_avinit_lbs_interp(int32_t N, int32_t J, int32_t V, const float* table, const int32_t* vertex_indices, const float* bary, float* out,
                          dwg_stream_t stream_) {
    if (N < 0 || J < 0 || V < 0) return DWG_E_ARG;
    if (N == 0 || J == 0) return DWG_OK;
    if (!vertex_indices || !bary || !out || (V > 0 && !table)) return DWG_E_ARG;
    const long long total = (long long)N * J;
    if ((total + 255) / 256 > 0x7fffffffLL) return DWG_E_ARG;
    DWG_LAUNCH("avinit_lbs_interp", k_lbs_interp, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, total, J, V, table,
               vertex_indices, bary, out);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_avinit_knn(int32_t Nq, const float* query, int32_t Nr, const float* ref, int32_t K, int32_t* idx, float* d2, dwg_stream_t stream_) {
    if (Nq < 0 || Nr < 0 || K < 1 || K > DWG_AVINIT_KNN_MAX_K || K > Nr) return DWG_E_ARG;
    if (Nq == 0) return DWG_OK;
    if (!query || !ref || !idx || !d2) return DWG_E_ARG;
    const size_t lds = knn_lds_bytes(K);
    static bool raised = false;
    if (!raised) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_knn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)knn_lds_bytes(DWG_AVINIT_KNN_MAX_K)) != hipSuccess) {
            (void)hipGetLastError();
            return DWG_E_LAUNCH;
        }
        raised = true;
    }
    DWG_LAUNCH("avinit_knn", k_knn, dim3(dwg_cdiv(Nq, kKnnLanes)), dim3(kKnnLanes), lds, (hipStream_t)stream_, Nq, query, Nr, ref, K, idx, d2);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_avinit_knn_weights(int32_t N, int32_t K, const int32_t* idx, const float* d2, const float* mesh_d2, int32_t use_sqrt, float low,
                           float high, float* knn_w, float* update_w, dwg_stream_t stream_) {
    if (N < 0 || K < 1 || K > DWG_AVINIT_KNN_MAX_K || !(high >= low)) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (!idx || !d2 || !mesh_d2 || !knn_w || !update_w) return DWG_E_ARG;
    DWG_LAUNCH("avinit_knn_weights", k_knn_weights, dim3(dwg_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream_, N, K, idx, d2, mesh_d2,
               use_sqrt ? 1 : 0, low, high, knn_w, update_w);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_avinit_smooth(int32_t N, int32_t J, int32_t K, const int32_t* idx, const float* knn_w, const float* update_w, const float* w_in,
                      float* w_tmp, float* w_out, int32_t iterations, dwg_stream_t stream_) {
    if (N < 0 || J < 0 || iterations < 0) return DWG_E_ARG;
    if (N == 0 || J == 0) return DWG_OK;
    if (!w_in || !w_out) return DWG_E_ARG;
    const size_t total = (size_t)N * (size_t)J, bytes = total * 4;
    if (overlap(w_in, w_out, bytes)) return DWG_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (iterations == 0) {
        if ((total + 255) / 256 > 0x7fffffffULL) return DWG_E_ARG;
        DWG_LAUNCH("avinit_copy", k_copy_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, w_in, w_out);
        DWG_RETURN_IF_LAUNCH_FAILED();
        return DWG_OK;
    }
    if (K < 1 || K > DWG_AVINIT_KNN_MAX_K || !idx || !knn_w || !update_w) return DWG_E_ARG;
    if (iterations > 1 && (!w_tmp || overlap(w_tmp, w_in, bytes) || overlap(w_tmp, w_out, bytes))) return DWG_E_ARG;
    const dim3 grid(dwg_cdiv(N, kSmoothWaves)), block(64 * kSmoothWaves);
    const float* src = w_in;
    for (int s = 0; s < iterations; s++) {
        float* dst = ((iterations - 1 - s) & 1) ? w_tmp : w_out;      // the last sweep writes w_out
        DWG_LAUNCH("avinit_smooth", k_smooth, grid, block, 0, stream, N, J, K, idx, knn_w, update_w, src, dst);
        src = dst;
    }
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
