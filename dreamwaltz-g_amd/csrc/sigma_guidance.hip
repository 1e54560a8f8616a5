// sigma_guidance.hip -- the geometry of the NeRF stage's SMPL-X sigma guidance (include/dwg_sigma.h, boundary B8): part-mesh
// preparation, area-weighted surface samples, brute-force point-to-mesh distance and the keep mask.
//
// Sizes: F <= ~21 k part faces, N <= ~21 k points.  The preparation and the sampling are one lane per face / vertex / point in fp64
// (a few microseconds of work); the distance pass is the only real cost: N x F point-triangle tests in fp32, split over a grid of
// (256-point tile x face slice) so that N = 5 000 points still fill the chip.  Each slice stages its face records in LDS (all lanes read
// the same record: a broadcast) and writes a per-point partial (d2, face); a second pass reduces the partials in slice order and
// recomputes the closest point of the winning face.  No atomics anywhere: the result does not depend on scheduling.
#include "dwg_common.h"
#include "dwg_prof_internal.h"
#include "../../include/dwg_sigma.h"

#include <math.h>

namespace {

constexpr int kRec = DWG_SIGMA_FACE_RECORD_FLOATS;
constexpr int kTile = 256;                 // points per distance workgroup, one per lane
constexpr int kStage = 256;                // face records staged in LDS per round (16 KB)
constexpr int kTargetGroups = 2048;        // distance workgroups to aim for (256 CUs x 8)
constexpr int kMinSliceFaces = 64;
constexpr float kTieAbs = 5e-7f;           // tie rule: a later face wins only when closer by more than kTieAbs + kTieRel * d
constexpr float kTieRel = 5e-7f;
constexpr float kFlagDegenerate = 1.f;     // record[3]: 0 regular, 1 collinear / zero-area (distance to its segments), 2 invalid
constexpr float kFlagInvalid = 2.f;

__device__ __forceinline__ bool face_ok(const int* t, int V) {
    return t[0] >= 0 && t[0] < V && t[1] >= 0 && t[1] < V && t[2] >= 0 && t[2] < V;
}

__device__ __forceinline__ void load3d(const float* p, double o[3]) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }

__global__ __launch_bounds__(256) void k_face_records(int V, const float* __restrict__ verts, int F, const int* __restrict__ faces,
                                                      float* __restrict__ rec, double* __restrict__ area) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int* t = faces + 3 * (size_t)f;
    float r[kRec];
#pragma unroll
    for (int k = 0; k < kRec; k++) r[k] = 0.f;
    double A = 0.0;
    if (!face_ok(t, V)) {
        r[3] = kFlagInvalid;
    } else {
        double a[3], b[3], c[3];
        load3d(verts + 3 * (size_t)t[0], a); load3d(verts + 3 * (size_t)t[1], b); load3d(verts + 3 * (size_t)t[2], c);
        const double e0[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e1[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
        const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        A = 0.5 * sqrt(nn);
        const double aa = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2], bb = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
        const double ab = e0[0] * e1[0] + e0[1] * e1[1] + e0[2] * e1[2];
        // collinear within sin^2 <= 1e-14 (or a zero edge): the face is its three segments
        r[3] = (nn <= 1e-14 * aa * bb) ? kFlagDegenerate : 0.f;
        for (int k = 0; k < 3; k++) {
            r[k] = (float)a[k];
            r[4 + k] = (float)e0[k];
            r[8 + k] = (float)e1[k];
        }
        r[7] = (float)aa; r[11] = (float)bb; r[12] = (float)ab;
    }
    float4* o = reinterpret_cast<float4*>(rec + (size_t)kRec * f);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    if (area) area[f] = A;
}

// One workgroup: each thread sums a contiguous chunk, a Hillis-Steele scan of the chunk sums, then each thread writes its chunk.
__global__ __launch_bounds__(1024) void k_area_cdf(int F, const double* __restrict__ area, double* __restrict__ cdf) {
    __shared__ double s[1024];
    const int tid = threadIdx.x, chunk = (F + 1023) / 1024;
    const int lo = min(F, tid * chunk), hi = min(F, lo + chunk);
    double sum = 0.0;
    for (int i = lo; i < hi; i++) sum += area[i];
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const double add = tid >= off ? s[tid - off] : 0.0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    double run = tid > 0 ? s[tid - 1] : 0.0;
    for (int i = lo; i < hi; i++) {
        run += area[i];
        cdf[i] = run;
    }
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ void unitize3(double v[3]) {
    const double n = sqrt(dot3(v, v));
    const double s = n > 1e-12 ? 1.0 / n : 0.0;
    v[0] *= s; v[1] *= s; v[2] *= s;
}

__global__ __launch_bounds__(256) void k_vertex_normals_angle(int V, const float* __restrict__ verts, const int* __restrict__ faces,
                                                              const int* __restrict__ vf_off, const int* __restrict__ vf_items,
                                                              float* __restrict__ vn) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int e = vf_off[v]; e < vf_off[v + 1]; e++) {
        const int item = vf_items[e], f = item / 3, c = item - 3 * f;
        const int* t = faces + 3 * (size_t)f;
        if (!face_ok(t, V)) continue;
        double p[3][3];
        for (int k = 0; k < 3; k++) load3d(verts + 3 * (size_t)t[k], p[k]);
        double e0[3], e1[3], u[3], w[3];
        for (int k = 0; k < 3; k++) {
            e0[k] = p[1][k] - p[0][k]; e1[k] = p[2][k] - p[0][k];
            u[k] = p[(c + 1) % 3][k] - p[c][k]; w[k] = p[(c + 2) % 3][k] - p[c][k];
        }
        double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
        unitize3(n); unitize3(u); unitize3(w);
        const double ang = acos(fmin(1.0, fmax(-1.0, dot3(u, w))));
        for (int k = 0; k < 3; k++) acc[k] += ang * n[k];
    }
    unitize3(acc);
    vn[3 * (size_t)v] = (float)acc[0]; vn[3 * (size_t)v + 1] = (float)acc[1]; vn[3 * (size_t)v + 2] = (float)acc[2];
}

__global__ __launch_bounds__(256) void k_sample(int N, const double* __restrict__ draws, int V, const float* __restrict__ verts, int F,
                                                const int* __restrict__ faces, const double* __restrict__ cdf, const float* __restrict__ vn,
                                                float noise_range, float* __restrict__ points, int* __restrict__ fidx,
                                                float* __restrict__ pnormals, float* __restrict__ noisy) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double u0 = draws[4 * (size_t)i], u3 = draws[4 * (size_t)i + 3];
    double r1 = draws[4 * (size_t)i + 1], r2 = draws[4 * (size_t)i + 2];
    // numpy's searchsorted(cdf, u0 * total, side='left'): the first face whose cumulative area reaches the pick
    const double x = u0 * cdf[F - 1];
    int lo = 0, hi = F - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] < x) lo = mid + 1; else hi = mid;
    }
    const int f = lo;
    if (r1 + r2 > 1.0) { r1 = fabs(r1 - 1.0); r2 = fabs(r2 - 1.0); }
    const int* t = faces + 3 * (size_t)f;
    double p[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
    if (face_ok(t, V)) {
        double a[3], b[3], c[3], na[3], nb[3], nc[3];
        load3d(verts + 3 * (size_t)t[0], a); load3d(verts + 3 * (size_t)t[1], b); load3d(verts + 3 * (size_t)t[2], c);
        load3d(vn + 3 * (size_t)t[0], na); load3d(vn + 3 * (size_t)t[1], nb); load3d(vn + 3 * (size_t)t[2], nc);
        const double l0 = 1.0 - r1 - r2;
        for (int k = 0; k < 3; k++) {
            p[k] = (r1 * (b[k] - a[k]) + r2 * (c[k] - a[k])) + a[k];
            n[k] = l0 * na[k] + r1 * nb[k] + r2 * nc[k];
        }
        unitize3(n);
    }
    const double s = (u3 - 0.5) * (double)noise_range;
    for (int k = 0; k < 3; k++) {
        points[3 * (size_t)i + k] = (float)p[k];
        pnormals[3 * (size_t)i + k] = (float)n[k];
        noisy[3 * (size_t)i + k] = (float)(p[k] + s * n[k]);
    }
    fidx[i] = f;
}

// ---- point-triangle closest point (Ericson, Real-Time Collision Detection 5.1.5), relative to v0 ------------------------------------
struct FaceRec {
    float4 q0, q1, q2, q3;     // (v0, flag), (e0, e0.e0), (e1, e1.e1), (e0.e1, -, -, -)
};

// parameter t of the closest point of segment o + t d to p (o, p relative to anything common)
__device__ __forceinline__ float seg_t(float px, float py, float pz, float dx, float dy, float dz) {
    const float dd = dx * dx + dy * dy + dz * dz;
    const float t = dd > 0.f ? (px * dx + py * dy + pz * dz) / dd : 0.f;
    return fminf(1.f, fmaxf(0.f, t));
}

// closest point of the face to ap = p - v0, as v0 + v e0 + w e1
__device__ __forceinline__ void closest_vw(const FaceRec& r, float apx, float apy, float apz, float& v, float& w) {
    const float e0x = r.q1.x, e0y = r.q1.y, e0z = r.q1.z, e1x = r.q2.x, e1y = r.q2.y, e1z = r.q2.z;
    if (r.q0.w != 0.f) {
        // degenerate: the nearest of the three segments (wave-uniform branch: every lane tests the same face)
        const float tab = seg_t(apx, apy, apz, e0x, e0y, e0z);
        const float tac = seg_t(apx, apy, apz, e1x, e1y, e1z);
        const float bcx = e1x - e0x, bcy = e1y - e0y, bcz = e1z - e0z;
        const float tbc = seg_t(apx - e0x, apy - e0y, apz - e0z, bcx, bcy, bcz);
        float dx = apx - tab * e0x, dy = apy - tab * e0y, dz = apz - tab * e0z;
        float best = dx * dx + dy * dy + dz * dz;
        v = tab; w = 0.f;
        dx = apx - tac * e1x; dy = apy - tac * e1y; dz = apz - tac * e1z;
        float d = dx * dx + dy * dy + dz * dz;
        if (d < best) { best = d; v = 0.f; w = tac; }
        dx = apx - e0x - tbc * bcx; dy = apy - e0y - tbc * bcy; dz = apz - e0z - tbc * bcz;
        d = dx * dx + dy * dy + dz * dz;
        if (d < best) { v = 1.f - tbc; w = tbc; }
        return;
    }
    const float aa = r.q1.w, bb = r.q2.w, ab = r.q3.x;
    const float d1 = e0x * apx + e0y * apy + e0z * apz;
    const float d2 = e1x * apx + e1y * apy + e1z * apz;
    const float d3 = d1 - aa, d4 = d2 - ab;        // e0 . (p - v1), e1 . (p - v1)
    const float d5 = d1 - ab, d6 = d2 - bb;        // e0 . (p - v2), e1 . (p - v2)
    if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; return; }
    if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; return; }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { v = d1 / (d1 - d3); w = 0.f; return; }
    if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; return; }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { v = 0.f; w = d2 / (d2 - d6); return; }
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        const float t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.f - t; w = t; return;
    }
    const float den = va + vb + vc;
    if (va >= 0.f && vb >= 0.f && vc >= 0.f && den > 0.f) {
        const float inv = 1.f / den;
        v = vb * inv; w = vc * inv; return;
    }
    // rounding left no region: the nearest point of the boundary (the three edges)
    const float tab = seg_t(apx, apy, apz, e0x, e0y, e0z);
    const float tac = seg_t(apx, apy, apz, e1x, e1y, e1z);
    const float bcx = e1x - e0x, bcy = e1y - e0y, bcz = e1z - e0z;
    const float tbc = seg_t(apx - e0x, apy - e0y, apz - e0z, bcx, bcy, bcz);
    float dx = apx - tab * e0x, dy = apy - tab * e0y, dz = apz - tab * e0z;
    float best = dx * dx + dy * dy + dz * dz;
    v = tab; w = 0.f;
    dx = apx - tac * e1x; dy = apy - tac * e1y; dz = apz - tac * e1z;
    float d = dx * dx + dy * dy + dz * dz;
    if (d < best) { best = d; v = 0.f; w = tac; }
    dx = apx - e0x - tbc * bcx; dy = apy - e0y - tbc * bcy; dz = apz - e0z - tbc * bcz;
    d = dx * dx + dy * dy + dz * dz;
    if (d < best) { v = 1.f - tbc; w = tbc; }
}

// squared distance of p to the face; +inf for an invalid face
__device__ __forceinline__ float face_d2(const FaceRec& r, float px, float py, float pz, float& v, float& w) {
    v = 0.f; w = 0.f;
    if (r.q0.w == kFlagInvalid) return INFINITY;
    const float apx = px - r.q0.x, apy = py - r.q0.y, apz = pz - r.q0.z;
    closest_vw(r, apx, apy, apz, v, w);
    const float dx = apx - (v * r.q1.x + w * r.q2.x), dy = apy - (v * r.q1.y + w * r.q2.y), dz = apz - (v * r.q1.z + w * r.q2.z);
    return dx * dx + dy * dy + dz * dz;
}

// the squared distance a later face must beat to replace the current best (d2 = the best's squared distance)
__device__ __forceinline__ float beat_threshold(float d2) {
    if (!(d2 < INFINITY)) return INFINITY;
    const float t = sqrtf(d2) * (1.f - kTieRel) - kTieAbs;
    return t > 0.f ? t * t : -1.f;
}

__device__ __forceinline__ FaceRec load_rec(const float* rec, int f) {
    const float4* q = reinterpret_cast<const float4*>(rec + (size_t)kRec * f);
    FaceRec r;
    r.q0 = q[0]; r.q1 = q[1]; r.q2 = q[2]; r.q3 = q[3];
    return r;
}

__global__ __launch_bounds__(kTile) void k_distance_partial(int N, const float* __restrict__ P, int F, const float* __restrict__ rec,
                                                            int slice_faces, float* __restrict__ part_d2, int* __restrict__ part_f) {
    __shared__ float4 s_rec[kStage * 4];
    const int i = blockIdx.x * kTile + threadIdx.x, slice = blockIdx.y;
    const bool live = i < N;
    const float px = live ? P[3 * (size_t)i] : 0.f, py = live ? P[3 * (size_t)i + 1] : 0.f, pz = live ? P[3 * (size_t)i + 2] : 0.f;
    const int f0 = slice * slice_faces, f1 = min(F, f0 + slice_faces);
    float best = INFINITY, thr = INFINITY;
    int bf = -1;
    for (int c = f0; c < f1; c += kStage) {
        const int cnt = min(kStage, f1 - c);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const float4* q = reinterpret_cast<const float4*>(rec + (size_t)kRec * (c + threadIdx.x));
#pragma unroll
            for (int k = 0; k < 4; k++) s_rec[4 * threadIdx.x + k] = q[k];
        }
        __syncthreads();
        for (int k = 0; k < cnt; k++) {
            FaceRec r;
            r.q0 = s_rec[4 * k]; r.q1 = s_rec[4 * k + 1]; r.q2 = s_rec[4 * k + 2]; r.q3 = s_rec[4 * k + 3];
            float v, w;
            const float d2 = face_d2(r, px, py, pz, v, w);
            if (d2 < thr) { best = d2; bf = c + k; thr = beat_threshold(d2); }
        }
    }
    if (live) {
        part_d2[(size_t)slice * N + i] = best;
        part_f[(size_t)slice * N + i] = bf;
    }
}

__global__ __launch_bounds__(256) void k_distance_finish(int N, const float* __restrict__ P, int F, const float* __restrict__ rec, int slices,
                                                         const float* __restrict__ part_d2, const int* __restrict__ part_f,
                                                         float* __restrict__ sqr_dist, int* __restrict__ closest_face,
                                                         float* __restrict__ closest_point) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float best = INFINITY, thr = INFINITY;
    int bf = -1;
    for (int s = 0; s < slices; s++) {
        const float d2 = part_d2[(size_t)s * N + i];
        if (d2 < thr) { best = d2; bf = part_f[(size_t)s * N + i]; thr = beat_threshold(d2); }
    }
    sqr_dist[i] = best;
    closest_face[i] = bf;
    if (closest_point) {
        float c[3] = {NAN, NAN, NAN};
        if (bf >= 0 && bf < F) {
            const FaceRec r = load_rec(rec, bf);
            float v, w;
            face_d2(r, P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], v, w);
            c[0] = r.q0.x + (v * r.q1.x + w * r.q2.x);
            c[1] = r.q0.y + (v * r.q1.y + w * r.q2.y);
            c[2] = r.q0.z + (v * r.q1.z + w * r.q2.z);
        }
        for (int k = 0; k < 3; k++) closest_point[3 * (size_t)i + k] = c[k];
    }
}

__global__ __launch_bounds__(1024) void k_keep_mask(int N, const float* __restrict__ d2, const int* __restrict__ cf, float thickness, int F,
                                                    const unsigned char* __restrict__ wrist, float* __restrict__ keep, int* __restrict__ kept) {
    __shared__ int s[1024];
    int cnt = 0;
    for (int i = threadIdx.x; i < N; i += 1024) {
        const int f = cf[i];
        bool k = sqrtf(d2[i]) > thickness;
        if (wrist && f >= 0 && f < F && wrist[f]) k = false;
        keep[i] = k ? 1.f : 0.f;
        cnt += k ? 1 : 0;
    }
    s[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) kept[0] = s[0];
}

// distance grid: 256-point tiles x face slices, ~kTargetGroups workgroups in all, at least kMinSliceFaces faces per slice
void distance_grid(int N, int F, int& tiles, int& slices, int& slice_faces) {
    tiles = dwg_cdiv(N, kTile);
    const int max_slices = dwg_cdiv(F, kMinSliceFaces);
    slices = min(max_slices, max(1, dwg_cdiv(kTargetGroups, tiles)));
    slice_faces = dwg_cdiv(F, slices);
    slices = dwg_cdiv(F, slice_faces);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int dwg_sigma_face_records(int32_t V, const float* verts, int32_t F, const int32_t* faces, float* records, double* area,
                           dwg_stream_t stream_) {
    if (V < 0 || F < 0) return DWG_E_ARG;
    if (F == 0) return DWG_OK;
    if (!verts || !faces || !records || !aligned16(records)) return DWG_E_ARG;
    DWG_LAUNCH("sigma_face_records", k_face_records, dim3(dwg_cdiv(F, 256)), dim3(256), 0, (hipStream_t)stream_, V, verts, F, faces,
               records, area);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_sigma_area_cdf(int32_t F, const double* area, double* cdf, dwg_stream_t stream_) {
    if (F < 0) return DWG_E_ARG;
    if (F == 0) return DWG_OK;
    if (!area || !cdf) return DWG_E_ARG;
    DWG_LAUNCH("sigma_area_cdf", k_area_cdf, dim3(1), dim3(1024), 0, (hipStream_t)stream_, F, area, cdf);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_sigma_vertex_normals(int32_t V, const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_items,
                             float* vnormals, dwg_stream_t stream_) {
    if (V < 0) return DWG_E_ARG;
    if (V == 0) return DWG_OK;
    if (!verts || !faces || !vf_offsets || !vf_items || !vnormals) return DWG_E_ARG;
    DWG_LAUNCH("sigma_vertex_normals", k_vertex_normals_angle, dim3(dwg_cdiv(V, 256)), dim3(256), 0, (hipStream_t)stream_, V, verts, faces,
               vf_offsets, vf_items, vnormals);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_sigma_sample(int32_t N, const double* draws, int32_t V, const float* verts, int32_t F, const int32_t* faces, const double* cdf,
                     const float* vnormals, float noise_range, float* points, int32_t* face_index, float* point_normals, float* noisy,
                     dwg_stream_t stream_) {
    if (N < 0 || V < 0 || F < 0) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (F == 0 || !draws || !verts || !faces || !cdf || !vnormals || !points || !face_index || !point_normals || !noisy) return DWG_E_ARG;
    if (!(noise_range == noise_range)) return DWG_E_ARG;
    DWG_LAUNCH("sigma_sample", k_sample, dim3(dwg_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream_, N, draws, V, verts, F, faces, cdf,
               vnormals, noise_range, points, face_index, point_normals, noisy);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

size_t dwg_sigma_distance_workspace_bytes(int32_t N, int32_t F) {
    if (N <= 0 || F <= 0) return 0;
    int tiles, slices, slice_faces;
    distance_grid(N, F, tiles, slices, slice_faces);
    return 2 * dwg_align_up((size_t)slices * (size_t)N * 4, 256);
}

int dwg_sigma_point_mesh_distance(int32_t N, const float* points, int32_t F, const float* records, float* sqr_dist, int32_t* closest_face,
                                  float* closest_point, void* workspace, size_t workspace_bytes, dwg_stream_t stream_) {
    if (N < 0 || F < 0) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (F == 0 || !points || !records || !aligned16(records) || !sqr_dist || !closest_face) return DWG_E_ARG;
    if (!workspace || !aligned16(workspace) || workspace_bytes < dwg_sigma_distance_workspace_bytes(N, F)) return DWG_E_ARG;
    int tiles, slices, slice_faces;
    distance_grid(N, F, tiles, slices, slice_faces);
    float* part_d2 = (float*)workspace;
    int* part_f = (int*)((char*)workspace + dwg_align_up((size_t)slices * (size_t)N * 4, 256));
    hipStream_t stream = (hipStream_t)stream_;
    DWG_LAUNCH("sigma_distance_partial", k_distance_partial, dim3(tiles, slices), dim3(kTile), 0, stream, N, points, F, records,
               slice_faces, part_d2, part_f);
    DWG_LAUNCH("sigma_distance_finish", k_distance_finish, dim3(dwg_cdiv(N, 256)), dim3(256), 0, stream, N, points, F, records, slices,
               (const float*)part_d2, (const int*)part_f, sqr_dist, closest_face, closest_point);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

int dwg_sigma_keep_mask(int32_t N, const float* sqr_dist, const int32_t* closest_face, float thickness, int32_t F, const uint8_t* wrist,
                        float* keep, int32_t* kept, dwg_stream_t stream_) {
    if (N < 0 || F < 0) return DWG_E_ARG;
    if (N == 0) return DWG_OK;
    if (!sqr_dist || !closest_face || !keep || !kept || !(thickness == thickness)) return DWG_E_ARG;
    DWG_LAUNCH("sigma_keep_mask", k_keep_mask, dim3(1), dim3(1024), 0, (hipStream_t)stream_, N, sqr_dist, closest_face, thickness, F, wrist,
               keep, kept);
    DWG_RETURN_IF_LAUNCH_FAILED();
    return DWG_OK;
}

}  // extern "C"
