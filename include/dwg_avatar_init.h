/*
 * include/dwg_avatar_init.h -- C-ABI of the avatar constructor's geometry (boundary B11): what the reference's DreamWaltzG.__init__ does on
 * the host with libigl, pytorch3d and a torch loop between the NeRF stage's point cloud and the first 3D-Gaussian step
 * (core/system/avatar.py:766-806, 865-911).
 *
 *   dwg_avinit_barycentric   barycentric coordinates of each closest point in its closest face, the face's vertex ids, the nearest vertex
 *   dwg_avinit_lbs_interp    barycentric interpolation of a per-vertex table (the LBS weights) at every point
 *   dwg_avinit_knn           exact K nearest reference points of every query (brute force, K-list in LDS, O(Nq K) memory)
 *   dwg_avinit_knn_weights   the smoothing's neighbour weights and per-point update weight
 *   dwg_avinit_smooth        `iterations` Jacobi sweeps of the neighbour average, one launch per sweep
 *
 * All pointers are device pointers; buffers are caller-allocated.  Every entry point returns DWG_E_ARG before any launch on a bad
 * argument; a size of 0 launches nothing.  Indices outside their table are not read (each entry point says what is written instead).
 * No float atomics: two runs are bit-identical.
 */
#ifndef DWG_AVATAR_INIT_H
#define DWG_AVATAR_INIT_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_AVINIT_KNN_MAX_K 64

/* closest_point [N, 3] fp32 and closest_face [N] int32 (dwg_sigma_point_mesh_distance's outputs) on the mesh verts [V, 3] fp32, faces
 * [F, 3] int32 -> bary [N, 3] fp32, vertex_indices [N, 3] int32, nearest_vertex [N] int32.
 * bary: with e0 = v1 - v0, e1 = v2 - v0, r = p - v0 evaluated in fp64, b1 = (e1.e1 e0.r - e0.e1 e1.r) / den, b2 = (e0.e0 e1.r - e0.e1 e0.r)
 * / den, den = e0.e0 e1.e1 - (e0.e1)^2, b0 = 1 - b1 - b2, rounded to fp32 (a zero-area face divides by zero as the formula reads).
 * vertex_indices: the face's three vertex ids.  nearest_vertex: vertex_indices[argmin bary], the first minimum winning.
 * A closest_face outside [0, F), or a face with a vertex id outside [0, V), writes zeros to bary and -1 to both index outputs. */
int dwg_avinit_barycentric(int32_t N, const float* closest_point, const int32_t* closest_face, int32_t V, const float* verts, int32_t F,
                           const int32_t* faces, float* bary, int32_t* vertex_indices, int32_t* nearest_vertex, dwg_stream_t stream);

/* table [V, J] fp32, vertex_indices [N, 3] int32, bary [N, 3] fp32 -> out [N, J] fp32,
 * out[n, j] = ((table[i0, j] b0) + table[i1, j] b1) + table[i2, j] b2.  A vertex id outside [0, V) contributes nothing. */
int dwg_avinit_lbs_interp(int32_t N, int32_t J, int32_t V, const float* table, const int32_t* vertex_indices, const float* bary, float* out,
                          dwg_stream_t stream);

/* query [Nq, 3], ref [Nr, 3] fp32 -> idx [Nq, K] int32, d2 [Nq, K] fp32: the K reference points nearest to each query, sorted by
 * (squared distance ascending, reference index ascending); that order also decides which of several equally distant points are kept.
 * Squared distance: fma(dz, dz, fma(dy, dy, dx dx)) in fp32 with d = ref - query.  1 <= K <= DWG_AVINIT_KNN_MAX_K and K <= Nr, otherwise
 * DWG_E_ARG.  A reference point whose distance is NaN or +inf is never selected; a row that runs out of candidates that way is padded
 * with (idx -1, d2 +inf).  No workspace: the running lists live in LDS. */
int dwg_avinit_knn(int32_t Nq, const float* query, int32_t Nr, const float* ref, int32_t K, int32_t* idx, float* d2, dwg_stream_t stream);

/* idx, d2 [N, K] (a point's neighbours and their squared distances), mesh_d2 [N] (squared distance of every point to the body mesh) ->
 * knn_w [N, K], update_w [N].  With s(x) = sqrt(x) when use_sqrt, else x:
 *   raw[k]   = 1 / (s(mesh_d2[idx[k]]) * s(d2[k]));   knn_w[k] = raw[k] / (raw[0] + raw[1] + ... in k order)
 *   update_w = m = s(mesh_d2[n]);  0 where m <= low;  1 where m >= high (this wins when low == high == m);  (m - low) / (high - low) between
 * IEEE arithmetic as the statements read: a neighbour that lies exactly on the mesh (or coincides with the point) gives raw = inf and a
 * row of NaN, as the reference's statements do.  An idx outside [0, N) reads a NaN mesh distance.  high >= low, otherwise DWG_E_ARG. */
int dwg_avinit_knn_weights(int32_t N, int32_t K, const int32_t* idx, const float* d2, const float* mesh_d2, int32_t use_sqrt, float low,
                           float high, float* knn_w, float* update_w, dwg_stream_t stream);

/* `iterations` Jacobi sweeps  w'[n, :] = (1 - u[n]) w[n, :] + u[n] sum_k knn_w[n, k] w[idx[n, k], :]  (k ascending, fma accumulation from
 * 0), every sweep reading the previous sweep's buffer only: one launch per sweep, ping-pong between w_tmp and w_out so that the result
 * lands in w_out whatever the parity.  iterations == 0 copies w_in to w_out.  w_in is never written.  Rows with u == 0 are copied
 * bit for bit without reading their neighbours.  An idx outside [0, N) contributes nothing.  w_in, w_tmp, w_out [N, J] must not overlap;
 * w_tmp may be NULL when iterations <= 1.  1 <= K <= DWG_AVINIT_KNN_MAX_K, J >= 1 (when N > 0). */
int dwg_avinit_smooth(int32_t N, int32_t J, int32_t K, const int32_t* idx, const float* knn_w, const float* update_w, const float* w_in,
                      float* w_tmp, float* w_out, int32_t iterations, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
