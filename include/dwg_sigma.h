/*
 * include/dwg_sigma.h -- C-ABI of the NeRF stage's SMPL-X sigma guidance geometry (boundary B8).
 *
 * What the reference's Trainer.calc_sigma_loss computes on the host with trimesh and libigl (core/trainer.py:718-825): area-weighted
 * samples on a part of the body mesh with interpolated vertex normals, noisy copies of them along the normal, and the squared distance of
 * every noisy point to the part mesh with its closest face, from which the points off the surface (and off the wrists) are kept.
 *
 *   dwg_sigma_face_records     per part face: the face record of the closest-point test and the area (fp64)
 *   dwg_sigma_area_cdf         inclusive fp64 scan of the areas in a fixed order (one workgroup)
 *   dwg_sigma_vertex_normals   corner-angle-weighted vertex normals of the part faces, gathered over a CSR table of incident faces
 *   dwg_sigma_sample           one lane per point: face pick in the CDF, the fold, the point, its normal, the noisy point
 *   dwg_sigma_point_mesh_distance   brute-force point-to-mesh squared distance, closest face and closest point
 *   dwg_sigma_keep_mask        sqrt(d2) > thickness, optionally not closest to a wrist face, and the count of kept points
 *
 * All pointers are device pointers; buffers are caller-allocated.  Every entry point returns DWG_E_ARG before any launch on a bad
 * argument; a size of 0 launches nothing.  Face indices outside [0, V) are not read: such a face gets area 0, a zero normal and an
 * infinite distance.  No float atomics: two runs are bit-identical.
 */
#ifndef DWG_SIGMA_H
#define DWG_SIGMA_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_SIGMA_FACE_RECORD_FLOATS 16   /* v0, flag | e0 = v1 - v0, e0.e0 | e1 = v2 - v0, e1.e1 | e0.e1, 0, 0, 0 */

/* verts [V, 3] fp32, faces [F, 3] int32 -> records [F, 16] fp32 (16-byte aligned), area [F] fp64 (NULL: not written). */
int dwg_sigma_face_records(int32_t V, const float* verts, int32_t F, const int32_t* faces, float* records, double* area,
                           dwg_stream_t stream);

/* area [F] fp64 -> cdf [F] fp64, cdf[i] = area[0] + ... + area[i] in a fixed order. */
int dwg_sigma_area_cdf(int32_t F, const double* area, double* cdf, dwg_stream_t stream);

/* vf_offsets [V + 1], vf_items [vf_offsets[V]] = 3 * face + corner of the faces incident to each vertex -> vnormals [V, 3] fp32:
 * unitize(sum of corner angle * unit face normal); a vertex without incident faces (or whose sum vanishes) gets a zero normal. */
int dwg_sigma_vertex_normals(int32_t V, const float* verts, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_items,
                             float* vnormals, dwg_stream_t stream);

/* draws [N, 4] fp64 in [0, 1): face pick, r1, r2, noise.  Outputs: points [N, 3], face_index [N], point_normals [N, 3], noisy [N, 3]
 * = points + (draw3 - 0.5) * noise_range * point_normals.  F >= 1. */
int dwg_sigma_sample(int32_t N, const double* draws, int32_t V, const float* verts, int32_t F, const int32_t* faces, const double* cdf,
                     const float* vnormals, float noise_range, float* points, int32_t* face_index, float* point_normals, float* noisy,
                     dwg_stream_t stream);

/* Workspace of the distance pass: per (face slice, point) partial minima.  0 when N <= 0 or F <= 0. */
size_t dwg_sigma_distance_workspace_bytes(int32_t N, int32_t F);

/* points [N, 3] fp32 against records [F, 16] -> sqr_dist [N], closest_face [N] (-1 when no face is valid), closest_point [N, 3]
 * (NULL: not written).  Ties: the lowest face index among minima equal within 5e-7 (1 + |d|) in distance.  workspace:
 * dwg_sigma_distance_workspace_bytes(N, F) bytes, 16-byte aligned. */
int dwg_sigma_point_mesh_distance(int32_t N, const float* points, int32_t F, const float* records, float* sqr_dist, int32_t* closest_face,
                                  float* closest_point, void* workspace, size_t workspace_bytes, dwg_stream_t stream);

/* keep[i] = 1.f when sqrt(sqr_dist[i]) > thickness and (wrist == NULL or wrist[closest_face[i]] == 0), else 0.f; kept[0] = count of
 * kept points (N == 0: nothing is written).  wrist [F] bytes. */
int dwg_sigma_keep_mask(int32_t N, const float* sqr_dist, const int32_t* closest_face, float thickness, int32_t F, const uint8_t* wrist,
                        float* keep, int32_t* kept, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
