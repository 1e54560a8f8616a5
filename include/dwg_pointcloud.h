/*
 * include/dwg_pointcloud.h -- C-ABI of the NeRF stage's point-cloud export (boundary B12): what the reference's export_point_cloud and
 * remove_points_inside_bboxes (core/nerf/to_point_cloud.py:27-114) do between a trained density field and the avatar constructor.
 *
 *   dwg_pc_lattice_sigma     density of the fused field (dwg_nerf.h) at every point of an nx x ny x nz lattice, in the reference's order
 *   dwg_pc_select_above      the indices i with values[i] > thresh, ascending, and their count
 *   dwg_pc_select_flags      the same over a byte mask
 *   dwg_pc_lattice_points    coordinates of lattice points given by their flat reference-order indices
 *   dwg_pc_fd_points         the six shifted, clamped point sets of the finite-difference normal (nerf_model.py:149-154)
 *   dwg_pc_finish            colours (latent_to_rgb, to_point_cloud.py:10-24) and normals (nerf_model.py:155-168) of the survivors
 *   dwg_pc_outside_boxes     keep mask of remove_points_inside_bboxes
 *
 * THE REFERENCE'S LATTICE ORDER.  Every axis is cut into chunks of `split` entries (the last one shorter).  Chunks follow each other as
 * (xi, yi, zi) with zi fastest; inside a chunk the points are row-major (ix, iy, iz) with iz fastest.  A flat index counts points in that
 * order.  split >= 1; a split beyond an axis' length means one chunk along that axis.
 *
 * All pointers are device pointers; buffers are caller-allocated.  Every entry point returns DWG_E_ARG before any launch on a bad
 * argument; a size of 0 launches nothing and succeeds.  No atomics: the order and the values of two runs are bit-identical.
 */
#ifndef DWG_POINTCLOUD_H
#define DWG_POINTCLOUD_H
#include "dwg_nerf.h"
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

/* number of (min, max) pairs dwg_pc_lattice_sigma writes */
#define DWG_PC_MINMAX_PAIRS 4096

/* sigma [nx ny nz] fp32 of desc's field at the lattice points (ax[ix], ay[iy], az[iz]), in the reference's order.  ax [nx], ay [ny],
 * az [nz] fp32 are the caller's axis tables (torch.linspace evaluated on the host); the kernel reads them and derives nothing.  The
 * arithmetic from the point on is dwg_nerf_field_forward's: sigma is bit-identical to that entry point on the materialised points, in
 * both precisions.  No albedo is written.  minmax [DWG_PC_MINMAX_PAIRS, 2] fp32 receives per-workgroup (min, max) partials of sigma
 * (unused pairs hold (+inf, -inf); NaN densities are skipped): their min / max is the density range.  desc->raw must be 0.
 * nx ny nz must be below 2^32. */
int dwg_pc_lattice_sigma(const dwg_nerf_field_desc* desc, const float* ax, const float* ay, const float* az, uint32_t nx, uint32_t ny,
                         uint32_t nz, uint32_t split, float* sigma, float* minmax, dwg_stream_t stream);

/* workspace of the two selections over M entries (one uint32 per block of the ordered write); 0 for M == 0 or M >= 2^32 */
size_t dwg_pc_select_workspace_bytes(uint64_t M);

/* idx_out <- the i in [0, M) with values[i] > thresh (strict, fp32; NaN is never selected), ascending; count_out [1] uint32 <- how many
 * there are.  At most `capacity` indices are written (the first ones); the count is the full count whatever the capacity.  M == 0 writes
 * nothing, not even the count.  M < 2^32.  workspace: dwg_pc_select_workspace_bytes(M) bytes, 4-byte aligned.  Three launches: per-block
 * counts (ballot + popcount), a scan of the block counts, the ordered write (slot = block base + wave base + lanes below in the ballot). */
int dwg_pc_select_above(uint64_t M, const float* values, float thresh, uint32_t* idx_out, uint64_t capacity, uint32_t* count_out,
                        void* workspace, size_t workspace_bytes, dwg_stream_t stream);

/* the same with flags[i] != 0 as the predicate; flags [M] uint8 */
int dwg_pc_select_flags(uint64_t M, const uint8_t* flags, uint32_t* idx_out, uint64_t capacity, uint32_t* count_out, void* workspace,
                        size_t workspace_bytes, dwg_stream_t stream);

/* points_out [n, 3] fp32 <- (ax[ix], ay[iy], az[iz]) of the flat reference-order indices idx [n] uint32, decoded by the function
 * dwg_pc_lattice_sigma uses.  An index at or beyond nx ny nz reads nothing and writes NaN. */
int dwg_pc_lattice_points(uint64_t n, const uint32_t* idx, const float* ax, const float* ay, const float* az, uint32_t nx, uint32_t ny,
                          uint32_t nz, uint32_t split, float* points_out, dwg_stream_t stream);

/* out [6, n, 3] fp32 <- clamp(points + d_s, -bound, bound) for d_s = (+eps,0,0), (-eps,0,0), (0,+eps,0), (0,-eps,0), (0,0,+eps),
 * (0,0,-eps): one fp32 add per component (the unshifted ones add +0), then the clamp on all three; NaN stays NaN.  bound >= 0. */
int dwg_pc_fd_points(uint64_t n, const float* points, float eps, float bound, float* out, dwg_stream_t stream);

/* albedo [n, C] fp32, C = 3 or 4; sig6 [6, n] fp32 (the densities at dwg_pc_fd_points' sets, same order)
 *   colors_out [n, 3]:  C == 3: albedo;  C == 4: albedo x the latent-to-RGB matrix, out_j = ((a0 m0j + a1 m1j) + a2 m2j) + a3 m3j,
 *                       every product and sum rounded to fp32 (no fused multiply-add)
 *   normals_out [n, 3]: v_a = (-0.5f (pos_a - neg_a)) / eps (IEEE division);  v / sqrt(max(v.v, 1e-20f)), v.v = (vx vx + vy vy) + vz vz
 *                       without fused multiply-adds (a NaN v.v stays NaN, as torch.clamp keeps it);  then NaN -> 0, +-inf -> +-FLT_MAX. */
int dwg_pc_finish(uint64_t n, uint32_t C, const float* albedo, const float* sig6, float eps, float* colors_out, float* normals_out,
                  dwg_stream_t stream);

/* keep [n] uint8 <- 0 where the point lies inside any box, else 1.  points [n, 3] fp32; boxes [nb, 2, 3] float64, (min corner, max
 * corner) per box.  Each coordinate is widened to double and compared inclusively (>= min and <= max on all three axes), as the
 * reference compares float64 numpy arrays.  nb == 0 keeps every point (boxes may be NULL). */
int dwg_pc_outside_boxes(uint64_t n, const float* points, uint32_t nb, const double* boxes, uint8_t* keep, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
