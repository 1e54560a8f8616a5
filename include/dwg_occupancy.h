/*
 * include/dwg_occupancy.h -- C-ABI of the NeRF stage's occupancy-grid update (boundary B13): what the reference's
 * _NeRFRenderer.update_extra_state (core/nerf/nerf_renderer.py:95-153) does between the field and the grid the marcher reads
 * (dwg_raymarch.h).
 *
 *   dwg_occ_lattice_sigma     density of the fused field (dwg_nerf.h) at the jittered point of every cell of every cascade, stored at the
 *                             cell's Morton index (:106-135)
 *   dwg_occ_lattice_points    the same points, materialised in meshgrid order
 *   dwg_occ_update            the decayed maximum, its statistics, the threshold and the bitfield (:137-147) without a host round trip
 *   dwg_raymarch_packbits_dev (dwg_raymarch.h) the last stage of dwg_occ_update on its own
 *
 * THE CELL POINT.  Cell (ix, iy, iz) of cascade c has the meshgrid index n = (ix H + iy) H + iz and the point, per component i and in
 * fp32 with every product and every sum rounded once (no fused multiply-add),
 *       axis[i] * scale[c] + (noise[c, n, k] * 2 - 1) * half[c]
 * axis [H], scale [C] and half [C] are the caller's tables: the entry points derive no formula of their own, because the rounding of
 * 2 i / (H - 1) - 1 depends on where the caller's framework evaluates it.  noise [C, H^3, 3] are uniform draws in [0, 1).
 *
 * Limits: H a power of two, 4 <= H <= 1024, 1 <= C <= 8, C H^3 < 2^32.  All pointers are device pointers; buffers are caller-allocated.
 * Every entry point returns DWG_E_ARG before any launch on a bad argument.  No atomics: two runs on the same inputs are bit-identical.
 */
#ifndef DWG_OCCUPANCY_H
#define DWG_OCCUPANCY_H
#include "dwg_nerf.h"
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

/* tmp_grid [C, H^3] fp32 <- the density of desc's field at the cell point of every cell, at tmp_grid[c, morton3d(ix, iy, iz)].  From the
 * staged point on the arithmetic is dwg_nerf_field_forward's, in both precisions (bit-identical to that entry point on the points of
 * dwg_occ_lattice_points).  random_sigmas != 0 adds 1.0f * expf(-((x^2 + z^2) + y^2) * (1 / 0.08f)) of the cell point: the reference's
 * blob 1.0 * exp(-(x ** 2).sum(-1) / (2 * 0.2 ** 2)) with the summation order and the rounding of the division that torch uses on the
 * device.  desc->raw must be 0. */
int dwg_occ_lattice_sigma(const dwg_nerf_field_desc* desc, const float* axis /*[H]*/, const float* noise /*[C,H^3,3]*/,
                          const float* scale /*[C]*/, const float* half /*[C]*/, uint32_t C, uint32_t H, uint32_t random_sigmas,
                          float* tmp_grid /*[C,H^3]*/, dwg_stream_t stream);

/* points_out [C, H^3, 3] fp32 <- the cell points in meshgrid order, by the device function dwg_occ_lattice_sigma stages them with */
int dwg_occ_lattice_points(const float* axis, const float* noise, const float* scale, const float* half, uint32_t C, uint32_t H,
                           float* points_out, dwg_stream_t stream);

/* bytes of dwg_occ_update's workspace (per-workgroup partials); 0 outside the limits */
size_t dwg_occ_update_workspace_bytes(uint32_t C, uint32_t H);

/* Three launches on `stream`:
 *   1. every cell with density_grid >= 0 (a NaN cell is not) becomes max(density_grid * decay, tmp_grid), NaN if either operand is NaN
 *      (torch.maximum); the other cells are left as they are.  Per-workgroup partials of the updated valid cells go to `workspace`:
 *      count, fp64 sum, min, max, NaN seen -- accumulated per lane, then per wave, then per workgroup, always in the same order.
 *   2. one workgroup sums the partials in workgroup order and writes
 *        stats [8] fp32 = { mean (the fp64 sum over the count, rounded to fp32 once; NaN for a count of 0), min, max (NaN if any valid
 *                           cell is NaN; +inf / -inf for a count of 0), clamp(log(min), -15, 15), clamp(log(max), -15, 15) (NaN stays),
 *                           thresh = density_thresh < mean ? density_thresh : mean (Python's min(mean, density_thresh): a NaN mean
 *                           gives NaN), and the valid count as two uint32 bit patterns, low word then high word }
 *   3. bitfield [C H^3 / 8] <- bit i of byte j = density_grid[8 j + i] > thresh (dwg_raymarch_packbits' rule; a NaN threshold sets no bit)
 * density_grid and tmp_grid [C, H^3] fp32, 16-byte aligned; workspace 16-byte aligned, dwg_occ_update_workspace_bytes(C, H) bytes
 * (DWG_E_CAPACITY when smaller). */
int dwg_occ_update(float* density_grid, const float* tmp_grid, uint32_t C, uint32_t H, float decay, float density_thresh,
                   uint8_t* bitfield, float* stats /*[8]*/, void* workspace, size_t workspace_bytes, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
