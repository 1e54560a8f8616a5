/*
 * include/dwg_raymarch.h -- C-ABI of the occupancy-grid ray marcher of the NeRF stage (boundary B6).
 *
 * Replaces the pybind backends `_raymarchingrgb` / `_raymarchinglatent` of the reference:
 *   prototypes  /root/reference/core/nerf/raymarching/{rgb,latent}/src/raymarching.h
 *   bindings    /root/reference/core/nerf/raymarching/{rgb,latent}/src/bindings.cpp
 *   callers     /root/reference/core/nerf/raymarching/rgb/raymarching.py
 * One entry point per backend function, in the backend's argument order.  `channels` is the colour width (3 = rgb, 4 = latent);
 * `binarize` exists only in the rgb variant (pass 0 for latent).  All buffers are fp32 / int32 / uint8 DEVICE pointers allocated by
 * the caller; every function returns DWG_OK or a DWG_E_* code and runs on `stream`.
 *
 * Differences from the reference backend, all on the caller-invisible side:
 *   - march_rays_train assigns point offsets with a device-side exclusive scan of the per-ray counts instead of atomicAdd, so the
 *     points are ray-major (rays[n,0] = counter_in + sum of the counts of rays 0..n-1) and the march is bit-reproducible.  The scan
 *     needs `workspace` (dwg_raymarch_train_workspace_bytes(N)); `M` bounds the write pass (a ray whose offset + count exceeds it is
 *     not written).
 *   - march_rays / composite_rays take the ray count `N` of rays_o / rays_t / image, and skip alive entries outside [0, N).
 */
#ifndef DWG_RAYMARCH_H
#define DWG_RAYMARCH_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

/* slab test of every ray against aabb[6] = (xmin, ymin, zmin, xmax, ymax, zmax); a miss gives near = far = FLT_MAX, near is
 * clamped up to min_near */
int dwg_raymarch_near_far_from_aabb(const float* rays_o /*[N,3]*/, const float* rays_d /*[N,3]*/, const float* aabb /*[6]*/, uint32_t N,
                                    float min_near, float* nears /*[N]*/, float* fars /*[N]*/, dwg_stream_t stream);
/* (theta, phi) in [-1, 1] of the far intersection with the sphere of `radius` (y up) */
int dwg_raymarch_sph_from_ray(const float* rays_o, const float* rays_d, float radius, uint32_t N, float* coords /*[N,2]*/,
                              dwg_stream_t stream);
int dwg_raymarch_morton3d(const int32_t* coords /*[N,3]*/, uint32_t N, int32_t* indices /*[N]*/, dwg_stream_t stream);
int dwg_raymarch_morton3d_invert(const int32_t* indices /*[N]*/, uint32_t N, int32_t* coords /*[N,3]*/, dwg_stream_t stream);
/* bit i of byte j = grid[8j + i] > density_thresh; N = C*H^3/8 bytes */
int dwg_raymarch_packbits(const float* grid /*[8N]*/, uint32_t N, float density_thresh, uint8_t* bitfield /*[N]*/, dwg_stream_t stream);
/* the same with the threshold read from device memory (density_thresh [1] fp32; NaN sets no bit): the last stage of dwg_occ_update
 * (dwg_occupancy.h), usable on its own.  grid 16-byte aligned. */
int dwg_raymarch_packbits_dev(const float* grid /*[8N]*/, uint32_t N, const float* density_thresh /*[1]*/, uint8_t* bitfield /*[N]*/,
                              dwg_stream_t stream);
/* res[rays[n,0] + i] = n for i < rays[n,1]; rays whose range leaves [0, M) are skipped */
int dwg_raymarch_flatten_rays(const int32_t* rays /*[N,2]*/, uint32_t N, uint32_t M, int32_t* res /*[M]*/, dwg_stream_t stream);

size_t dwg_raymarch_train_workspace_bytes(uint32_t N);
/* xyzs == NULL: count pass -- rays[n,1] = samples of ray n (<= max_steps), rays[n,0] = counter[0] + exclusive prefix sum of the
 * counts, counter[0] += total.  xyzs != NULL (dirs, ts too): write pass -- re-marches ray n up to rays[n,1] samples and writes them at
 * rays[n,0] (xyzs: contracted coordinates, ts[:,0] = t after the step, ts[:,1] = dt); `M` is the row count of xyzs / dirs / ts. */
int dwg_raymarch_march_rays_train(const float* rays_o, const float* rays_d, const uint8_t* grid /*[C*H^3/8]*/, float bound,
                                  uint32_t contract, float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H,
                                  const float* nears, const float* fars, float* xyzs /*[M,3] or NULL*/, float* dirs /*[M,3]*/,
                                  float* ts /*[M,2]*/, uint32_t M, int32_t* rays /*[N,2]*/, int32_t* counter /*[1]*/,
                                  const float* noises /*[N]*/, void* workspace, size_t workspace_bytes, dwg_stream_t stream);
/* weights [M] are written up to the sample where T first drops below T_thresh (the caller pre-zeroes them); weights_sum / depth
 * [N], image [N,channels] are overwritten (zero for empty rays and rays whose range exceeds M) */
int dwg_raymarch_composite_rays_train_forward(const float* sigmas /*[M]*/, const float* rgbs /*[M,channels]*/, const float* ts /*[M,2]*/,
                                              const int32_t* rays /*[N,2]*/, uint32_t M, uint32_t N, uint32_t channels, float T_thresh,
                                              uint32_t binarize, float* weights, float* weights_sum, float* depth, float* image,
                                              dwg_stream_t stream);
/* The same pass, which also reports where each ray stopped (boundary B18, dwg_nerf_train.h).  weights (when given), weights_sum, depth
 * and image are those of dwg_raymarch_composite_rays_train_forward, bit for bit; weights may be NULL.  live[n] is the number of leading
 * samples of ray n that were composited: up to and including the sample where T first drops below T_thresh, rays[n,1] for a ray that
 * never stops, 0 for an empty ray and for one whose range exceeds M.  Rows at or beyond live[n] get no weight and, in the backward, no
 * gradient. */
int dwg_raymarch_composite_rays_train_forward_live(const float* sigmas /*[M]*/, const float* rgbs /*[M,channels]*/,
                                                   const float* ts /*[M,2]*/, const int32_t* rays /*[N,2]*/, uint32_t M, uint32_t N,
                                                   uint32_t channels, float T_thresh, uint32_t binarize, float* weights /*[M] or NULL*/,
                                                   float* weights_sum, float* depth, float* image, int32_t* live /*[N]*/,
                                                   dwg_stream_t stream);
/* the reference's gradient formula (raymarching.cu:652-694); grad_sigmas / grad_rgbs are written up to the same sample as the
 * forward pass (the caller pre-zeroes them) */
int dwg_raymarch_composite_rays_train_backward(const float* grad_weights /*[M]*/, const float* grad_weights_sum /*[N]*/,
                                               const float* grad_depth /*[N]*/, const float* grad_image /*[N,channels]*/,
                                               const float* sigmas, const float* rgbs, const float* ts, const int32_t* rays,
                                               const float* weights_sum, const float* depth, const float* image, uint32_t M, uint32_t N,
                                               uint32_t channels, float T_thresh, uint32_t binarize, float* grad_sigmas,
                                               float* grad_rgbs, dwg_stream_t stream);

/* inference: n_step samples per alive ray from rays_t[rays_alive[n]], written at n*n_step (unwritten rows keep the caller's zeros) */
int dwg_raymarch_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* rays_alive, const float* rays_t, const float* rays_o,
                            const float* rays_d, float bound, uint32_t contract, float dt_gamma, uint32_t max_steps, uint32_t C,
                            uint32_t H, const uint8_t* grid, const float* nears, const float* fars, uint32_t N, float* xyzs, float* dirs,
                            float* ts, const float* noises /*[n_alive]*/, dwg_stream_t stream);
/* accumulates into weights_sum / depth / image [N,channels] in place; a terminated ray is marked -1 in rays_alive, a live one gets
 * its last t in rays_t */
int dwg_raymarch_composite_rays(uint32_t n_alive, uint32_t n_step, uint32_t channels, float T_thresh, uint32_t binarize,
                                int32_t* rays_alive, float* rays_t, const float* sigmas, const float* rgbs, const float* ts,
                                uint32_t N, float* weights_sum, float* depth, float* image, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
