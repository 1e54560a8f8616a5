/*
 * include/dwg_nerf_render.h -- C-ABI of the one-launch inference render of the NeRF stage (boundary B14): what the evaluation branch of
 * the reference's _NeRFRenderer.run_cuda (core/nerf/nerf_renderer.py:351-385) computes with a Python loop over march_rays, the field
 * network and composite_rays, for perturb False: dwg_nerf_render_infer for shading 'albedo', dwg_nerf_render_shaded (boundary B15) for
 * 'normal', 'textureless' and 'lambertian'.
 *
 * One persistent kernel marches every ray from near to its end (the marching rule of dwg_raymarch.h), evaluates the fused field of
 * dwg_nerf.h on the samples of 256 rays at a time (64-point tiles on the matrix cores, the layers in LDS) and composites each sample
 * with the statements of dwg_raymarch_composite_rays, in their order.  No sample position, density or colour is written to memory and
 * nothing returns to the host.  A ray's arithmetic does not depend on which workgroup or slot took it: two runs, and runs with different
 * max_workgroups, are bit-identical.  No atomics on global memory.
 *
 * A ray ends when t >= far, when the transmittance 1 - weights_sum BEFORE a sample is below T_thresh (that sample is still composited,
 * as the loop does), or after exactly max_steps composited samples.  The loop's budget counts n_step per iteration instead and lets a
 * ray alive at the end composite between max_steps and max_steps + 7 samples; rays that end by far or T_thresh are unaffected.
 *
 * Limits: those of dwg_nerf.h and of the marcher (bound > 0, max_steps >= 1, 1 <= C <= 8, 1 <= H <= 1024, C H^3 < 2^32);
 * out_dim - 1 is 3 (rgb) or 4 (latent); desc->raw must be 0.  All pointers are device pointers; buffers are caller-allocated.
 */
#ifndef DWG_NERF_RENDER_H
#define DWG_NERF_RENDER_H
#include "dwg_nerf.h"
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rays_o / rays_d [N, 3], nears / fars [N] fp32; bitfield [C H^3 / 8].  The outputs are OVERWRITTEN: a ray with near >= far, or one that
 * finds no occupied cell, gets zeros.  The albedo of a sample is rounded through the field's precision (fp16 under precision 1) before it
 * is composited in fp32, as dwg_nerf_field_forward stores it.  binarize: alpha > 0.5 ? 1 : 0.  counts may be NULL.
 * max_workgroups: the number of persistent workgroups (0: the default); workgroup w of G owns the 64-ray blocks w, w + G, ...
 * DWG_E_ARG before any device call on a bad argument; N == 0 returns DWG_OK and launches nothing. */
int dwg_nerf_render_infer(const dwg_nerf_field_desc* desc,
    const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t N,
    const uint8_t* bitfield, float bound, uint32_t contract, float dt_gamma, uint32_t max_steps,
    uint32_t C, uint32_t H, float T_thresh, uint32_t binarize,
    float* weights_sum /*[N]*/, float* depth /*[N]*/, float* image /*[N, out_dim-1]*/,
    int32_t* counts /*[N] or NULL: samples composited per ray*/,
    uint32_t max_workgroups /*0: the default*/, dwg_stream_t stream);

/* The same render with the colour of every sample shaded from the finite-difference normal of the density (boundary B15): what the loop
 * computes for shading 'normal', 'textureless' and 'lambertian' (forward() and normal(), core/nerf/nerf_model.py:74-105, 146-169).
 * Per sample the field is evaluated at seven points: the sample, and the sample with one component shifted by +epsilon or -epsilon and
 * clamped to [-desc->bound, desc->bound] (an fp32 add; NaN stays NaN).  Each shifted density takes the density prior at the shifted
 * point.  Then, in fp32 and every operation rounded on its own:
 *   g[a] = (-0.5 (s_pos[a] - s_neg[a])) / epsilon;  n = nan_to_num(g / sqrt(max(g . g, 1e-20)))   (NaN -> 0, +-inf -> +-FLT_MAX)
 *   shading 1 (normal):       rgb = (n + 1) / 2
 *   shading 2 (textureless):  lam = ambient_ratio + (1 - ambient_ratio) max(n . (-light_d), 0);  rgb = (lam, lam, lam)
 *   shading 3 (lambertian):   rgb = albedo lam, the albedo as dwg_nerf_render_infer takes it
 * With out_dim == 5 (latent) shadings 1 and 2 write a fourth channel of 0, the reference's zero pad; shading 3 is ill-formed there (five
 * channels into a four-channel image) and refused.  light_d [3] is a device pointer, read by the kernel only; it may be NULL for
 * shading 1.  weights_sum, depth and counts are those of dwg_nerf_render_infer on the same rays, bit for bit: shading touches no
 * geometry.  Everything else -- the march, the three ray-ending rules, max_workgroups, bit-identical repeat runs, no global atomics and no
 * intermediate buffer -- is as above.
 * DWG_E_ARG before any device call for a shading outside 1..3, a NULL light_d with shading 2 or 3, shading 3 with out_dim == 5, an
 * epsilon that is not positive (NaN included) and everything dwg_nerf_render_infer refuses; N == 0 returns DWG_OK and launches nothing. */
int dwg_nerf_render_shaded(const dwg_nerf_field_desc* desc,
    const float* rays_o, const float* rays_d, const float* nears, const float* fars, uint32_t N,
    const uint8_t* bitfield, float bound, uint32_t contract, float dt_gamma, uint32_t max_steps,
    uint32_t C, uint32_t H, float T_thresh, uint32_t binarize,
    uint32_t shading /*1 normal, 2 textureless, 3 lambertian*/, const float* light_d /*[3] device; may be NULL for 1*/,
    float ambient_ratio, float epsilon /*> 0; the reference's 1e-3*/,
    float* weights_sum /*[N]*/, float* depth /*[N]*/, float* image /*[N, out_dim-1]*/,
    int32_t* counts /*[N] or NULL*/, uint32_t max_workgroups /*0: the default*/, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
