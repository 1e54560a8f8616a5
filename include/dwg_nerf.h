/*
 * include/dwg_nerf.h -- C-ABI of the fused NeRF field network of stage I (boundary B7).
 *
 * Replaces, for the grid backbone, what the reference's _NeRFNetwork.common_forward / local_geometry_forward compute through
 * PyTorch (core/nerf/nerf_model.py:268-295): the grid encoder (B2), sigma_net (nerf_model.py:12-33: Linear + ReLU, the last layer
 * without ReLU), the density activation and prior (nerf_model.py:38-53, 213-226) and the albedo postprocess (nerf_model.py:55-64).
 * One launch per tile of 64 points goes from x to (sigma, albedo); the encoding and the hidden layers stay in LDS.  The backward
 * recomputes them per tile instead of reading stored activations.
 *
 * Limits: encoder D = 3, C = 2, 1 <= L <= 32; 1 <= num_layers <= 4; hidden <= 64; 2 <= out_dim <= 16.
 * Precision 0 (f32): exact-f32 arithmetic (v_mfma_f32_16x16x4_f32).  Precision 1 (f16, the reference under autocast): the table
 * is read as fp16, the encoding, the weights and each layer's output are rounded to fp16, products accumulate in fp32 with an fp32
 * bias (v_mfma_f32_16x16x16_f16), and the density activation runs in fp32 on the fp16 pre-activation.
 * All pointers are device pointers unless marked HOST; buffers are caller-allocated.  No float atomics: two runs are bit-identical.
 */
#ifndef DWG_NERF_H
#define DWG_NERF_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_NERF_MAX_LAYERS 4

typedef struct dwg_nerf_field_desc {
    /* grid encoder (dwg_gridenc.h conventions) */
    const float* embeddings;            /* [offsets[L], 2] fp32 */
    const int32_t* offsets;             /* [L+1] */
    const int32_t* host_offsets;        /* [L+1] HOST copy of offsets (backward: table-gradient sizing) */
    uint32_t num_levels;                /* L */
    float log2_per_level_scale;         /* S */
    uint32_t base_resolution;           /* H */
    uint32_t gridtype;                  /* 0 hash, 1 tiled */
    uint32_t align_corners;
    uint32_t interp;                    /* 0 linear, 1 smoothstep */
    float bound;                        /* x in [-bound, bound] is encoded at (x + bound) / (2 bound) */
    /* sigma_net: weight[l] is nn.Linear's [out, in] row-major fp32, bias[l] [out] fp32 */
    uint32_t num_layers;
    uint32_t hidden;
    uint32_t out_dim;                   /* 4 + additional_dim_size: sigma, then out_dim - 1 albedo channels */
    const float* weight[DWG_NERF_MAX_LAYERS];
    const float* bias[DWG_NERF_MAX_LAYERS];
    /* epilogue */
    uint32_t density_activation;        /* 0 exp (trunc_exp), 1 softplus, 2 scaling: softplus(h * exp(sigma_scale) - 1) */
    uint32_t density_prior;             /* 0 none, 1 gaussian, 2 sqrt */
    uint32_t albedo_sigmoid;            /* 1: sigmoid (rgb field postprocess, also under raw for local_geometry_forward), 0: identity */
    uint32_t raw;                       /* 1: sigma is the last layer's output: no activation, no prior */
    const float* sigma_scale;           /* [1]; read by `scaling` only */
    uint32_t precision;                 /* 0 f32, 1 f16 */
} dwg_nerf_field_desc;

/* Gradients written by the backward; a NULL pointer is a gradient not asked for. */
typedef struct dwg_nerf_field_grads {
    float* embeddings;                  /* [offsets[L], 2]: ACCUMULATED into (the B2 table-gradient contract) */
    float* weight[DWG_NERF_MAX_LAYERS];
    float* bias[DWG_NERF_MAX_LAYERS];
    float* sigma_scale;                 /* [1]; `scaling` only */
    uint32_t accumulate;                /* 1: weight / bias / sigma_scale gradients are added to the buffers, 0: overwritten */
} dwg_nerf_field_grads;

/* sigma [M] fp32; albedo [M, out_dim - 1], fp32 (precision 0) or fp16 (precision 1).  M == 0 launches nothing. */
int dwg_nerf_field_forward(const dwg_nerf_field_desc* desc, const float* x /*[M,3]*/, uint64_t M, float* sigma, void* albedo,
                           dwg_stream_t stream);

/* Workspace of the backward: per-workgroup weight-gradient partials, the encoding gradient of one chunk of points and the slab-binned
 * table gradient's workspace for that chunk.  0 on a bad descriptor. */
size_t dwg_nerf_field_backward_workspace_bytes(const dwg_nerf_field_desc* desc, uint64_t M);

/* dsigma [M] fp32, dalbedo [M, out_dim - 1] in the forward's albedo dtype.  Points are processed in chunks: per chunk one launch
 * recomputes the field, adds its tiles' weight gradients into per-workgroup partials and writes d_enc [chunk, 2L] fp32, which the
 * slab-binned table gradient (dwg_grid_encode_backward_slabs, accumulate = 1) adds into grads->embeddings.  One more launch sums the
 * partials in a fixed order.  workspace: dwg_nerf_field_backward_workspace_bytes(desc, M) bytes, 256-byte aligned. */
int dwg_nerf_field_backward(const dwg_nerf_field_desc* desc, const float* x, uint64_t M, const float* dsigma, const void* dalbedo,
                            const dwg_nerf_field_grads* grads, void* workspace, size_t workspace_bytes, dwg_stream_t stream);

/* The field at x and the density at the six shifted points of the finite-difference normal (_NeRFNetwork.normal, nerf_model.py:146-159),
 * in one launch (boundary B19): per tile of 64 points seven passes of the field, at x and at (x +- epsilon e_a).clamp(-bound, bound) for
 * the shifts +x, -x, +y, -y, +z, -z, made in registers -- the shifted points never touch memory.  sigma / albedo are
 * dwg_nerf_field_forward's bit for bit; sigma_fd [M, 6] fp32, column s is dwg_nerf_field_forward's density at the points of shift s bit
 * for bit (the prior is taken at the shifted point).  desc->raw must be 0, epsilon > 0.  M == 0 launches nothing. */
int dwg_nerf_field_forward_fd(const dwg_nerf_field_desc* desc, const float* x /*[M,3]*/, uint64_t M, float epsilon, float* sigma, void* albedo,
                              float* sigma_fd, dwg_stream_t stream);

/* The backward of dwg_nerf_field_forward_fd with respect to the parameters (x is not differentiated): dsigma [M], dalbedo [M, out_dim - 1]
 * in the albedo dtype or NULL (the albedo has no gradient: no buffer of zeros is read), dsigma_fd [M, 6] fp32.  The chunk loop of
 * dwg_nerf_field_backward with seven launches per chunk, one per point set (the six shifted sets of every chunk first, in their +-
 * pairs, then the points: the opposite-signed gradients of a pair cancel before smaller terms are added); the weight-gradient partials
 * accumulate across passes and chunks and are summed once at the end, the encoding gradient of a pass goes through dwg_grid_encode_backward_slabs (accumulate = 1)
 * before the next pass reuses its buffer.  The result is what seven dwg_nerf_field_backward calls (accumulate = 1) on the shifted points
 * give, up to the order of the fp32 sums; two runs are bit-identical.  workspace: dwg_nerf_field_backward_workspace_bytes(desc, M)
 * bytes -- no more than one dwg_nerf_field_backward call takes --, 256-byte aligned. */
int dwg_nerf_field_backward_fd(const dwg_nerf_field_desc* desc, const float* x, uint64_t M, float epsilon, const float* dsigma,
                               const void* dalbedo, const float* dsigma_fd, const dwg_nerf_field_grads* grads, void* workspace,
                               size_t workspace_bytes, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
