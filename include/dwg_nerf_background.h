/*
 * include/dwg_nerf_background.h -- C-ABI of the learned background of stage I (boundary B22, bg_mode 'nerf').
 *
 * Replaces what the reference's _NeRFNetwork.background computes through PyTorch for the learned mode (core/nerf/nerf_model.py:134-139,
 * 248-256): the frequency encoding of the ray direction (encoder_bg, FreqEncoder(3, degree)), the small bg_net MLP (Linear + ReLU, the
 * last layer without ReLU) and the sigmoid (rgb) or identity (latent) epilogue.  One launch goes from rays_d to the [N, C] image that
 * dwg_nerf_view_compose_forward mixes as DWG_VIEW_BG_IMAGE: a workgroup takes 64 rays at a time, the encoding and the hidden layers
 * stay in LDS.  The backward recomputes them per tile from rays_d and the parameters, nothing else is saved.
 *
 * The encoding: out[c] = x[c] for c < 3; c = 3 + (2 f + s) * 3 + d holds sin(2^f x[d]) (s = 0) or cos(2^f x[d]) (s = 1), f < degree.
 * Limits: 1 <= degree <= 8 (width 3 + 6 degree <= 51); 1 <= num_layers <= 3; hidden 16, 32 or 64; out_dim 3 or 4; every layer biased;
 * N < 2^31.  Precision 0 (f32): exact-f32 arithmetic (v_mfma_f32_16x16x4_f32).  Precision 1 (f16, the reference under autocast): the
 * encoding is computed in fp32, then it, the weights and each layer's output are rounded to fp16, products accumulate in fp32 with an
 * fp32 bias (v_mfma_f32_16x16x16_f16), and the sigmoid's output is rounded to fp16; the output buffer is fp32 and holds those values.
 * All pointers are device pointers; buffers are caller-allocated.  No float atomics: two runs are bit-identical.  Every entry point
 * returns DWG_E_ARG before any launch on a bad argument.
 */
#ifndef DWG_NERF_BACKGROUND_H
#define DWG_NERF_BACKGROUND_H
#include "dwg_types.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DWG_NERF_BG_MAX_LAYERS 3
#define DWG_NERF_BG_MAX_DEGREE 8

typedef struct dwg_nerf_bg_desc {
    uint32_t degree;                    /* encoder_bg: input width of bg_net is 3 + 6 degree */
    uint32_t num_layers;
    uint32_t hidden;                    /* read when num_layers > 1 */
    uint32_t out_dim;                   /* C: 3 (rgb) or 4 (latent) */
    /* bg_net: weight[l] is nn.Linear's [out, in] row-major fp32, bias[l] [out] fp32 */
    const float* weight[DWG_NERF_BG_MAX_LAYERS];
    const float* bias[DWG_NERF_BG_MAX_LAYERS];
    uint32_t sigmoid;                   /* 1: sigmoid epilogue (rgb), 0: identity (latent) */
    uint32_t precision;                 /* 0 f32, 1 f16 */
} dwg_nerf_bg_desc;

/* Gradients written (overwritten) by the backward; a NULL pointer is a gradient not asked for. */
typedef struct dwg_nerf_bg_grads {
    float* weight[DWG_NERF_BG_MAX_LAYERS];
    float* bias[DWG_NERF_BG_MAX_LAYERS];
} dwg_nerf_bg_grads;

/* out [N, 3 + 6 degree] fp32 <- the encoding of dirs [N, 3] fp32.  N == 0 launches nothing. */
int dwg_nerf_freq_encode(uint32_t N, const float* dirs, uint32_t degree, float* out, dwg_stream_t stream);

/* out [N, out_dim] fp32 <- epilogue(bg_net(encode(dirs))).  N == 0 launches nothing. */
int dwg_nerf_bg_forward(uint32_t N, const float* dirs, const dwg_nerf_bg_desc* desc, float* out, dwg_stream_t stream);

/* Bytes of the backward's workspace: the per-workgroup weight- and bias-gradient partials.  0 on a bad descriptor. */
size_t dwg_nerf_bg_backward_workspace_bytes(const dwg_nerf_bg_desc* desc);

/* d_out [N, out_dim] fp32 (rounded to fp16 on entry under precision 1, as autograd hands the reference a half gradient).  One launch
 * recomputes the forward per tile, walks the layers backwards and leaves per-workgroup partials in the workspace; a second launch sums
 * them in workgroup order into the gradients asked for.  There is no gradient with respect to dirs.  workspace:
 * dwg_nerf_bg_backward_workspace_bytes(desc) bytes, 256-byte aligned.  With no gradient asked for, or N == 0, nothing is launched
 * (N == 0: nothing is written). */
int dwg_nerf_bg_backward(uint32_t N, const float* dirs, const float* d_out, const dwg_nerf_bg_desc* desc, const dwg_nerf_bg_grads* grads,
                         void* workspace, size_t workspace_bytes, dwg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
