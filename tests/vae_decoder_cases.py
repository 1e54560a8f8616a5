"""Shared pieces of the VAE-decoder tests (B26): the cases, the float64 oracle of AutoencoderKL.decode, the float64 statement of the
scheduler step with its per-element bound, and the inputs of the two boundary converters.  Used by test_vae_decoder_host.py (what can be
shown without a GPU: parameter counts, the clamp condition of the cases, the step formulas returning x0, the inference grid) and
test_vae_decoder_gpu.py (the kernels and plans).

The oracle is plain torch on the CPU in float64, written with the layer helpers of oracle/sd15.py.  The weights are the seeded random ones
of sd15.random_state_dict.  Random weights make conv_out arbitrary in scale, and GroupNorm removes any scale put on the latents, so the only
place where the range of the decoded image can be set is the last layer: `decoder.conv_out`'s weight and bias are multiplied by
CONV_OUT_SCALE.  The constant is chosen so that, in the float64 oracle of every case, between 10 % and 90 % of the output elements lie
strictly inside (0, 1) after x / 2 + 0.5 and both clamps occur (asserted by the host test): the clamped comparison then exercises the
linear part and both saturated parts.

Tolerances of the decoder against float64 are the ones the project already asserts for the encoder's forward pass, which is made of the same
layer kinds at the same widths: relative L2 of the raw output f32x 1e-4, f32 1e-3, f16 4e-3, bf16 3e-2 (tests/test_sd15_f32x_gpu.py,
test_sd15_fp32_gpu.py, test_sd15_fp16_gpu.py, test_guidance_gpu.py).  The clamped image is compared per element: the clamp is 1-Lipschitz,
so |got - ref| <= bar * max|raw_ref|.

The scheduler step (include/dwg_sds.h dwg_sds_ddpm_step) is compared per element in the project's form |out - ref| <= ARITH (|ref| + S),
S the same expression evaluated over absolute values (what the cancellation in x_t - sqrt(1 - a_t) eps can cost) and ARITH the fp32-grade
bar of tests/nn_norm_cases.py."""
import functools

import torch
import torch.nn.functional as F

from tests.nn_norm_cases import ARITH  # noqa: F401  (re-exported: the step's bound)

CONV_OUT_SCALE = 2.0
REL_L2_BAR = {"f32x": 1e-4, "f32": 1e-3, "f16": 4e-3, "bf16": 3e-2}
STEP_TIMESTEPS = [(981, 961), (501, 481), (21, 1), (1, -19), (0, -20)]      # (t, t_prev); the last: no noise term; (1, -19): a_p = 1, 1e-20 floor
STEP_SHAPE = (4, 9, 9)                                                       # 324 elements per view: no multiple of any block size


def main_case():
    """Four levels at reduced width, latent 16 -> 128 x 128, one image (the widths of test_guidance_gpu.py's VAE)."""
    from dreamwaltz_g_amd import sd15
    return dict(name="main", cfg=sd15.VAEConfig(block_out_channels=(32, 64, 64, 64)), latent_hw=16, batch=1, seed=31)


def two_level_case():
    """Two levels, one resnet pair per block, batch 2 with different latents per image (batch indexing)."""
    from dreamwaltz_g_amd import sd15
    return dict(name="two_level", cfg=sd15.VAEConfig(block_out_channels=(16, 32), layers_per_block=1, groups=8), latent_hw=8, batch=2, seed=32)


def state_dict(case):
    """fp32 decoder weights of a case, conv_out scaled."""
    from dreamwaltz_g_amd import sd15
    sd = sd15.random_state_dict(sd15.vae_decoder_param_shapes(case["cfg"]), seed=case["seed"])
    sd["decoder.conv_out.weight"] = sd["decoder.conv_out.weight"] * CONV_OUT_SCALE
    sd["decoder.conv_out.bias"] = sd["decoder.conv_out.bias"] * CONV_OUT_SCALE
    return sd


def latents(case):
    """[B, 4, h, h] fp32 at the scale of SD latents (unit normal times the scaling factor's inverse cancels: plain unit normal)."""
    g = torch.Generator().manual_seed(case["seed"] + 100)
    return torch.randn(case["batch"], case["cfg"].latent_channels, case["latent_hw"], case["latent_hw"], generator=g)


def decode_oracle(cfg, sd, lat):
    """AutoencoderKL.decode(1 / scaling_factor * latents) in the dtype of `lat` / `sd`: the RAW image [B, 3, H, W] (before x / 2 + 0.5 and the clamp)."""
    from oracle import sd15 as osd
    g = cfg.groups
    h = osd._conv(1 / cfg.scaling_factor * lat, sd, "post_quant_conv", padding=0)
    h = osd._conv(h, sd, "decoder.conv_in")
    h = osd.resnet(h, sd, "decoder.mid_block.resnets.0", None, g, 1e-6)
    a = "decoder.mid_block.attentions.0"
    B, C, H, W = h.shape
    n = osd._gn(h, sd, a + ".group_norm", g, 1e-6).permute(0, 2, 3, 1).reshape(B, H * W, C)
    o = osd._attn(osd._lin(n, sd, a + ".to_q"), osd._lin(n, sd, a + ".to_k"), osd._lin(n, sd, a + ".to_v"), 1)
    h = osd._lin(o, sd, a + ".to_out.0").reshape(B, H, W, C).permute(0, 3, 1, 2) + h
    h = osd.resnet(h, sd, "decoder.mid_block.resnets.1", None, g, 1e-6)
    nb = len(cfg.block_out_channels)
    for i in range(nb):
        for j in range(cfg.layers_per_block + 1):
            h = osd.resnet(h, sd, "decoder.up_blocks.%d.resnets.%d" % (i, j), None, g, 1e-6)
        if i != nb - 1:
            h = osd._conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), sd, "decoder.up_blocks.%d.upsamplers.0.conv" % i)
    return osd._conv(F.silu(osd._gn(h, sd, "decoder.conv_norm_out", g, 1e-6)), sd, "decoder.conv_out")


def postprocess(raw):
    """VaeImageProcessor.postprocess(..., 'pt'): (x / 2 + 0.5).clamp(0, 1)."""
    return (raw / 2 + 0.5).clamp(0, 1)


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = {"main": main_case, "two_level": two_level_case}[name]()
    sd = state_dict(case)
    lat = latents(case)
    with torch.no_grad():
        raw = decode_oracle(case["cfg"], {k: v.double() for k, v in sd.items()}, lat.double())
    return case, sd, lat, raw


def reference(name):
    """(case, fp32 state dict, fp32 latents, float64 raw oracle output), computed once per process and shared: do not modify."""
    return _reference(name)


# ---------------------------------------------------------------------------------------------------------------- scheduler step
def alphas_cumprod():
    """The fp32 table the guidance object holds (scaled-linear betas of SD-1.5)."""
    from oracle import sd15 as osd
    return osd.sd15_alphas_cumprod()


def ddpm_step_ref(acp, t, t_prev, x_t, eps, noise):
    """The definition (include/dwg_sds.h) in float64 from the fp32 table's values, for ONE view: -> (x0, prev, S_x0, S_prev), S_* the same
    expressions over absolute values."""
    acp, x_t, eps, noise = acp.double(), x_t.double(), eps.double(), noise.double()
    a_t = acp[t]
    a_p = acp[t_prev] if t_prev >= 0 else torch.tensor(1.0, dtype=torch.float64)
    alpha = a_t / a_p
    beta = 1 - alpha
    x0 = (x_t - (1 - a_t).sqrt() * eps) / a_t.sqrt()
    s_x0 = (x_t.abs() + (1 - a_t).sqrt() * eps.abs()) / a_t.sqrt()
    c0, ct = a_p.sqrt() * beta / (1 - a_t), alpha.sqrt() * (1 - a_p) / (1 - a_t)
    prev = c0 * x0 + ct * x_t
    s_prev = c0 * s_x0 + ct * x_t.abs()
    if t > 0:
        sd = ((1 - a_p) / (1 - a_t) * beta).clamp_min(1e-20).sqrt()
        prev = prev + sd * noise
        s_prev = s_prev + sd * noise.abs()
    return x0, prev, s_x0, s_prev


def step_within_bound(out, ref, s):
    """(ok, worst err / bound) of |out - ref| <= ARITH (|ref| + S)."""
    err = (out.double().cpu() - ref).abs()
    bound = ARITH * (ref.abs() + s)
    return bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())


def step_draw(seed, views):
    """(x_t, eps, noise) [views, 4, 9, 9] fp32."""
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((views,) + STEP_SHAPE, generator=g) for _ in range(3))


# ---------------------------------------------------------------------------------------------------------------- converters
def converter_latents(B=2, C=4, h=8):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, C, h, h, generator=g) * 3.0


def converter_image_values(B=2, H=8):
    """fp32 [B, H, H, 8] as the last convolution leaves it (channels 3..7 arbitrary: the unpack must not read them into the image): values inside
    the linear part, beyond both clamps, exactly on them, and one NaN."""
    g = torch.Generator().manual_seed(78)
    v = torch.randn(B, H, H, 8, generator=g) * 1.5
    v[0, 0, 0, 0], v[0, 0, 1, 1], v[1, 2, 3, 2] = 7.25, -9.5, float("nan")
    v[1, 0, 0, 0], v[1, 0, 0, 1] = 1.0, -1.0
    return v
