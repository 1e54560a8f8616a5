"""What the VAE decoder work (B26) can show without a GPU: the parameter inventory against SD-1.5's published counts, the clamp condition
the GPU cases rely on, the oracle's output shape, the scheduler step's formulas in float64, the inference grid, and the argument checks of
the three new C-ABI entries (made before any device call)."""
import ctypes
import math

import pytest
import torch

from tests import vae_decoder_cases as vc


def _count(shapes, prefix):
    return sum(math.prod(s) for k, s in shapes.items() if k.startswith(prefix))


def test_parameter_counts_are_sd15s():
    from dreamwaltz_g_amd import sd15
    cfg = sd15.VAEConfig()
    dec, enc = sd15.vae_decoder_param_shapes(cfg), sd15.vae_encoder_param_shapes(cfg)
    assert _count(dec, "decoder.") == 49490179 and _count(dec, "post_quant_conv.") == 20
    assert all(k.startswith(("decoder.", "post_quant_conv.")) for k in dec)
    assert _count(enc, "encoder.") == 34163592 and _count(enc, "quant_conv.") == 72
    assert sum(math.prod(s) for s in list(dec.values()) + list(enc.values())) == 83653863
    # the widths change where diffusers' do: the first resnet of a block takes the previous block's width
    assert dec["decoder.up_blocks.2.resnets.0.conv_shortcut.weight"] == (256, 512, 1, 1)
    assert dec["decoder.up_blocks.3.resnets.0.conv_shortcut.weight"] == (128, 256, 1, 1)
    assert "decoder.up_blocks.1.resnets.0.conv_shortcut.weight" not in dec and "decoder.up_blocks.3.upsamplers.0.conv.weight" not in dec
    assert dec["decoder.conv_in.weight"] == (512, 4, 3, 3) and dec["decoder.conv_out.weight"] == (3, 128, 3, 3)


@pytest.mark.parametrize("name", ["main", "two_level"])
def test_cases_reach_both_clamps_and_the_linear_part(name):
    case, sd, lat, raw = vc.reference(name)
    levels = len(case["cfg"].block_out_channels)
    H = case["latent_hw"] * 2 ** (levels - 1)
    assert raw.shape == (case["batch"], 3, H, H) and raw.dtype == torch.float64
    img = raw / 2 + 0.5
    inside = float(((img > 0) & (img < 1)).double().mean())
    assert 0.10 <= inside <= 0.90, inside
    assert int((img <= 0).sum()) > 0 and int((img >= 1).sum()) > 0
    post = vc.postprocess(raw)
    assert float(post.min()) == 0.0 and float(post.max()) == 1.0
    if case["batch"] > 1:
        assert not torch.equal(lat[0], lat[1])


@pytest.mark.parametrize("t,t_prev", vc.STEP_TIMESTEPS)
def test_step_formulas_return_x0_when_eps_is_the_noise(t, t_prev):
    acp = vc.alphas_cumprod()
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(vc.STEP_SHAPE, generator=g, dtype=torch.float64)
    eps = torch.randn(vc.STEP_SHAPE, generator=g, dtype=torch.float64)
    z = torch.randn(vc.STEP_SHAPE, generator=g, dtype=torch.float64)
    a_t = acp.double()[t]
    x_t = a_t.sqrt() * x0 + (1 - a_t).sqrt() * eps
    got, prev, s0, sp = vc.ddpm_step_ref(acp, t, t_prev, x_t, eps, z)
    assert float((got - x0).abs().max()) <= 1e-12 * float(s0.max())
    assert bool((s0 >= got.abs()).all()) and bool((sp >= prev.abs() - 1e-15).all())
    # the posterior mean is a convex-like mix: with eps exact, prev - noise term = sqrt(a_p) x0 + sqrt(1 - a_p - var) ... checked through its limits
    _, prev0, _, _ = vc.ddpm_step_ref(acp, t, t_prev, x_t, eps, torch.zeros_like(z))
    if t_prev < 0:                       # a_p = 1: the previous sample IS x0 (plus 1e-10 noise when t > 0)
        assert float((prev0 - x0).abs().max()) <= 1e-12 * float(s0.max())
        assert float((prev - prev0).abs().max()) <= (1.0001e-10 * float(z.abs().max()) if t > 0 else 0.0)
    else:
        assert float((prev - prev0).abs().max()) > 0


def test_inference_grid():
    from dreamwaltz_g_amd import guidance
    g50 = guidance.inference_timesteps(50)
    assert g50 == list(range(981, 0, -20)) and len(g50) == 50 and g50[0] == 981 and g50[-1] == 1
    assert guidance.inference_timesteps(5) == [801, 601, 401, 201, 1]
    assert guidance.inference_timesteps(5, steps_offset=0) == [800, 600, 400, 200, 0]
    assert [(t, t - 20) for t in g50 if t in (981, 501, 21, 1)] == vc.STEP_TIMESTEPS[:4]
    with pytest.raises(ValueError, match="num_timesteps"):
        guidance.inference_timesteps(0)


def test_new_entries_validate_their_arguments_host_only():
    """Null pointers, negative sizes and misaligned f32x buffers are DWG_E_ARG before any device call; empty calls succeed without a launch."""
    import dreamwaltz_g_amd._lib as _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert L.dwg_vae_latent_pack(0, 4, 8, 8, fake, 1.0, fake, None) == 0 and L.dwg_vae_latent_pack(1, 4, 0, 8, fake, 1.0, fake, None) == 0
    assert L.dwg_vae_latent_pack(1, 4, 8, 8, None, 1.0, fake, None) != 0 and L.dwg_vae_latent_pack(1, 4, 8, 8, fake, 1.0, None, None) != 0
    assert L.dwg_vae_latent_pack(1, 4, 8, 8, fake, 1.0, odd, None) != 0 and L.dwg_vae_latent_pack(-1, 4, 8, 8, fake, 1.0, fake, None) != 0
    assert L.dwg_vae_latent_pack(1, 0, 8, 8, fake, 1.0, fake, None) != 0 and L.dwg_vae_latent_pack(1, 9, 8, 8, fake, 1.0, fake, None) != 0
    assert L.dwg_vae_latent_pack(1, 4, -8, 8, fake, 1.0, fake, None) != 0
    assert L.dwg_vae_image_unpack(0, 8, 8, fake, 0, fake, None) == 0 and L.dwg_vae_image_unpack(2, 8, 0, fake, 1, fake, None) == 0
    assert L.dwg_vae_image_unpack(1, 8, 8, None, 0, fake, None) != 0 and L.dwg_vae_image_unpack(1, 8, 8, fake, 0, None, None) != 0
    assert L.dwg_vae_image_unpack(1, 8, 8, odd, 0, fake, None) != 0 and L.dwg_vae_image_unpack(1, -8, 8, fake, 0, fake, None) != 0
    step = L.dwg_sds_ddpm_step
    assert step(0, 324, fake, fake, fake, fake, 1000, fake, fake, fake, fake, None) == 0
    assert step(2, 0, fake, fake, fake, fake, 1000, fake, fake, fake, fake, None) == 0
    assert step(2, 324, fake, fake, fake, fake, 1000, fake, fake, None, None, None) == 0            # nothing asked for: nothing launched
    assert step(-1, 324, fake, fake, fake, fake, 1000, fake, fake, fake, fake, None) != 0
    assert step(2, -4, fake, fake, fake, fake, 1000, fake, fake, fake, fake, None) != 0
    assert step(2, 322, fake, fake, fake, fake, 1000, fake, fake, fake, fake, None) != 0             # 4 | n
    assert step(2, 324, fake, fake, fake, fake, 0, fake, fake, fake, fake, None) != 0
    assert step(2, 324, None, fake, fake, fake, 1000, fake, fake, fake, fake, None) != 0
    assert step(2, 324, fake, None, fake, fake, 1000, fake, fake, fake, fake, None) != 0
    assert step(2, 324, fake, fake, fake, None, 1000, fake, fake, fake, fake, None) != 0
    assert step(2, 324, fake, fake, fake, fake, 1000, None, fake, fake, fake, None) != 0
    assert step(2, 324, fake, fake, fake, fake, 1000, fake, None, fake, fake, None) != 0
    assert step(2, 324, fake, fake, None, fake, 1000, fake, fake, fake, fake, None) != 0             # prev_sample needs the noise
    assert step(2, 324, odd, fake, fake, fake, 1000, fake, fake, fake, fake, None) != 0
    assert step(2, 324, fake, fake, fake, fake, 1000, fake, fake, odd, fake, None) != 0
    assert step(2, 324, fake, fake, fake, fake, 1000, fake, fake, fake, odd, None) != 0


def test_decoder_refusals_before_any_launch():
    """The checks that need no device: latent_hw range, a state dict that lacks a decoder key (the first missing key is named), a CPU tensor."""
    from dreamwaltz_g_amd import sd15
    case = vc.two_level_case()
    sd = vc.state_dict(case)
    for hw in (4, 7, 129, 256):
        with pytest.raises(ValueError, match="latent_hw must be in 8..128"):
            sd15.VAEDecoderPlan(case["cfg"], sd, "cpu", latent_hw=hw)
    order = list(sd15.vae_decoder_param_shapes(case["cfg"]))
    lacking = {k: v for k, v in sd.items() if k not in ("decoder.mid_block.attentions.0.to_k.bias", "decoder.conv_out.weight")}
    first = [k for k in order if k not in lacking][0]
    assert first == "decoder.mid_block.attentions.0.to_k.bias"
    with pytest.raises(KeyError, match="lacks the decoder key 'decoder.mid_block.attentions.0.to_k.bias'"):
        sd15.VAEDecoderPlan(case["cfg"], lacking, "cpu", latent_hw=8)


def test_denoising_losses_are_refused_in_multi_rank_and_captured_steps():
    """Refused by name before anything is built: the new loss types walk the scheduler grid on the host."""
    import types
    from dreamwaltz_g_amd import step_graph, trainer
    diffusion = types.SimpleNamespace(is_denoising_mode=True, loss_type="x0_final")
    with pytest.raises(NotImplementedError, match="sds_loss_type 'x0_final' is single rank"):
        trainer.SDSTrainer(None, None, diffusion, None, world=2)
    stub = types.SimpleNamespace(model=types.SimpleNamespace(), diffusion=diffusion)
    with pytest.raises(NotImplementedError, match="GraphedTrainStep with sds_loss_type 'x0_final'"):
        step_graph.GraphedTrainStep(stub, {}, {})
