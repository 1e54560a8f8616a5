"""Without a GPU: what a shared-prefix denoiser plan (sd15.DenoiserPlan(shared_prefix=True)) checks before it builds anything, and that a
CPU device is turned away exactly like it is for the plain plan -- the plans are lists of HIP launches and have no CPU path."""
import pytest
import torch

from dreamwaltz_g_amd import sd15


def _args():
    ucfg = sd15.UNetConfig(block_out_channels=(32, 64), layers_per_block=1, heads=4, cross_dim=48, groups=8, attn_blocks=(True, False),
                           cond_channels=(16, 32))
    return ucfg, sd15.random_state_dict(sd15.unet_param_shapes(ucfg), seed=0), sd15.random_state_dict(sd15.controlnet_param_shapes(ucfg), seed=1)


def test_shared_prefix_arguments_are_checked_before_anything_is_built():
    ucfg, usd, csd = _args()
    with pytest.raises(ValueError):                     # the CFG pair of each view: batch = 2 views
        sd15.DenoiserPlan(ucfg, usd, csd, torch.device("cpu"), batch=2, latent_hw=8, dtype="f32x", views=2, shared_prefix=True)
    with pytest.raises(ValueError):
        sd15.DenoiserPlan(ucfg, usd, csd, torch.device("cpu"), batch=3, latent_hw=8, dtype="bf16", views=1, shared_prefix=True)
    with pytest.raises(NotImplementedError):            # exact-f32 attention runs on dwg_gemm: image x head are its two batch levels
        sd15.DenoiserPlan(ucfg, usd, csd, torch.device("cpu"), batch=2, latent_hw=8, dtype="f32", shared_prefix=True)


@pytest.mark.parametrize("shared", [False, True])
def test_a_cpu_device_is_refused_the_same_way_with_and_without_the_flag(shared):
    """No CPU fallback on the product path (gemm.gemm_raw): the first contraction of the plan raises, for both kinds of plan."""
    ucfg, usd, csd = _args()
    with pytest.raises(RuntimeError, match="GPU only"):
        sd15.DenoiserPlan(ucfg, usd, csd, torch.device("cpu"), batch=2, latent_hw=8, dtype="bf16", shared_prefix=shared)
