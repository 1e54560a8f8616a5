"""-m gpu tests of the image reconstruction loss (boundary B17, dreamwaltz_g_amd.image_loss over csrc/image_loss.hip) against the float64
oracle of tests/image_loss_cases.py, and of the nerf2gs forward and step built on it.

The tolerance is measured against the reference's arithmetic, never against the kernels: a result passes with an error of at most
max(4 e_ref, floor), where e_ref is the error of the reference's composition run in fp32 on the CPU (image_loss_cases.case / bound)."""
import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from dreamwaltz_g_amd import image_loss as il
from tests import image_loss_cases as ic

pytestmark = pytest.mark.gpu

PARITY = [(name, layout) for name, (_, layouts, _) in ic.CASES.items() for layout in layouts]


def _leaf(t32, layout):
    """-> (leaf tensor in the layout's memory order, its [B, C, H, W] view)."""
    if layout == "nhwc":
        leaf = t32.permute(0, 2, 3, 1).contiguous().cuda()
        return leaf, leaf.permute(0, 3, 1, 2)
    leaf = t32.contiguous().cuda()
    return leaf, leaf


def _grad_nchw(leaf, layout):
    g = leaf.grad
    return (g.permute(0, 3, 1, 2) if layout == "nhwc" else g).contiguous()


def _loss_and_grad(c, layout, scale=None):
    leaf, _ = _leaf(c["x"], layout)
    leaf.requires_grad_(True)
    _, y = _leaf(c["y"], layout)
    view = leaf.permute(0, 3, 1, 2) if layout == "nhwc" else leaf
    loss = il.ImageReconstructionLoss(ic.LAMBDA)(view, y)
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), _grad_nchw(leaf, layout), view.detach(), y


@pytest.mark.parametrize("name,layout", PARITY)
def test_parity_with_the_float64_oracle(name, layout):
    c = ic.case(name)
    loss, grad, x, y = _loss_and_grad(c, layout)
    got = {"loss": float(loss), "l1": float(il.l1_loss(x, y)), "ssim": float(il.ssim(x, y)), "grad": grad.double().cpu().numpy()}      # x: detached
    if c["shape"][0] > 1:
        per_item = il.ssim(x, y, size_average=False)
        assert per_item.shape == (c["shape"][0],)
        got["ssim_batch"] = per_item.double().cpu().numpy()
    errs = {k: float(np.max(np.abs(np.asarray(v) - np.asarray(c["want"][k])))) for k, v in got.items()}
    gmax = float(np.max(np.abs(c["want"]["grad"])))
    print("image_loss %s %s: " % (name, layout) + "  ".join("%s err %.3e e_ref %.3e bound %.3e" % (k, errs[k], c["e_ref"][k], ic.bound(c, k))
                                                            for k in errs) + "  max|g64| %.3e" % gmax)
    for k in errs:
        assert errs[k] <= ic.bound(c, k), (k, errs[k], c["e_ref"][k], ic.bound(c, k))


def test_two_runs_give_the_same_bits_and_nhwc_equals_nchw():
    c = ic.case("batch_ragged")
    loss_a, grad_a, _, _ = _loss_and_grad(c, "nchw")
    loss_b, grad_b, _, _ = _loss_and_grad(c, "nchw")
    assert torch.equal(loss_a, loss_b) and torch.equal(grad_a, grad_b)
    loss_n, grad_n, _, _ = _loss_and_grad(c, "nhwc")               # read in place through strides against the permuted copy
    assert torch.equal(loss_n, loss_a) and torch.equal(grad_n, grad_a)


def test_gradient_is_exactly_zero_where_the_oracles_is():
    c = ic.case("blob_shifted")
    _, grad, _, _ = _loss_and_grad(c, c["layouts"][0])
    zero = torch.from_numpy(c["want"]["grad"] == 0)
    assert int(zero.sum()) > 100
    assert bool((grad.cpu()[zero] == 0).all())
    assert bool((grad.cpu()[~zero] != 0).any())


def test_upstream_gradient_scales_exactly():
    c = ic.case("one_past_a_tile")
    _, g1, _, _ = _loss_and_grad(c, "nchw")
    _, g3, _, _ = _loss_and_grad(c, "nchw", scale=3.0)
    assert torch.equal(g3, 3.0 * g1) and bool((g1 != 0).any())
    # ssim and l1_loss are differentiable on their own, the per-item ssim with a gradient per item
    leaf, _ = _leaf(c["x"], "nchw")
    leaf.requires_grad_(True)
    y = c["y"].cuda()
    (0.8 * il.l1_loss(leaf, y) + 0.2 * (1.0 - il.ssim(leaf, y))).backward()
    tol = ic.bound(c, "grad")
    assert float((leaf.grad - g1).abs().max()) <= 2 * tol


def test_identical_images_give_exactly_one_and_zero():
    """What the oracle's self-check holds in float64 holds on the device: numerator and denominator of the map are the same bits."""
    c = ic.case("batch_ragged")
    x = c["x"].cuda().requires_grad_(True)
    y = c["x"].cuda().clone()
    loss = il.ImageReconstructionLoss(ic.LAMBDA)(x, y)
    loss.backward()
    xd = x.detach()
    assert float(loss.detach()) == 0.0 and float(il.ssim(xd, y)) == 1.0 and float(il.l1_loss(xd, y)) == 0.0
    assert bool((il.ssim(xd, y, size_average=False) == 1.0).all())
    assert float(x.grad.abs().max()) <= ic.GRAD_FLOOR * float(np.max(np.abs(c["want"]["grad"])))      # zero to rounding


def test_inference_mode_keeps_nothing_for_a_backward():
    c = ic.case("one_past_a_tile")
    loss_fn = il.ImageReconstructionLoss(ic.LAMBDA)
    x, y = c["x"].cuda().requires_grad_(True), c["y"].cuda()
    before = dict(il.stats)
    kept = loss_fn(x, y)
    assert il.stats["maps_allocations"] == before["maps_allocations"] + 1 and il.stats["last_maps_bytes"] == 3 * x.numel() * 4
    with torch.inference_mode():
        free = loss_fn(x, y)
    assert il.stats["forward_calls"] == before["forward_calls"] + 2
    assert il.stats["maps_allocations"] == before["maps_allocations"] + 1 and il.stats["last_maps_bytes"] == 0
    assert torch.equal(free, kept.detach()) and not free.requires_grad
    with torch.no_grad():
        assert torch.equal(loss_fn(x, y), kept.detach()) and il.stats["last_maps_bytes"] == 0
    assert torch.equal(loss_fn(x.detach(), y), kept.detach()) and il.stats["last_maps_bytes"] == 0      # nothing to differentiate


# ---------------------------------------------------------------------------------------------------------------------------------
# nerf2gs: the forward against a bound NeRF teacher, and the step
# ---------------------------------------------------------------------------------------------------------------------------------
# 2400 Gaussians = 2160 free + 240 mesh-bound: from gridencoder.SLAB_MIN_POINTS = 2048 points the grid encoder's table gradient takes its
# deterministic slab path; below it the existing avatar backward adds floats atomically and no step repeats bit for bit
RES, GAUSSIANS = 32, 2400


class _Teacher:
    """What the loop reads of the reference's nerf_guidance: render(data=, shading=) -> {'image_fg': [1, H, W, 3], ...}."""

    def __init__(self, render):
        self._render, self.calls = render, []

    def render(self, data, shading='albedo'):
        self.calls.append((shading, torch.is_grad_enabled()))
        return {"image_fg": self._render()}


def _trainer(dev):
    from dreamwaltz_g_amd import camera, configs, scene as sc, sds_step, synth, trainer as tr
    cfg = configs.TrainConfig()
    cfg.device = str(dev)
    cfg.render.bg_color = (0.5, 0.5, 0.5)
    avatar, _, _ = sds_step.build_synthetic_avatar(GAUSSIANS, dev, seed=0)
    optimizers = avatar.get_optimizer(cfg)
    scene = sc.Scene(cfg, avatar, async_pair_count=False).to(dev)      # exact pair sizing, as the binding builds its scene
    scene.train()
    data = dict(camera.make_camera(radius=2.0, azimuth=20.0, elevation=80.0, fovy=55.0, height=RES, width=RES, device=dev))
    data["smpl_inputs"] = synth.random_smpl_inputs(seed=0, device=dev)
    return tr.SDSTrainer(cfg, scene, None, optimizers, {}, use_controlnet=False, max_step=100), data


def _trainable(trainer):
    return [p for o in trainer.optimizers.values() for pg in o.param_groups for p in pg["params"]]


def test_nerf2gs_forward_end_to_end():
    from dreamwaltz_g_amd import nerf
    from tests import nerf_render_cases as rc
    dev = torch.device("cuda:0")
    o, d, bits, bound = rc.make_scene(2, 32, RES * RES, seed=9)
    net = rc.make_render_network(32, bound).cuda().eval()
    with torch.no_grad():
        net.density_bitfield.copy_(torch.from_numpy(bits))
    assert nerf.bind_nerf_network(net) is None
    rays_o, rays_d = torch.from_numpy(o).cuda()[None], torch.from_numpy(d).cuda()[None]
    teacher = _Teacher(lambda: net.run_cuda(rays_o, rays_d, light_d=rays_o[0, 0], max_steps=rc.MAX_STEPS, T_thresh=rc.T_THRESH)["image"]
                       .reshape(1, RES, RES, 3))
    trainer, data = _trainer(dev)
    trainer.nerf_guidance = teacher
    trainer.losses = {"image": il.ImageReconstructionLoss()}
    trainer._begin_step(trainer.get_spatial_scale(data))
    loss, render_outputs, nerf_outputs = il.nerf2gs_forward(trainer, data)
    assert teacher.calls == [("albedo", False)] and net.run_calls == []          # under no_grad, on the one-launch render
    image, target = render_outputs["image_fg"], nerf_outputs["image_fg"]
    assert image.shape == target.shape == (1, RES, RES, 3) and not target.requires_grad
    assert float((image.detach() - target).abs().max()) > 1e-3
    want = il.ImageReconstructionLoss()(image.detach().permute(0, 3, 1, 2), target.permute(0, 3, 1, 2))
    assert torch.equal(loss.detach(), want) and loss.requires_grad and loss.shape == ()
    loss.backward()
    params = _trainable(trainer)
    assert params and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert any(bool((p.grad != 0).any()) for p in params)
    assert all(p.grad is None for p in net.parameters())


def _three_steps(dev, target):
    trainer, data = _trainer(dev)
    teacher = _Teacher(lambda: target)
    losses = []
    for _ in range(3):
        loss, render_outputs, nerf_outputs = trainer.nerf2gs_step(data, teacher)
        losses.append(loss.detach().clone())
    assert trainer.train_step_index == 3 and nerf_outputs["image_fg"] is target and render_outputs["image_fg"].shape == target.shape
    return losses, trainer.optimizers.buffers.flat.detach().clone()


def test_nerf2gs_step_lowers_the_loss_and_repeats_bit_for_bit():
    dev = torch.device("cuda:0")
    target = torch.rand(1, RES, RES, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    losses_a, flat_a = _three_steps(dev, target)
    losses_b, flat_b = _three_steps(dev, target)
    print("nerf2gs_step losses:", [float(v) for v in losses_a])
    assert float(losses_a[2]) < float(losses_a[0])
    assert all(torch.equal(a, b) for a, b in zip(losses_a, losses_b)) and torch.equal(flat_a, flat_b)
