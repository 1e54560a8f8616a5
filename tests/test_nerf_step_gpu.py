"""GPU tests of the native stage-I step (boundary B20): nerf_model.NeRFNetwork + nerf_trainer.NeRFSDSTrainer at 33 x 65 on the
(2, 32, ., 9) scene's box (bound 2, a 32^3 grid in two cascades; the 'scaling' activation, so that sigma_scale takes part) with a stub guidance (a fixed seeded image gradient) and all three
sparsity lambdas set, against the same step composed from the public pieces it replaces and torch.optim.Adam.

Bounds: gradients in the flat buffer against the composed step's, relative L2 <= F32_BWD = 1e-4 (two orders of the same fp32 sums);
parameters after the step against torch.optim.Adam(betas=(0.9, 0.99), eps=1e-15) on the native gradients, rtol 2e-5 / atol 2e-6 (the
tolerance of tests/test_adam_gpu.py)."""
import types

import numpy as np
import pytest
import torch

from tests import nerf_train_cases as tc
from tests import nerf_view_cases as vc
from tests import sigma_guidance_cases as sgc

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda"
H, W = 33, 65
BOUND, GRID = 2.0, 32
SEED = 9


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cfg(**top):
    from dreamwaltz_g_amd import configs
    cfg = configs.TrainConfig()
    cfg.stage, cfg.device = 'nerf', DEV
    cfg.nerf = configs.NeRFConfig(bound=BOUND, grid_size=GRID, num_levels=8, desired_resolution=128, density_prior='gaussian', density_activation='scaling', lr=1e-3,
                                  lambda_opacity=5e-3, lambda_entropy=1e-3, lambda_emptiness=0.5, sparsity_multiplier=20, sparsity_step=0.5)
    cfg.prompt.text_augmentation = False
    cfg.optim.iters = 100
    for k, v in top.items():
        setattr(cfg, k, v)
    return cfg


def _network(cfg, seed=0):
    """A NeRFNetwork with non-trivial parameters (as tests/nerf_field_cases.make_network draws them)."""
    from dreamwaltz_g_amd import nerf_model
    net = nerf_model.NeRFNetwork(cfg.nerf)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.encoder.embeddings.copy_((torch.rand(net.encoder.embeddings.shape, generator=g) * 2 - 1) * 0.5)
        for lin in net.sigma_net.net:
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (2.0 / lin.in_features) ** 0.5)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
        net.sigma_scale.fill_(0.3)
    return net.to(DEV).train()


class _StubGuidance:
    """loss = sum(image * G) with a fixed seeded G: the guidance's call signature and result key."""

    def __init__(self):
        self.G = _t(np.random.RandomState(SEED).randn(1, 3, H, W).astype(f32))
        self.calls = []

    def __call__(self, inputs, text_embeds_dict=None, train_step=0, max_iteration=1, **kwargs):
        self.calls.append((tuple(inputs.shape), inputs.is_contiguous(), train_step, sorted(kwargs)))
        return {"diffusion_loss": (inputs * self.G).sum().reshape(1)}


def _data(h=H, w=W):
    c2w, K = vc.camera(h, w, BOUND)
    return {'c2w': _t(c2w)[None], 'intrinsics': _t(K)[None], 'image_height': h, 'image_width': w, 'body_part': 'full'}


def _trainer(cfg=None, diffusion=None, **kw):
    from dreamwaltz_g_amd import nerf_trainer
    cfg = cfg or _cfg()
    net = _network(cfg)
    opts, _ = net.get_optimizer(cfg.nerf)
    calls = []
    orig = net.update_extra_state

    def counted(*a, **k):
        calls.append(len(calls))
        return orig(*a, **k)
    net.update_extra_state = counted
    text = {'pos': torch.zeros(1, 77, 8, device=DEV)}                        # the stub reads none of it; the trainer selects 'pos'
    tr = nerf_trainer.NeRFSDSTrainer(cfg, net, diffusion or _StubGuidance(), opts, text_embeds_dict=text, use_controlnet=False, **kw)
    tr.update_calls = calls
    return tr


def _named(net):
    return [("embeddings", net.encoder.embeddings), ("sigma_scale", net.sigma_scale)] + [
        ("%s%d" % (n, l), p) for l, lin in enumerate(net.sigma_net.net) for n, p in (("w", lin.weight), ("b", lin.bias))]


def _torch_sparsity(ws, lambdas, mult):
    lo, le, lm = lambdas
    al = ws.clamp(1e-6, 1 - 1e-6)
    loss = lo * torch.sqrt((ws ** 2 + 0.01).mean()) + le * (- al * torch.log2(al) - (1 - al) * torch.log2(1 - al)).mean() \
        + lm * (10000 * torch.log(1 + 10 * ws).mean())
    return loss * mult


def test_the_step_against_the_composed_step_and_torch_adam():
    from dreamwaltz_g_amd import nerf_render, nerf_view, raymarch
    torch.manual_seed(0)
    tr = _trainer()
    net, opts = tr.model, tr.optimizers
    data = _data()
    noises = _t(tc.noises(H * W, SEED))
    before = {n: p.detach().clone() for n, p in _named(net)}
    loss, ro, sd, _ = tr.train_step(data, render_kwargs=dict(noises=noises))
    assert tr.update_calls == [0] and tr.train_step_index == 1 and net.local_step == 1
    assert tr.diffusion.calls == [((1, 3, H, W), True, 1, ['grad_viz', 'scaler'])] and tr.text_embeds_dict['text'] is tr.text_embeds_dict['pos']
    assert float(ro['weights_sum'].detach().max()) > 0.5 and int((ro['weights_sum'] == 0).sum()) > 0
    assert 'sparsity_loss' in ro['regularizations'] and bool(torch.isfinite(loss).all())
    g_native = {n: p.grad.detach().clone() for n, p in _named(net)}
    assert all(opts.buffers.owns_grad(p) for _, p in _named(net))             # the gradients ARE the flat buffer's slices
    after = {n: p.detach().clone() for n, p in _named(net)}

    # the same step from the public pieces: the occupancy grid as the step's update left it, the parameters as they were before it
    twin = _network(tr.cfg)
    twin.load_state_dict(net.state_dict())
    with torch.no_grad():
        for n, p in _named(twin):
            p.copy_(before[n])
    rays_o, rays_d, _, _ = nerf_view.view_rays(data['c2w'], data['intrinsics'], H, W, twin.aabb_train)
    nears, fars = raymarch.near_far_from_aabb(rays_o[0], rays_d[0], twin.aabb_train)
    ws, depth, image = nerf_render.render_rays_train(
        rays_o[0], rays_d[0], nears, fars, twin.density_bitfield, twin.cascade, twin.grid_size, twin.encoder, twin.sigma_net, twin.sigma_scale,
        twin.bound, density_activation=twin.opt.density_activation, density_prior='gaussian', albedo_sigmoid=True, perturb=True, noises=noises)
    image, ws4 = image.reshape(1, H, W, 3), ws.reshape(1, H, W, 1)
    img = (image + (1 - ws4) * torch.tensor([0.5, 0.5, 0.5], device=DEV)).permute(0, 3, 1, 2).contiguous()
    total = (img * tr.diffusion.G).sum() + _torch_sparsity(ws4, (5e-3, 1e-3, 0.5), 1.0)
    total.backward()
    assert torch.equal(ro['image_nchw'], img) and torch.equal(ro['weights_sum'], ws4)
    assert abs(float(loss) - float(total)) <= 1e-5 * abs(float(total))
    worst = 0.0
    for n, p in _named(twin):
        den = float(p.grad.double().norm())
        assert den > 0, n
        worst = max(worst, float((g_native[n].double() - p.grad.double()).norm()) / den)
    print("stage-I step: flat-buffer gradients against the composed step, relative L2 %.3g (bound %g)" % (worst, tc.F32_BWD))
    assert worst <= tc.F32_BWD

    # the parameters after the step: torch.optim.Adam on the native gradients
    ref = {n: torch.nn.Parameter(before[n].clone()) for n, _ in _named(net)}
    lr = tr.cfg.nerf.lr
    groups = [dict(params=[ref["embeddings"]], lr=lr * 10), dict(params=[ref[n] for n in ref if n[0] in "wb"], lr=lr),
              dict(params=[ref["sigma_scale"]], lr=lr)]
    opt = torch.optim.Adam(groups, betas=(0.9, 0.99), eps=1e-15)
    for n, r in ref.items():
        r.grad = g_native[n].clone()
    opt.step()
    for n, r in ref.items():
        assert torch.allclose(after[n], r.data, rtol=2e-5, atol=2e-6), (n, float((after[n] - r.data).abs().max()))
        assert not torch.equal(after[n], before[n]), n


def test_update_extra_state_runs_on_steps_0_and_16_only():
    torch.manual_seed(1)
    tr = _trainer()
    data = _data()
    seen = []
    for i in range(17):
        tr.train_step(data)
        seen.append(len(tr.update_calls))
    assert seen == [1] * 16 + [2], seen
    assert tr.train_step_index == 17 and tr.model.local_step == 1             # the update at step 16 reset the step counter's row index
    assert tr.model.mean_count > 0


def test_sparsity_loss_alone_on_more_elements_than_an_image_side_holds():
    """SparsityLoss(...)(weights_sum) at 256 x 256 (65 536 elements, above the 32 768 limit of an image side) against the float64
    restatement, 2^-23 relative, and its gradient against the restatement's with one rounding per element."""
    from dreamwaltz_g_amd import nerf_view
    sp = nerf_view.SparsityLoss(_cfg().nerf)
    r = np.random.RandomState(11)
    ws = r.rand(1, 256, 256, 1).astype(f32)
    ws.reshape(-1)[:64] = [0.0, 1.0, 1e-7, 1 - 2.0 ** -24] * 16
    t = _t(ws).requires_grad_(True)
    loss = sp(t, current_step=60, max_iteration=100)
    lambdas = (5e-3, 1e-3, 0.5)
    l64 = vc.sparsity_loss(ws.reshape(-1), lambdas, 20.0)
    assert tuple(loss.shape) == () and abs(float(loss) - l64) <= 2.0 ** -23 * abs(l64), (float(loss), l64)
    loss.backward()
    g64 = vc.sparsity_grad(ws.reshape(-1), lambdas, 20.0)
    assert tuple(t.grad.shape) == (1, 256, 256, 1) and (np.abs(t.grad.reshape(-1).cpu().numpy() - g64) <= 2.0 ** -23 * np.abs(g64)).all()
    with pytest.raises(RuntimeError, match="element count"):
        nerf_view.view_compose(None, t.detach().reshape(-1)[:0], None, 1, 0, sparsity=lambdas + (1.0,))


def test_the_schedule_multiplies_the_sparsity_loss():
    torch.manual_seed(2)
    tr = _trainer()
    data = _data()
    noises = _t(tc.noises(H * W, SEED))
    tr.model.update_extra_state()
    sp = tr.losses['sparsity']
    with torch.no_grad():
        tr.train_step_index = 49
        a = tr.render(data, noises=noises)['sparsity_loss']
        tr.train_step_index = 50                                             # 50 / 100 >= sparsity_step
        b = tr.render(data, noises=noises)['sparsity_loss']
        alone = sp(tr.render(data, noises=noises)['weights_sum'], current_step=50, max_iteration=100)
    assert float(a) > 0 and abs(float(b) - 20 * float(a)) <= 4 * 2.0 ** -23 * float(b) and torch.equal(alone, b)


class _SMPLStub:
    def __init__(self, faces, part_fids, wrist_fids):
        self.model = types.SimpleNamespace(faces=faces)
        self.part_fids, self.wrist_fids = part_fids, wrist_fids

    def get_semantic_indices(self, select_parts):
        return None, (list(self.wrist_fids) if list(select_parts) == ['wrists'] else list(self.part_fids))


def test_the_sigma_guidance_branch_runs():
    torch.manual_seed(3)
    V, F = sgc.make_icosphere(2)
    V = (V * 0.6).astype(f32)
    cfg = _cfg(use_sigma_guidance=True, sigma_prob=1.0, predefined_body_parts="hands", sigma_loss_type='margin', sigma_noise_range=0.05,
               sigma_num_points=500, sigma_surface_thickness=0.005, sigma_guidance_peak=15.0, sigma_guidance_delta=0.2, lambda_sigma_sigma=1.0,
               lambda_sigma_albedo=0.0, lambda_sigma_normal=0.0)
    part_fids, wrist_fids = sgc.make_part(V, F)
    smpl = _SMPLStub(np.asarray(F), part_fids, wrist_fids)
    tr = _trainer(cfg, smpl_model=smpl)
    data = dict(_data(), smpl_outputs=types.SimpleNamespace(vertices=_t(V)[None]))
    before = tr.model.sigma_net.net[0].weight.detach().clone()
    loss, ro, _, _ = tr.train_step(data)
    regs = ro['regularizations']
    assert sorted(regs) == ['sigma_loss', 'sparsity_loss'] and bool(torch.isfinite(regs['sigma_loss'])) and float(regs['sigma_loss']) > 0
    total = (ro['image_nchw'] * tr.diffusion.G).sum() + regs['sigma_loss'] + regs['sparsity_loss']
    assert abs(float(loss) - float(total)) <= 1e-5 * abs(float(loss))
    assert not torch.equal(tr.model.sigma_net.net[0].weight, before)
    # without the switch (and with a body part that asks for none) the branch stays out
    tr2 = _trainer()
    _, ro2, _, _ = tr2.train_step(_data())
    assert sorted(ro2['regularizations']) == ['sparsity_loss']


def test_one_step_with_the_reduced_width_guidance():
    """The real guidance object at the reduced width tests/test_sds_step_gpu.py uses, 64 x 64: the loss is finite and the parameters move."""
    from dreamwaltz_g_amd import guidance, sd15
    torch.manual_seed(4)
    res = 64
    dev = torch.device(DEV)
    ucfg = sd15.UNetConfig(block_out_channels=(64, 128, 128, 128), cross_dim=64, cond_channels=(16, 32, 32, 64))
    vcfg = sd15.VAEConfig(block_out_channels=(32, 64, 64, 64))
    usd = sd15.random_state_dict(sd15.unet_param_shapes(ucfg), seed=1)
    csd = sd15.random_state_dict(sd15.controlnet_param_shapes(ucfg), seed=2)
    vsd = sd15.random_state_dict(sd15.vae_encoder_param_shapes(vcfg), seed=3)
    gd = guidance.ControlNetScoreDistillation(dev, ucfg, vcfg, usd, csd, vsd, image_hw=res, dtype="f32x")
    tg = torch.Generator().manual_seed(5)
    text = {k: torch.randn(1, 77, 64, generator=tg).to(dev) for k in ("neg", "pos", "text")}
    from dreamwaltz_g_amd import nerf_trainer
    cfg = _cfg()
    net = _network(cfg)
    opts, _ = net.get_optimizer(cfg.nerf)
    tr = nerf_trainer.NeRFSDSTrainer(cfg, net, gd, opts, text_embeds_dict=text, use_controlnet=True)
    data = dict(_data(res, res), cond_images=torch.rand(1, 3, res, res, generator=tg).to(dev))
    before = {n: p.detach().clone() for n, p in _named(net)}
    loss, ro, sd, _ = tr.train_step(data)
    assert bool(torch.isfinite(loss).all()) and tuple(ro['image_nchw'].shape) == (1, 3, res, res)
    assert bool(torch.isfinite(sd['gradients']).all())
    for n, p in _named(net):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p, before[n]), n


def test_a_checkpoint_round_trip_reproduces_the_next_steps_gradients(tmp_path):
    torch.manual_seed(5)
    tr = _trainer()
    data = _data()
    n1, n2 = _t(tc.noises(H * W, SEED)), _t(tc.noises(H * W, SEED + 1))
    tr.train_step(data, render_kwargs=dict(noises=n1))
    path = tr.save_checkpoint(str(tmp_path), full=True)
    tr.train_step(data, render_kwargs=dict(noises=n2))
    want_g = tr.optimizers.buffers.grad.clone()
    want_p = tr.optimizers.buffers.flat.clone()
    tr2 = _trainer()
    assert not torch.equal(tr2.optimizers.buffers.flat, want_p)
    tr2.load_checkpoint(path)
    assert tr2.train_step_index == 1 and tr2.model.local_step == 1 and tr2.optimizers['nerf'].t == 1
    assert torch.equal(tr2.model.density_bitfield, tr.model.density_bitfield)
    tr2.train_step(data, render_kwargs=dict(noises=n2))
    assert tr2.update_calls == []                                            # step index 1: no occupancy update, the loaded grid is used
    assert torch.equal(tr2.optimizers.buffers.grad, want_g) and torch.equal(tr2.optimizers.buffers.flat, want_p)
