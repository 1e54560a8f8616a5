"""GPU tests of the native stage-I step under cfg.optim.fp16 (boundary B21): the tiny configuration of tests/test_nerf_step_gpu.py
(its box, grid, 8 levels and stub guidance) with the step under fp16 autocast and grad_scaler.FlatGradScaler, against the same pieces
under autocast driven by torch.amp.GradScaler('cuda') and the plain FlatOptimizer.step().

Bounds: the loss 1e-5 relative; flat-buffer gradients (scaled on both sides) against the composed step's, relative L2 <= F32_BWD = 1e-4
(the two sides share every f16 kernel and differ in fp32 statements only); parameters after each step rtol 2e-5 / atol 2e-6, the composed
side stepping on the native gradients as the fp32 twin's torch.optim.Adam does; scale and growth tracker exact."""
import types

import numpy as np
import pytest
import torch

from tests import nerf_train_cases as tc
from tests import sigma_guidance_cases as sgc
from tests import test_nerf_step_gpu as base

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = base.DEV
H, W, SEED = base.H, base.W, base.SEED


class _Guidance(base._StubGuidance):
    """The stub with a choice of image gradient, and a non-finite one on the trainer steps listed in `bad_steps`."""

    def __init__(self, G=None, bad_steps=()):
        super().__init__()
        if G is not None:
            self.G = G
        self.bad_steps = set(bad_steps)

    def __call__(self, inputs, text_embeds_dict=None, train_step=0, max_iteration=1, **kwargs):
        self.calls.append((tuple(inputs.shape), inputs.is_contiguous(), train_step, sorted(kwargs)))
        G = torch.full_like(self.G, float("inf")) if train_step in self.bad_steps else self.G
        return {"diffusion_loss": (inputs * G).sum().reshape(1)}


def _trainer(fp16=True, diffusion=None, cfg=None, scaler_kw=None, **kw):
    from dreamwaltz_g_amd.grad_scaler import FlatGradScaler
    cfg = cfg or base._cfg()
    cfg.optim.fp16 = fp16
    tr = base._trainer(cfg, diffusion=diffusion or _Guidance(), **kw)
    if fp16:
        assert isinstance(tr.scaler, FlatGradScaler) and tr.scaler.get_scale() == 65536.0
        tr.scaler = FlatGradScaler(device=DEV, **dict(dict(growth_interval=2), **(scaler_kw or {})))
    return tr


def _noises(k):
    return base._t(tc.noises(H * W, SEED + k))


def _composed_forward(twin, data, noises, G):
    """The forward of the step from the public pieces, under the reference's autocast region: -> (total loss, image, weights_sum)."""
    from dreamwaltz_g_amd import nerf_render, nerf_view, raymarch
    with torch.autocast('cuda', dtype=torch.float16):
        rays_o, rays_d, _, _ = nerf_view.view_rays(data['c2w'], data['intrinsics'], H, W, twin.aabb_train)
        nears, fars = raymarch.near_far_from_aabb(rays_o[0], rays_d[0], twin.aabb_train)
        ws, depth, image = nerf_render.render_rays_train(
            rays_o[0], rays_d[0], nears, fars, twin.density_bitfield, twin.cascade, twin.grid_size, twin.encoder, twin.sigma_net, twin.sigma_scale,
            twin.bound, density_activation=twin.opt.density_activation, density_prior='gaussian', albedo_sigmoid=True, perturb=True, noises=noises)
        image, ws4 = image.reshape(1, H, W, 3), ws.reshape(1, H, W, 1)
        img = (image + (1 - ws4) * torch.tensor([0.5, 0.5, 0.5], device=DEV)).permute(0, 3, 1, 2).contiguous()
        total = (img * G).sum() + base._torch_sparsity(ws4, (5e-3, 1e-3, 0.5), 1.0)
    return total, img, ws4


def test_the_fp16_step_against_the_composed_step_under_torchs_grad_scaler():
    from dreamwaltz_g_amd import optim
    torch.manual_seed(0)
    tr = _trainer()
    net, opts = tr.model, tr.optimizers
    data = base._data()
    twin = base._network(tr.cfg)
    opts_b, _ = twin.get_optimizer(tr.cfg.nerf)
    ts = torch.amp.GradScaler('cuda', growth_interval=2)
    worst = 0.0
    for step in range(4):
        noises = _noises(step)
        loss, ro, _, _ = tr.train_step(data, render_kwargs=dict(noises=noises))
        assert loss.dtype == torch.float32 and bool(torch.isfinite(loss).all())
        g_native = opts.buffers.grad.clone()                                   # scaled: the unscale is the Adam launch's
        if step == 0:
            # the occupancy grid as the step's update left it; the parameters as they were before it (both networks start from one seed)
            assert tr.update_calls == [0]
            keep = opts_b.buffers.flat.clone()
            twin.load_state_dict(net.state_dict())
            opts_b.buffers.flat.copy_(keep)
            optim.PARAM_EPOCH[0] += 1
        total, img, ws4 = _composed_forward(twin, data, noises, tr.diffusion.G)
        opts_b.zero_grad()
        ts.scale(total).backward()
        assert torch.equal(ro['image_nchw'], img) and torch.equal(ro['weights_sum'], ws4)
        assert abs(float(loss.detach()) - float(total.detach())) <= 1e-5 * abs(float(total.detach()))
        for (n, p), (_, q) in zip(base._named(net), base._named(twin)):
            off, cnt = p._dwg_off, p.numel()
            a, b = g_native[off:off + cnt].double(), q.grad.reshape(-1).double()
            den = float(b.norm())
            assert den > 0, n
            worst = max(worst, float((a - b).norm()) / den)
        # the composed side steps on the native gradients (what the fp32 twin's torch.optim.Adam does): the bound below is the optimizer's
        opts_b.buffers.grad.copy_(g_native)
        ts.step(opts_b['nerf'])
        ts.update()
        tr_scale, tr_tracker = tr.scaler.get_scale(), tr.scaler._get_growth_tracker()
        assert tr_scale == ts.get_scale() and tr_tracker == ts._get_growth_tracker(), (step, tr_scale, tr_tracker)
        assert tr_scale == (65536.0, 131072.0, 131072.0, 262144.0)[step] and tr_tracker == (1, 0, 1, 0)[step]
        diff = float((opts.buffers.flat - opts_b.buffers.flat).abs().max())
        print("fp16 step %d: max |parameter difference| against the composed step %.3g" % (step, diff))
        assert torch.allclose(opts.buffers.flat, opts_b.buffers.flat, rtol=2e-5, atol=2e-6), (step, diff)
        assert opts['nerf'].device_step_counts() == [step + 1] * 3 and [pg["t"] for pg in opts_b['nerf'].param_groups] == [step + 1] * 3
    print("fp16 stage-I step: flat-buffer gradients against the composed step over 4 steps, relative L2 %.3g (bound %g)" % (worst, tc.F32_BWD))
    assert worst <= tc.F32_BWD


def test_a_nonfinite_image_gradient_skips_that_step_only():
    torch.manual_seed(1)
    tr = _trainer(diffusion=_Guidance(bad_steps=(2,)))
    buf, o = tr.optimizers.buffers, tr.optimizers['nerf']
    data = base._data()
    tr.train_step(data, render_kwargs=dict(noises=_noises(0)))
    assert tr.scaler.get_scale() == 65536.0 and tr.scaler._get_growth_tracker() == 1 and o.device_step_counts() == [1, 1, 1]
    before = [t.clone() for t in (buf.flat, buf.m, buf.v)]
    tr.train_step(data, render_kwargs=dict(noises=_noises(1)))
    assert not bool(torch.isfinite(buf.grad).all())
    assert all(torch.equal(a, b) for a, b in zip(before, (buf.flat, buf.m, buf.v)))
    assert tr.scaler.get_scale() == 32768.0 and tr.scaler._get_growth_tracker() == 0 and o.device_step_counts() == [1, 1, 1]
    assert tr.train_step_index == 2 and o.t == 2
    tr.train_step(data, render_kwargs=dict(noises=_noises(2)))
    assert bool(torch.isfinite(buf.grad).all()) and bool(torch.isfinite(buf.flat).all())
    assert not any(torch.equal(a, b) for a, b in zip(before, (buf.flat, buf.m, buf.v)))
    assert tr.scaler.get_scale() == 32768.0 and tr.scaler._get_growth_tracker() == 1 and o.device_step_counts() == [2, 2, 2]


def test_the_scale_keeps_small_gradients_that_fp16_flushes_without_it():
    """A stub image gradient of 2^-22 per element: at scale 1 every output-layer dZ is below fp16's smallest subnormal (2^-24 and less
    once the compositing weights have multiplied it) and rounds to 0 or one quantum; at 2^16 the same values sit near 2^-6.  The unscaled
    sigma_net gradient of the fp16 step against the fp32 step's on the same scene: the error at 2^16 is smaller than at 1.  (Sparsity
    lambdas off: only the guidance's gradient flows.)

    The network is the tiny configuration's with its table scaled by 0.2 and its weights by 0.5.  The fp32 step is a reference for the
    f16 backward only where the f16 FORWARD tracks the f32 one; with the step test's large random weights it does not (measured with a
    stub gradient of magnitude 1, where nothing flushes and the scale cannot matter: sigma_net 0.79 relative L2, cosine 0.70), with the
    scaled ones it does (0.18, cosine 0.98), and what is left to compare is the backward's rounding.  Measured here: 0.18 at scale
    2^16 (the forward's difference again: nothing is lost to the flush) against 1.0 at scale 1 (the gradient is exactly zero)."""
    from dreamwaltz_g_amd import optim
    torch.manual_seed(2)
    signs = np.sign(np.random.RandomState(SEED).randn(1, 3, H, W)).astype(f32)
    G = base._t(signs * f32(2.0 ** -22))

    def cfg():
        c = base._cfg()
        c.nerf.lambda_opacity = c.nerf.lambda_entropy = c.nerf.lambda_emptiness = 0.0
        return c
    runs = {"fp32": _trainer(False, _Guidance(G), cfg()), 65536.0: _trainer(True, _Guidance(G), cfg(), dict(init_scale=65536.0)),
            1.0: _trainer(True, _Guidance(G), cfg(), dict(init_scale=1.0))}
    first = runs["fp32"]
    with torch.no_grad():
        first.model.encoder.embeddings.mul_(0.2)
        for lin in first.model.sigma_net.net:
            lin.weight.mul_(0.5)
    first.model.update_extra_state()                                          # one set of parameters and one occupancy grid for the three runs
    state = first.model.state_dict()
    render_state = {k: getattr(first.model, k) for k in ('local_step', 'mean_count', 'iter_density', 'mean_density')}
    data, noises = base._data(), _noises(0)
    grads = {}
    for key, tr in runs.items():
        tr.model.load_state_dict(state)
        optim.PARAM_EPOCH[0] += 1
        for k, v in render_state.items():
            setattr(tr.model, k, v)
        tr.train_step_index = 1                                               # no occupancy update inside the step
        tr.train_step(data, render_kwargs=dict(noises=noises))
        pg = tr.optimizers['nerf'].param_groups[1]
        assert pg['name'] == 'sigma_net'
        g = tr.optimizers.buffers.grad[pg['start']:pg['end']].double()
        grads[key] = g if key == "fp32" else g / key
    den = float(grads["fp32"].norm())
    assert den > 0
    err = {k: float((grads[k] - grads["fp32"]).norm()) / den for k in (65536.0, 1.0)}
    print("sigma_net gradient of the fp16 step against the fp32 step's, relative L2: %.3g at scale 2^16, %.3g at scale 1" % (err[65536.0], err[1.0]))
    assert err[65536.0] < err[1.0]


def test_the_sigma_guidance_branch_and_the_normal_shading_run_under_fp16():
    torch.manual_seed(3)
    V, F = sgc.make_icosphere(2)
    V = (V * 0.6).astype(f32)
    cfg = base._cfg(use_sigma_guidance=True, sigma_prob=1.0, predefined_body_parts="hands", sigma_loss_type='margin', sigma_noise_range=0.05,
                    sigma_num_points=500, sigma_surface_thickness=0.005, sigma_guidance_peak=15.0, sigma_guidance_delta=0.2, lambda_sigma_sigma=1.0,
                    lambda_sigma_albedo=0.0, lambda_sigma_normal=0.0)
    part_fids, wrist_fids = sgc.make_part(V, F)
    smpl = base._SMPLStub(np.asarray(F), part_fids, wrist_fids)
    tr = _trainer(cfg=cfg, smpl_model=smpl)
    data = dict(base._data(), smpl_outputs=types.SimpleNamespace(vertices=base._t(V)[None]))
    before = tr.model.sigma_net.net[0].weight.detach().clone()
    loss, ro, _, _ = tr.train_step(data)
    regs = ro['regularizations']
    assert sorted(regs) == ['sigma_loss', 'sparsity_loss'] and bool(torch.isfinite(regs['sigma_loss'])) and float(regs['sigma_loss'].detach()) > 0
    assert bool(torch.isfinite(loss.detach()).all()) and tr.optimizers['nerf'].device_step_counts() == [1, 1, 1]
    assert not torch.equal(tr.model.sigma_net.net[0].weight, before)
    # shading 'normal' (the normal-adapted guidance).  The finite-difference normal multiplies the gradient by 1 / (2 epsilon) = 500, so the
    # f16 backward overflows at the initial scale of 2^16 (the stub's gradient is of order 1): those steps are skipped bit for bit while the
    # scale halves, as under torch's GradScaler, until one fits.  2^16 x 500 x the stub's largest |G| (below 8) is under 2^28 and fp16
    # holds 2^16: twelve halvings are more than enough.
    cfg2 = base._cfg()
    cfg2.guide.diffusion = 'normal-adapted'
    tr2 = _trainer(cfg=cfg2, scaler_kw=dict(growth_interval=2000))
    buf, o = tr2.optimizers.buffers, tr2.optimizers['nerf']
    data2, skipped = base._data(), 0
    for _ in range(12):
        before = [t.clone() for t in (buf.flat, buf.m, buf.v)]
        loss2, ro2, _, _ = tr2.train_step(data2)
        assert tuple(ro2['image_nchw'].shape) == (1, 3, H, W) and bool(torch.isfinite(loss2.detach()).all())
        if o.device_step_counts() == [1, 1, 1]:
            break
        skipped += 1
        assert o.device_step_counts() == [0, 0, 0] and not bool(torch.isfinite(buf.grad).all())
        assert all(torch.equal(a, b) for a, b in zip(before, (buf.flat, buf.m, buf.v)))
        assert tr2.scaler.get_scale() == 65536.0 / 2 ** skipped
    print("fp16 step with shading 'normal': %d steps skipped, the first step taken at scale %g" % (skipped, tr2.scaler.get_scale()))
    assert o.device_step_counts() == [1, 1, 1] and bool(torch.isfinite(buf.grad).all()) and bool(torch.isfinite(buf.flat).all())
    assert not torch.equal(before[0], buf.flat)


def test_a_checkpoint_round_trip_after_a_skipped_step_reproduces_the_next_step(tmp_path):
    torch.manual_seed(5)
    tr = _trainer(diffusion=_Guidance(bad_steps=(2,)))
    data = base._data()
    tr.train_step(data, render_kwargs=dict(noises=_noises(0)))
    tr.train_step(data, render_kwargs=dict(noises=_noises(1)))                # skipped
    path = tr.save_checkpoint(str(tmp_path), full=True)
    saved = torch.load(path, weights_only=False)
    assert saved['scaler'] == {"scale": 32768.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2, "_growth_tracker": 0}
    assert [pg["t"] for pg in saved['optimizers'][0]['param_groups']] == [1, 1, 1] and saved['optimizers'][0]['t'] == 2
    tr.train_step(data, render_kwargs=dict(noises=_noises(2)))
    want_g, want_p = tr.optimizers.buffers.grad.clone(), tr.optimizers.buffers.flat.clone()
    tr2 = _trainer(diffusion=_Guidance(bad_steps=(2,)))
    assert not torch.equal(tr2.optimizers.buffers.flat, want_p)
    tr2.load_checkpoint(path)
    assert tr2.train_step_index == 2 and tr2.scaler.get_scale() == 32768.0 and tr2.scaler._get_growth_tracker() == 0
    tr2.train_step(data, render_kwargs=dict(noises=_noises(2)))
    assert tr2.update_calls == []
    assert tr2.scaler.get_scale() == tr.scaler.get_scale() and tr2.scaler._get_growth_tracker() == tr.scaler._get_growth_tracker() == 1
    assert tr2.optimizers['nerf'].device_step_counts() == tr.optimizers['nerf'].device_step_counts() == [2, 2, 2]
    assert torch.equal(tr2.optimizers.buffers.grad, want_g) and torch.equal(tr2.optimizers.buffers.flat, want_p)
    assert torch.equal(tr2.optimizers.buffers.m, tr.optimizers.buffers.m) and torch.equal(tr2.optimizers.buffers.v, tr.optimizers.buffers.v)
