"""Host-side tests of the view around the NeRF render (boundary B20): csrc/view_math.h compiled for the host (gcc -ffp-contract=off)
against the float64 restatement of tests/nerf_view_cases.py and the reference's own results (tests/golden/nerf_view.npz), the
restatement against the reference, the argument refusals, the optimizer groups of the stage-I model and the binding's decisions.
Needs no device.

THE BOUNDS (the issue's).  rays_d: 16 * 2^-24 absolute per component -- a unit vector after about ten fp32 roundings (subtract, divide,
three squares and two adds, sqrt, divide, three products and two adds against rotation entries <= 1).  Sparsity terms, loss and
derivative: 2^-23 relative -- evaluated in double, one fp32 rounding at the end.  The float64 restatement against the reference's fp32
loss: N * 2^-24 relative, the worst case of an fp32 mean over N = 2145 terms (a check on the restatement, not on the kernel)."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from tests import nerf_view_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32
E_ARG = -1
REL = 2.0 ** -23


def _golden():
    return np.load(os.path.join(HERE, "golden", "nerf_view.npz"))


def _hostlib():
    src = os.path.join(HERE, "hostmath", "view_math_host.c")
    out = os.path.join(HERE, "hostmath", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libview_math_host.so")
    hdr = os.path.join(ROOT, "dreamwaltz-g_amd", "csrc", "view_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src, "-lm"], check=True)
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _host_sparsity(ws, lambdas, mult):
    L = _hostlib()
    N = len(ws)
    terms, sums, loss, grad = np.zeros((N, 3), f32), np.zeros(3, np.float64), np.zeros(1, f32), np.zeros(N, f32)
    L.host_sparsity(N, _p(np.ascontiguousarray(ws, f32)), *(ctypes.c_double(v) for v in lambdas), ctypes.c_double(mult), _p(terms), _p(sums),
                    _p(loss), _p(grad))
    return terms, sums, float(loss[0]), grad


@pytest.mark.parametrize("H,W", vc.SIZES)
def test_rays_against_golden_and_float64(H, W):
    g = _golden()
    tag = "%dx%d" % (H, W)
    c2w, K = vc.camera(H, W)
    assert np.array_equal(c2w, g["c2w_" + tag]) and np.array_equal(K, g["K_" + tag])
    assert K[0, 2] != W / 2 and K[0, 0] != K[1, 1] and (c2w[:3, :3] != 0).all()
    ro, rd = np.zeros((H * W, 3), f32), np.zeros((H * W, 3), f32)
    _hostlib().host_view_rays(_p(c2w), _p(K), H, W, _p(ro), _p(rd))
    o64, d64 = vc.rays(c2w, K, H, W)
    e64, eg = np.abs(rd - d64).max(), np.abs(rd.astype(np.float64) - g["rays_d_" + tag]).max()
    print("view_math rays %s: error / bound %.3g against float64, %.3g against the reference" % (tag, e64 / vc.RAY_BOUND, eg / vc.RAY_BOUND))
    assert e64 <= vc.RAY_BOUND and eg <= vc.RAY_BOUND
    assert np.abs(g["rays_d_" + tag] - d64).max() <= vc.RAY_BOUND             # the restatement itself against the reference
    assert np.array_equal(ro, g["rays_o_" + tag]) and np.array_equal(ro, o64.astype(f32))


def test_the_mix_rounds_every_operation_on_its_own():
    r = np.random.RandomState(4)
    N = 999
    for C, per_pixel in ((3, 0), (4, 0), (3, 1), (4, 1)):
        fg, ws = r.randn(N, C).astype(f32), r.rand(N).astype(f32)
        bg = r.randn(N, C).astype(f32) if per_pixel else r.randn(C).astype(f32)
        out = np.zeros((C, N), f32)
        _hostlib().host_view_mix(N, C, _p(fg), _p(ws), _p(bg), per_pixel, _p(out))
        want = fg + (f32(1) - ws)[:, None] * bg                               # numpy fp32: each operation rounded once
        assert np.array_equal(out, np.ascontiguousarray(want.T))


@pytest.mark.parametrize("case", sorted(vc.LAMBDAS))
@pytest.mark.parametrize("when", sorted(vc.STEPS))
def test_sparsity_terms_loss_and_derivative_against_float64(case, when):
    ws = vc.ws_vector()
    lambdas, mult = vc.LAMBDAS[case], vc.multiplier(vc.STEPS[when])
    terms, sums, loss, grad = _host_sparsity(ws, lambdas, mult)
    t64 = np.stack(vc.sparsity_terms(ws), -1)
    assert (np.abs(terms - t64) <= REL * np.abs(t64)).all()
    l64, g64 = vc.sparsity_loss(ws, lambdas, mult), vc.sparsity_grad(ws, lambdas, mult)
    print("view_math sparsity %s %s: loss error / bound %.3g, derivative %.3g" % (
        case, when, abs(loss - l64) / (REL * abs(l64)), (np.abs(grad - g64) / np.maximum(REL * np.abs(g64), 1e-300))[g64 != 0].max()))
    assert abs(loss - l64) <= REL * abs(l64)
    assert (np.abs(grad - g64) <= REL * np.abs(g64)).all()
    # the entropy term passes no gradient where its clamp is active
    if case == "entropy":
        clamped = (ws.astype(np.float64) < vc.LO) | (ws.astype(np.float64) > vc.HI)
        assert clamped.sum() >= 120 and (grad[clamped] == 0).all() and (grad[~clamped & (ws != 0.5)] != 0).all()


@pytest.mark.parametrize("case", sorted(vc.LAMBDAS))
@pytest.mark.parametrize("when", sorted(vc.STEPS))
def test_the_float64_restatement_against_the_references_fp32_loss(case, when):
    g = _golden()
    ws = vc.ws_vector()
    assert np.array_equal(ws, g["ws"]) and len(ws) == vc.N_WS
    assert (ws == 0).sum() >= 40 and (ws == 1).sum() >= 40 and ((ws > 0) & (ws < 1e-6)).sum() >= 30 and ((ws > 1 - 1e-6) & (ws < 1)).sum() >= 40
    lambdas, mult = vc.LAMBDAS[case], vc.multiplier(vc.STEPS[when])
    want = float(g["loss_%s_%s" % (case, when)])
    l64 = vc.sparsity_loss(ws, lambdas, mult)
    print("restatement %s %s: error / bound %.3g" % (case, when, abs(l64 - want) / (vc.N_WS * vc.U * abs(want))))
    assert abs(l64 - want) <= vc.N_WS * vc.U * abs(want)
    if when == "after":
        assert mult == vc.MULTIPLIER and want > float(g["loss_%s_before" % case]) * 10
    # where the entropy clamp is active the reference's autograd has no gradient either
    if case == "entropy":
        clamped = (ws.astype(np.float64) < vc.LO) | (ws.astype(np.float64) > vc.HI)
        assert (g["grad_%s_%s" % (case, when)][clamped] == 0).all()
        assert np.array_equal(vc.sparsity_grad(ws, lambdas, mult) == 0, g["grad_%s_%s" % (case, when)] == 0)


def test_the_entropy_gate_sits_on_torchs_fp32_thresholds():
    """torch clamps the fp32 tensor against fp32(1e-6) and fp32(1 - 1e-6) and passes the gradient where min <= x <= max: a weights_sum
    equal to a threshold gets a gradient, its fp32 neighbour outside does not -- against fp32 torch autograd of the reference's
    statement on the CPU."""
    lo, hi = f32(1e-6), f32(1 - 1e-6)
    ws = np.array([lo, np.nextafter(lo, f32(0)), np.nextafter(lo, f32(1)), hi, np.nextafter(hi, f32(1)), np.nextafter(hi, f32(0)), 0.25], f32)
    t = torch.from_numpy(ws.copy()).requires_grad_(True)
    al = t.clamp(1e-6, 1 - 1e-6)
    (2e-3 * (- al * torch.log2(al) - (1 - al) * torch.log2(1 - al)).mean()).backward()
    want = t.grad.numpy()
    _, _, _, grad = _host_sparsity(ws, vc.LAMBDAS["entropy"], 1.0)
    assert list(want != 0) == [True, False, True, True, False, True, True]
    assert np.array_equal(grad != 0, want != 0)
    g64 = vc.sparsity_grad(ws, vc.LAMBDAS["entropy"], 1.0)
    assert (np.abs(grad - g64) <= REL * np.abs(g64)).all()


def test_the_library_exports_the_view_and_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    for name in ("dwg_nerf_view_rays", "dwg_nerf_view_compose_workspace_bytes", "dwg_nerf_view_compose_forward", "dwg_nerf_view_compose_backward"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.dwg_nerf_view_compose_workspace_bytes(0) == 0
    assert L.dwg_nerf_view_compose_workspace_bytes(256) == 2 * 24 and L.dwg_nerf_view_compose_workspace_bytes(257) == 3 * 24
    p, odd, p8 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)
    rays = L.dwg_nerf_view_rays
    assert rays(p, p, p, 0, 8, 0.2, p, p, p, p, None) == E_ARG and rays(p, p, p, 8, 40000, 0.2, p, p, p, p, None) == E_ARG
    assert rays(None, p, p, 8, 8, 0.2, p, p, p, p, None) == E_ARG and rays(p, p, p, 8, 8, 0.2, p, None, p, p, None) == E_ARG
    assert rays(p, p, p, 8, 8, float("nan"), p, p, p, p, None) == E_ARG
    assert rays(p, p, ctypes.c_void_p(4098), 8, 8, 0.2, p, p, p, p, None) == E_ARG
    fwd = L.dwg_nerf_view_compose_forward
    lam = (0.0, 0.0, 0.0, 1.0)
    assert fwd(0, 3, 3, p, p, None, 0, *lam, p, None, None, 0, None) == E_ARG                      # N
    assert fwd(64, 5, 3, p, p, None, 0, *lam, p, None, None, 0, None) == E_ARG                     # C
    assert fwd(64, 3, 4, p, p, None, 0, *lam, p, None, None, 0, None) == E_ARG                     # channels_out > C
    assert fwd(64, 3, 3, p, p, None, 1, *lam, p, None, None, 0, None) == E_ARG                     # a mode without its background
    assert fwd(64, 3, 3, p, p, p, 0, *lam, p, None, None, 0, None) == E_ARG                        # a background without a mode
    assert fwd(64, 3, 3, p, p, p, 3, *lam, p, None, None, 0, None) == E_ARG
    assert fwd(64, 4, 4, p8, p, None, 0, *lam, p, None, None, 0, None) == E_ARG                    # four channels: 16-byte rows
    assert fwd(64, 4, 4, p, p, p8, 2, *lam, p, None, None, 0, None) == E_ARG
    assert fwd(64, 3, 3, p, p, None, 0, *lam, p, p, None, 0, None) == E_ARG                        # a loss without its workspace
    assert fwd(64, 3, 3, p, p, None, 0, *lam, p, p, p, 24, None) == E_ARG                          # ... or a small one
    assert fwd(64, 3, 3, p, p, None, 0, float("nan"), 0.0, 0.0, 1.0, p, None, None, 0, None) == E_ARG
    assert fwd(64, 3, 3, None, p, None, 0, *lam, None, None, None, 0, None) == E_ARG               # neither an image nor a loss
    bwd = L.dwg_nerf_view_compose_backward
    assert bwd(64, 3, 3, p, None, None, None, 0, 0, *lam, None, 0, p, p, None, None) == E_ARG      # weights_sum
    assert bwd(64, 3, 3, p, None, p, None, 0, 0, *lam, None, 0, p, None, None, None) == E_ARG      # d_weights_sum
    assert bwd(64, 3, 3, p, None, p, p, 1, 0, *lam, None, 0, p, p, p, None) == E_ARG               # d_image_bg of a constant background
    assert bwd(64, 3, 3, p, p, p, None, 0, 0, *lam, None, 0, p, p, None, None) == E_ARG            # d_sparsity without the forward's sums
    assert bwd(64, 4, 4, p, None, p, None, 0, 0, *lam, None, 0, p8, p, None, None) == E_ARG


def test_python_entry_points_refuse_bad_arguments():
    """B != 1, wrong dtypes and devices: refused on the host, before the library is asked for a launch."""
    from dreamwaltz_g_amd import nerf_view
    c2w, K, aabb = torch.eye(4)[None], torch.eye(3)[None], torch.tensor([-1., -1, -1, 1, 1, 1])
    with pytest.raises(RuntimeError, match="one camera per call"):
        nerf_view.view_rays(torch.eye(4).repeat(2, 1, 1), K, 8, 8, aabb)
    with pytest.raises(RuntimeError, match="one camera per call"):
        nerf_view.view_rays(c2w, torch.eye(3).repeat(3, 1, 1), 8, 8, aabb)
    with pytest.raises(RuntimeError, match="CUDA"):
        nerf_view.view_rays(c2w, K, 8, 8, aabb)
    with pytest.raises(RuntimeError, match="float32|CUDA"):
        nerf_view.view_rays(c2w.double(), K, 8, 8, aabb)
    with pytest.raises(RuntimeError, match="tensor"):
        nerf_view.view_rays(c2w.numpy(), K, 8, 8, aabb)
    with pytest.raises(RuntimeError, match="image size"):
        nerf_view.view_rays(c2w, K, 0, 8, aabb)
    fg, ws = torch.zeros(64, 3), torch.zeros(64)
    with pytest.raises(RuntimeError, match="CUDA"):
        nerf_view.view_compose(fg, ws, None, 8, 8)
    with pytest.raises(RuntimeError, match="H \\* W"):
        nerf_view.view_compose(fg, torch.zeros(63), None, 8, 8)
    with pytest.raises(RuntimeError, match="image_fg"):
        nerf_view.view_compose(torch.zeros(64, 5), ws, None, 8, 8)
    with pytest.raises(RuntimeError, match="tensor"):
        nerf_view.view_compose(fg, ws.numpy(), None, 8, 8)


def _cfg(**kw):
    from dreamwaltz_g_amd import configs
    c = configs.NeRFConfig(bound=1.0, grid_size=16, num_levels=4, desired_resolution=128)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_sparsity_loss_has_the_references_fields_and_schedule():
    from dreamwaltz_g_amd import nerf_view
    sp = nerf_view.SparsityLoss(_cfg(lambda_opacity=1e-3, lambda_emptiness=1.0, sparsity_multiplier=20, sparsity_step=0.4))
    assert (sp.lambda_opacity, sp.lambda_entropy, sp.lambda_emptiness, sp.use_schedule, sp.sparsity_multiplier, sp.sparsity_step) == (
        1e-3, 0.0, 1.0, True, 20, 0.4)
    assert sp.available and not nerf_view.SparsityLoss(_cfg()).available
    assert sp.terms(current_step=39, max_iteration=100) == (1e-3, 0.0, 1.0, 1.0)
    assert sp.terms(current_step=40, max_iteration=100) == (1e-3, 0.0, 1.0, 20.0)
    assert nerf_view.SparsityLoss(_cfg(lambda_opacity=1e-3, sparsity_step=0.4), use_schedule=False).terms(90, 100)[3] == 1.0
    assert nerf_view.SparsityLoss(_cfg())(torch.zeros(4)) == 0.0
    # the loss alone takes any element count: at 256 x 256 only the device check is left to refuse a CPU tensor
    with pytest.raises(RuntimeError, match="CUDA"):
        sp(torch.zeros(1, 256, 256, 1), current_step=1, max_iteration=100)


def test_the_model_refuses_what_is_not_covered_by_name():
    from dreamwaltz_g_amd import nerf_model, nerf_view, nerf_trainer, configs
    for kw, word in ((dict(bg_mode='nerf'), "'nerf' background"), (dict(dmtet=True), "dmtet"), (dict(cuda_ray=False), "cuda_ray"),
                     (dict(structure='dual_mlp'), "dual_mlp"), (dict(nerf_type='latent_tune'), "latent_tune")):
        with pytest.raises(NotImplementedError, match=word):
            nerf_model.NeRFNetwork(_cfg(**kw))
    net = nerf_model.NeRFNetwork(_cfg())
    for kw, word in ((dict(optimizer='adan'), "adan"), (dict(optimizer='adamw'), "adamw"), (dict(lr_policy='warmup'), "warmup"),
                     (dict(lr_policy='ddpm'), "ddpm")):
        with pytest.raises(NotImplementedError, match=word):
            net.get_optimizer(_cfg(**kw))
    # the 'nerf' background asked for at the call: refused before anything is rendered
    data = {'c2w': torch.eye(4)[None], 'intrinsics': torch.eye(3)[None], 'image_height': 4, 'image_width': 4}
    with pytest.raises(NotImplementedError, match="'nerf' background"):
        nerf_view.render_view(net, data, bg_mode='nerf')
    with pytest.raises(RuntimeError, match="one camera per call"):
        nerf_view.render_view(net, dict(data, c2w=torch.eye(4).repeat(2, 1, 1)))
    cfg = configs.TrainConfig()
    cfg.stage, cfg.nerf = 'nerf', _cfg(optimizer='adan')
    with pytest.raises(NotImplementedError, match="adan"):
        nerf_trainer.NeRFSDSTrainer(cfg, net, lambda **kw: None, {})
    cfg.stage, cfg.nerf = 'gs', _cfg()
    with pytest.raises(RuntimeError, match="stage-I"):
        nerf_trainer.NeRFSDSTrainer(cfg, net, lambda **kw: None, {})


def test_get_optimizer_groups_learning_rates_betas_and_eps():
    from dreamwaltz_g_amd import nerf_model, optim
    cfg = _cfg(lr=2e-3)
    net = nerf_model.NeRFNetwork(cfg)
    assert net.img_dims == 3 and net.bg_mode == 'gray' and torch.equal(net.bg_colors['gray'], torch.tensor([0.5, 0.5, 0.5]))
    assert net.cascade == 1 and tuple(net.aabb_train.tolist()) == (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0) and tuple(net.step_counter.shape) == (16, 2)
    assert [type(l) for l in net.sigma_net.net] == [torch.nn.Linear] * 3 and all(l.bias is not None for l in net.sigma_net.net)
    lat = nerf_model.NeRFNetwork(_cfg(nerf_type='latent'))
    assert lat.img_dims == 4 and lat.sigma_net.net[-1].out_features == 5 and lat.bg_colors['gray'].numel() == 4
    before = {k: v.clone() for k, v in net.state_dict().items()}
    opts, scheduler = net.get_optimizer(cfg)
    assert scheduler is None and isinstance(opts, optim.FlatOptimizerDict) and list(opts) == ['nerf']
    o = opts['nerf']
    assert [pg['name'] for pg in o.param_groups] == ['encoder', 'sigma_net', 'sigma_scale']
    assert [pg['lr'] for pg in o.param_groups] == [2e-3 * 10, 2e-3, 2e-3]
    assert all(pg['betas'] == (0.9, 0.99) and pg['eps'] == 1e-15 for pg in o.param_groups)
    assert [len(pg['params']) for pg in o.param_groups] == [1, 6, 1]
    assert o.param_groups[0]['params'][0] is net.encoder.embeddings and o.param_groups[2]['params'][0] is net.sigma_scale
    n = [sum(p.numel() for p in pg['params']) for pg in o.param_groups]
    assert [pg['end'] - pg['start'] >= k for pg, k in zip(o.param_groups, n)] == [True] * 3
    assert o.param_groups[0]['start'] == 0 and o.param_groups[1]['start'] >= o.param_groups[0]['end']
    # re-homing keeps the values, and every gradient is a slice of the one flat buffer
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert all(opts.buffers.owns_grad(p) for p in net.parameters())


class _StubNet:
    """What nerf_view.covered_view and the installed render read of a reference network."""

    def __init__(self, **kw):
        self.training, self.cuda_ray, self.dmtet = False, True, False
        self.bg_mode, self.bg_colors = 'gray', {'gray': None, 'white': None, 'black': None}
        self.aabb_train = self.aabb_infer = torch.zeros(6)
        self.calls = []
        self.__dict__.update(kw)


def test_covered_view_decisions_on_a_stub_network(monkeypatch):
    """The decisions that precede the render's own (covered_call / covered_train_call are B14-B19's and tested there): a fake device
    camera is enough, nothing is launched."""
    from dreamwaltz_g_amd import nerf_view, nerf_render
    seen = []
    monkeypatch.setattr(nerf_render, "covered_call", lambda ref, o, d, shading, perturb, light_d=None: seen.append(("eval", shading, perturb)) or True)
    monkeypatch.setattr(nerf_render, "covered_train_call", lambda ref, o, d, shading, light_d=None: seen.append(("train", shading)) or True)
    monkeypatch.setattr(nerf_view, "_camera_ok", lambda t, tail: isinstance(t, torch.Tensor) and t.dtype == torch.float32
                        and tuple(t.shape) == (1,) + tuple(tail))
    data = {'c2w': torch.eye(4)[None], 'intrinsics': torch.eye(3)[None], 'image_height': 5, 'image_width': 7}
    net = _StubNet()
    assert nerf_view.covered_view(net, data) and seen == [("eval", 'albedo', False)]
    net.training = True
    assert nerf_view.covered_view(net, data, shading='normal') and seen[-1] == ("train", 'normal')
    net.training = False
    n = len(seen)
    assert not nerf_view.covered_view(_StubNet(dmtet=True), data)
    assert not nerf_view.covered_view(_StubNet(cuda_ray=False), data)
    assert not nerf_view.covered_view(net, data, staged=True)
    assert not nerf_view.covered_view(net, dict(data, c2w=torch.eye(4).repeat(2, 1, 1)))             # B != 1
    assert not nerf_view.covered_view(net, dict(data, c2w=torch.eye(4)[None].double()))             # not fp32
    assert not nerf_view.covered_view(net, dict(data, intrinsics=torch.eye(3)[None].numpy()))
    assert not nerf_view.covered_view(net, data, bg_mode='nerf')
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf'), data)
    assert nerf_view.covered_view(_StubNet(bg_mode='nerf'), data, shading='normal')                 # 'normal' never asks for a background
    assert not nerf_view.covered_view(net, data, bg_mode='checkerboard')
    assert not nerf_view.covered_view(net, {'c2w': data['c2w']})
    assert not nerf_view.covered_view(net, data, ambient_ratio=torch.tensor(0.5))
    assert len(seen) == n + 1                                                                       # none of the refusals reached the render's own check
    monkeypatch.undo()
    assert not nerf_view.covered_view(net, data)                                                    # a camera on the CPU


def test_the_binding_installs_render_on_request_and_falls_through(monkeypatch):
    from dreamwaltz_g_amd import nerf, nerf_view

    class Ref:
        def render(self, data, shading='albedo', bg_mode=None, staged=False, **kwargs):
            return ("orig", shading, bg_mode, staged, kwargs)
    ref = Ref()
    assert nerf.bind_nerf_view(ref) is not None and "render" not in ref.__dict__      # only on a network bind_nerf_network has bound
    ref._dwg_nerf_bound = True
    assert nerf.bind_nerf_view(ref) is None
    assert "render" in ref.__dict__ and ref.render.__wrapped__.__func__ is Ref.render
    took = []
    monkeypatch.setattr(nerf_view, "covered_view", lambda *a: took[-1] if took else False)
    monkeypatch.setattr(nerf_view, "render_view", lambda r, data, shading, bg_mode, **kw: ("native", shading, bg_mode, kw))
    assert ref.render({}, shading='normal', bg_mode='white') == ("orig", 'normal', 'white', False, {})
    took.append(True)
    assert ref.render({}, shading='normal', ambient_ratio=0.3) == ("native", 'normal', None, {"ambient_ratio": 0.3})
    assert ref.render({}, unknown_argument=1)[0] == "orig"
    took.append(False)
    assert ref.render({}, staged=True) == ("orig", 'albedo', None, True, {})
    nerf.unbind_nerf_network(ref)
    assert "render" not in ref.__dict__ and ref.render({})[0] == "orig"


_BIND_PROBE = r"""
import json, os, sys, types
sys.path.insert(0, %r); sys.path.insert(0, %r)
import dwg_import  # noqa: F401
import dwg_bind
from dreamwaltz_g_amd import nerf
calls = []
nerf.bind_nerf_network = lambda ref, *a, **kw: calls.append(["network", list(a), kw])
nerf.bind_nerf_view = lambda ref, *a, **kw: calls.append(["view", list(a), kw])
dwg_bind.bind_nerf(types.SimpleNamespace())
print("DWG_NERF_VIEW_BIND " + json.dumps(calls))
"""


def test_the_drop_in_binds_render_only_on_request():
    import json
    import sys
    out = {}
    for value in (None, "1"):
        env = {k: v for k, v in os.environ.items() if k not in ("DWG_BIND_NERF_VIEW", "DWG_BIND_NERF_TRAIN", "DWG_BIND_NERF")}
        if value is not None:
            env["DWG_BIND_NERF_VIEW"] = value
        r = subprocess.run([sys.executable, "-c", _BIND_PROBE % (ROOT, os.path.join(ROOT, "dropin"))], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("DWG_NERF_VIEW_BIND ")][-1]
        out[value] = json.loads(line[len("DWG_NERF_VIEW_BIND "):])
    assert out[None] == [["network", [], {"shaded_render": True}]]
    assert out["1"] == [["network", [], {"shaded_render": True}], ["view", [], {}]]
