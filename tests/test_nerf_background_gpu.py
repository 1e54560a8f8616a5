"""GPU tests of the learned background (boundary B22, dreamwaltz_g_amd.nerf_background): the encoding and the fused bg_net kernels
against the float64 restatement of tests/nerf_background_cases.py, render_view against the composition of the public pieces, the
stage-I step with the bg_net group, and the binding of a reference-shaped network.

THE BOUNDS.
  freq_encode: columns 0..2 exact; the others within 2 * FREQ_DEV of float64, FREQ_DEV being the device's sinf / cosf error on the
      exact argument (the host test's bound form, measured on the device).
  forward, precision 0: max|err| / max|ref| against float64 at most 2 * (the fp32 torch composition's) + 1e-7 -- the rule
      tests/test_nerf_field_gpu.py uses for fp16 --, and at most F32_FWD_BG = 4 * the native error measured on the first green run.
  backward, precision 0: every gradient within relative L2 F32_BWD = 1e-4 of float64 (fp32 sums of this kind).
  precision 1: forward and every gradient at most 2 * (the autocast torch composition's error) + 1e-7, all against float64.
  render_view, the step, the binding: bit for bit against the composition of the public pieces."""
import random

import numpy as np
import pytest
import torch

from tests import nerf_background_cases as bc
from tests import nerf_render_cases as rc
from tests import nerf_train_cases as tc
from tests import nerf_view_cases as vc

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda"
FREQ_DEV = 5.73e-8           # measured on an MI355X: max |error| of the device's sinf / cosf over test_freq_encode's cases (degree 6 and 8 alike)
F32_FWD_BG = 4 * 2.6e-7      # 4 x the largest native max|err| / max|ref| measured on an MI355X over test_forward_f32's cases (the fp32 torch
                             # composition's largest there: 2.34e-7)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nb():
    from dreamwaltz_g_amd import nerf_background
    return nerf_background


_DIRS = {}


def _dirs(n):
    if n not in _DIRS:
        _DIRS[n] = _t(bc.directions(n, seed=n))
    return _DIRS[n]


# --------------------------------------------------------------------------------------------------------------------------------------
# 1. the encoding
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [6, 8])
@pytest.mark.parametrize("N", bc.NS)
def test_freq_encode(N, degree):
    x = _dirs(N)
    got = _nb().freq_encode(x, degree)
    assert tuple(got.shape) == (N, 3 + 6 * degree) and got.dtype == torch.float32 and got.is_contiguous()
    want = bc.encode(x, degree)
    assert torch.equal(got[:, :3], x)
    err = (got.double() - want).abs()
    for c in (3, 3 + 6 * degree - 1):                                                   # the layout's ends, by the formula
        kind, f, d = bc.column(degree, c)
        col = (torch.sin if kind == 'sin' else torch.cos)(x[:, d].double() * 2.0 ** f)
        assert float((got[:, c].double() - col).abs().max()) <= 2 * FREQ_DEV
    print("freq_encode N=%d degree=%d: max |error| %.3g (FREQ_DEV %.3g)" % (N, degree, float(err.max()), FREQ_DEV))
    assert float(err.max()) <= 2 * FREQ_DEV
    # the module and a [..., 3] prefix
    enc = _nb().FreqEncoder(3, degree).to(DEV)
    assert torch.equal(enc(x.view(1, N, 3)), got.view(1, N, -1))


# --------------------------------------------------------------------------------------------------------------------------------------
# 2-5. the fused background
# --------------------------------------------------------------------------------------------------------------------------------------
def _case(C, layers, hidden, degree=6, seed=0):
    return bc.make_bg(C=C, layers=layers, hidden=hidden, degree=degree, seed=seed + 10 * C + layers, device=DEV)


SHAPES = [(1, 16, 6), (2, 16, 6), (1, 64, 6), (2, 64, 6), (3, 32, 8)]                   # (layers, hidden, degree); the last: every maximum but the width


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("layers,hidden,degree", SHAPES)
def test_forward_f32(layers, hidden, degree, C):
    enc, bg = _case(C, layers, hidden, degree)
    sigmoid = C == 3
    worst = 0.0
    for N in bc.NS:
        x = _dirs(N)
        with torch.no_grad():
            got = _nb().learned_background(x, enc, bg, sigmoid=sigmoid, precision=0)
            ref = bc.background(x, enc, bg, sigmoid, torch.float64)
            comp = bc.background(x, enc, bg, sigmoid, torch.float32)
        assert tuple(got.shape) == (N, C) and got.dtype == torch.float32 and not got.requires_grad
        en, ec = bc.rel_max(got, ref), bc.rel_max(comp, ref)
        print("learned_background f32 layers=%d hidden=%d degree=%d C=%d N=%d: native %.3g, composition %.3g" % (layers, hidden, degree, C, N, en, ec))
        assert en <= 2 * ec + 1e-7, (N, en, ec)
        worst = max(worst, en)
    assert worst <= F32_FWD_BG, worst
    assert sigmoid == bool(float(got.min()) >= 0 and float(got.max()) <= 1)              # the identity epilogue leaves the unit interval


def _native_grads(x, enc, bg, sigmoid, cot, precision, trainable=None):
    ps = [p for lin in bg.net for p in (lin.weight, lin.bias)]
    for i, p in enumerate(ps):
        p.grad = None
        p.requires_grad_(trainable is None or i in trainable)
    out = _nb().learned_background(x, enc, bg, sigmoid=sigmoid, precision=precision)
    out.backward(cot)
    g = [None if p.grad is None else p.grad.detach().clone() for p in ps]
    for p in ps:
        p.grad = None
        p.requires_grad_(True)
    return out.detach(), g


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("layers,hidden,degree", [(1, 64, 6), (2, 64, 6), (2, 16, 6), (3, 32, 8)])
@pytest.mark.parametrize("N", [1, 65, 4097])
def test_backward_f32(N, layers, hidden, degree, C):
    enc, bg = _case(C, layers, hidden, degree)
    sigmoid = C == 3
    x = _dirs(N)
    cot = torch.randn(N, C, device=DEV, generator=torch.Generator(DEV).manual_seed(N + C))
    _, want = bc.oracle_grads(x, enc, bg, sigmoid, cot)
    out, got = _native_grads(x, enc, bg, sigmoid, cot, 0)
    worst = 0.0
    for a, b in zip(got, want):
        assert a is not None and a.shape == b.shape and float(b.norm()) > 0
        worst = max(worst, bc.rel_l2(a, b))
    print("learned_background backward f32 layers=%d hidden=%d C=%d N=%d: worst relative L2 %.3g (bound %g)" % (layers, hidden, C, N, worst, bc.F32_BWD))
    assert worst <= bc.F32_BWD
    if layers == 2 and hidden == 64:
        # only layer 1's weight trainable: that gradient alone, with the bits of the full run
        _, part = _native_grads(x, enc, bg, sigmoid, cot, 0, trainable={2})
        assert [g is None for g in part] == [True, True, False, True] and torch.equal(part[2], got[2])
        # nothing trainable, or no_grad: nothing is saved and nothing flows
        ps = [p for lin in bg.net for p in (lin.weight, lin.bias)]
        with torch.no_grad():
            quiet = _nb().learned_background(x, enc, bg, sigmoid=sigmoid, precision=0)
        assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, out)
        for p in ps:
            p.requires_grad_(False)
        try:
            frozen = _nb().learned_background(x, enc, bg, sigmoid=sigmoid, precision=0)
            assert not frozen.requires_grad and torch.equal(frozen, out)
        finally:
            for p in ps:
                p.requires_grad_(True)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("layers,hidden,degree", [(2, 64, 6), (1, 16, 6), (3, 32, 8)])
@pytest.mark.parametrize("N", [65, 4097])
def test_f16_against_the_autocast_composition(N, layers, hidden, degree, C):
    enc, bg = _case(C, layers, hidden, degree)
    sigmoid = C == 3
    x = _dirs(N)
    cot = torch.randn(N, C, device=DEV, generator=torch.Generator(DEV).manual_seed(N + C)) * 0.1
    ref, want = bc.oracle_grads(x, enc, bg, sigmoid, cot)
    ps = [p for lin in bg.net for p in (lin.weight, lin.bias)]
    with torch.autocast('cuda', dtype=torch.float16):
        out = _nb().learned_background(x, enc, bg, sigmoid=sigmoid)
        comp = bc.background(x, enc, bg, sigmoid, torch.float32)
    assert out.dtype == torch.float32 and torch.equal(out, out.half().float()) and comp.dtype == torch.float16
    for p in ps:
        p.grad = None
    out.backward(cot)
    got = [p.grad.detach().clone() for p in ps]
    for p in ps:
        p.grad = None
    comp.backward(cot.half())
    cg = [p.grad.detach().clone() for p in ps]
    for p in ps:
        p.grad = None
    en, ec = bc.rel_max(out, ref), bc.rel_max(comp.float(), ref)
    print("learned_background f16 layers=%d hidden=%d C=%d N=%d: forward native %.3g, composition %.3g" % (layers, hidden, C, N, en, ec))
    assert en <= 2 * ec + 1e-7, (en, ec)
    for i, (a, b, w) in enumerate(zip(got, cg, want)):
        ea, eb = bc.rel_max(a, w), bc.rel_max(b, w)
        print("    gradient %d: native %.3g, composition %.3g" % (i, ea, eb))
        assert ea <= 2 * eb + 1e-7, (i, ea, eb)
    # the explicit precision is the same launch
    with torch.no_grad():
        assert torch.equal(_nb().learned_background(x, enc, bg, sigmoid=sigmoid, precision=1), out)


@pytest.mark.parametrize("precision", [0, 1])
def test_two_runs_give_the_same_bits(precision):
    N = 70000                                                                           # 1094 tiles over 512 workgroups, the last tile partial
    enc, bg = _case(3, 2, 64)
    r = np.random.RandomState(5).randn(N, 3)
    x = _t((r / np.linalg.norm(r, axis=1, keepdims=True)).astype(f32))
    cot = torch.randn(N, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1)) * 0.01
    o1, g1 = _native_grads(x, enc, bg, True, cot, precision)
    o2, g2 = _native_grads(x, enc, bg, True, cot, precision)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    assert all(bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0 for a in g1)
    if precision == 0:
        _, want = bc.oracle_grads(x, enc, bg, True, cot)
        assert max(bc.rel_l2(a, b) for a, b in zip(g1, want)) <= bc.F32_BWD


# --------------------------------------------------------------------------------------------------------------------------------------
# 6. render_view
# --------------------------------------------------------------------------------------------------------------------------------------
H = W = 16
BOUND, GRID = 1.0, 16


def _nerf_cfg(**kw):
    from dreamwaltz_g_amd import configs
    c = configs.NeRFConfig(bound=BOUND, grid_size=GRID, num_levels=4, desired_resolution=128, density_prior='gaussian', bg_mode='nerf', lr=1e-3,
                           bg_lr=1e-3, lambda_opacity=5e-3, lambda_entropy=1e-3, lambda_emptiness=0.05)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _network(cfg, seed=0):
    """A BackgroundNeRFNetwork with non-trivial parameters and the occupancy bits of the (1, 16, ., 1) scene."""
    from dreamwaltz_g_amd import nerf_model
    net = nerf_model.build_nerf_network(cfg)
    assert type(net) is nerf_model.BackgroundNeRFNetwork
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.encoder.embeddings.copy_((torch.rand(net.encoder.embeddings.shape, generator=g) * 2 - 1) * 0.5)
        for lin in net.sigma_net.net:
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (2.0 / lin.in_features) ** 0.5)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
        for lin in net.bg_net.net:
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (2.0 / lin.in_features) ** 0.5)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
        _, _, bits, bound = rc.make_scene(1, GRID, 5, seed=1)
        assert bound == BOUND
        net.density_bitfield.copy_(torch.from_numpy(bits))
    return net.to(DEV).train()


def _data(h=H, w=W):
    c2w, K = vc.camera(h, w, BOUND)
    return {'c2w': _t(c2w)[None], 'intrinsics': _t(K)[None], 'image_height': h, 'image_width': w, 'body_part': 'full'}


def _bg_params(net):
    return [p for lin in net.bg_net.net for p in (lin.weight, lin.bias)]


def _composed(net, data, noises, train, bg=True, detach_ws=False):
    """render() from the public pieces: view_rays -> run_cuda_native -> learned_background -> view_compose."""
    from dreamwaltz_g_amd import nerf_render, nerf_view
    ro, rd, nears, fars = nerf_view.view_rays(data['c2w'], data['intrinsics'], H, W, net.aabb_train if train else net.aabb_infer)
    res = nerf_render.run_cuda_native(net, train, ro.shape[:-1], ro.view(-1, 3), rd.view(-1, 3), nears, fars, None, 1.0, 'albedo', train, 0, 1024,
                                      1e-4, noises=noises)
    fg = res['image'].reshape(1, H, W, -1)
    ws = res['weights_sum'].reshape(1, H, W, 1)
    image_bg = _nb().learned_background(rd.view(-1, 3), net.encoder_bg, net.bg_net, sigmoid=not net.latent_mode).reshape(fg.shape)
    nchw, _ = nerf_view.view_compose(fg, ws, image_bg, H, W, detach_ws=detach_ws)
    return nchw, image_bg, ws


@pytest.mark.parametrize("variant", ["rgb", "latent", "detach", "at_call"])
def test_render_view_with_the_learned_background(variant):
    from dreamwaltz_g_amd import nerf_view
    latent = variant == "latent"
    cfg = _nerf_cfg(nerf_type='latent' if latent else 'rgb', detach_bg_weights_sum=variant == "detach")
    net = _network(cfg)
    C = 4 if latent else 3
    data = _data()
    noises = _t(tc.noises(H * W, 1))
    G = torch.randn(1, C, H, W, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    kw = dict(bg_mode='nerf') if variant == "at_call" else {}
    ps = _bg_params(net)

    def grads():
        g = [p.grad.detach().clone() for p in ps]
        for p in net.parameters():
            p.grad = None
        return g

    torch.manual_seed(0)
    out = nerf_view.render_view(net, data, shading='albedo', noises=noises, **kw)
    (out['image_nchw'] * G).sum().backward()
    g_native = grads()
    net.local_step = 0
    torch.manual_seed(0)
    nchw, image_bg, ws = _composed(net, data, noises, True, detach_ws=variant == "detach")
    (nchw * G).sum().backward()
    g_comp = grads()
    assert float(ws.detach().max()) > 0.5 and int((ws == 0).sum()) > 0                   # the view sees the body, and misses it somewhere
    assert torch.equal(out['image_nchw'], nchw) and torch.equal(out['image'], nchw.permute(0, 2, 3, 1))
    assert tuple(out['image_bg'].shape) == (1, H, W, C) == tuple(out['image_fg'].shape) and torch.equal(out['image_bg'], image_bg)
    assert out['image_bg'].dtype == torch.float32
    for a, b in zip(g_native, g_comp):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    # evaluation: the one-launch render under the same background
    net.eval()
    with torch.no_grad():
        ev = nerf_view.render_view(net, data, **kw)
        nchw_e, bg_e, _ = _composed(net, data, None, False)
    assert torch.equal(ev['image_nchw'], nchw_e) and torch.equal(ev['image_bg'], bg_e) and tuple(ev['image_bg'].shape) == (1, H, W, C)
    assert torch.equal(bg_e, image_bg.detach())                                          # the background does not depend on the mode
    net.train()
    if variant == "rgb":
        # shading 'normal' mixes no background: bg_net takes no part
        light_d = _t(np.array([0.3, -0.5, 0.8], f32) / np.linalg.norm([0.3, -0.5, 0.8]).astype(f32))
        out = nerf_view.render_view(net, data, shading='normal', noises=noises, light_d=light_d)
        assert 'image_bg' not in out and tuple(out['image_nchw'].shape) == (1, 3, H, W)
        (out['image_nchw'] * G).sum().backward()
        assert all(p.grad is None for p in ps) and net.sigma_net.net[0].weight.grad is not None
        # the other modes stay available on this network, and rand_bg_prob = 1 turns the learned one gray with one host draw
        net.rand_bg_prob = 1.0
        random.seed(3)
        gray = nerf_view.render_view(net, data, noises=noises)
        state = random.getstate()
        random.seed(3)
        random.random()
        assert random.getstate() == state and bool((gray['image_bg'] == 0.5).all())
        net.rand_bg_prob = None
        white = nerf_view.render_view(net, data, bg_mode='white', noises=noises)
        assert bool((white['image_bg'] == 1.0).all())


# --------------------------------------------------------------------------------------------------------------------------------------
# 7. the step
# --------------------------------------------------------------------------------------------------------------------------------------
class _StubGuidance:
    """loss = sum(image * G) with a fixed seeded G (tests/test_nerf_step_gpu.py's stand-in); non-finite on the steps in bad_steps."""

    def __init__(self, scale=1.0, bad_steps=()):
        self.G = _t(np.random.RandomState(9).randn(1, 3, H, W).astype(f32)) * scale
        self.bad_steps = set(bad_steps)

    def __call__(self, inputs, text_embeds_dict=None, train_step=0, max_iteration=1, **kwargs):
        G = torch.full_like(self.G, float("inf")) if train_step in self.bad_steps else self.G
        return {"diffusion_loss": (inputs * G).sum().reshape(1)}


def _trainer(fp16=False, diffusion=None, **nerf_kw):
    from dreamwaltz_g_amd import configs, nerf_trainer
    cfg = configs.TrainConfig()
    cfg.stage, cfg.device = 'nerf', DEV
    cfg.nerf = _nerf_cfg(**nerf_kw)
    cfg.prompt.text_augmentation = False
    cfg.optim.iters = 100
    cfg.optim.fp16 = fp16
    net = _network(cfg.nerf)
    opts, _ = net.get_optimizer(cfg.nerf)
    text = {'pos': torch.zeros(1, 77, 8, device=DEV)}
    return nerf_trainer.NeRFSDSTrainer(cfg, net, diffusion or _StubGuidance(), opts, text_embeds_dict=text, use_controlnet=False)


def _group(tr, name):
    return [pg for pg in tr.optimizers['nerf'].param_groups if pg['name'] == name][0]


def _snapshot(tr):
    net = tr.model
    return {"bg": [p.detach().clone() for p in _bg_params(net)], "emb": net.encoder.embeddings.detach().clone(),
            "w0": net.sigma_net.net[0].weight.detach().clone()}


def _bg_moments(tr):
    pg, b = _group(tr, 'bg_net'), tr.optimizers.buffers
    return b.m[pg['start']:pg['end']].clone(), b.v[pg['start']:pg['end']].clone()


def test_the_step_moves_bg_net_and_rand_bg_prob_leaves_it_alone():
    torch.manual_seed(0)
    tr = _trainer()
    data = _data()
    before = _snapshot(tr)
    for k in range(2):
        loss, ro, _, _ = tr.train_step(data, render_kwargs=dict(noises=_t(tc.noises(H * W, k))))
        assert bool(torch.isfinite(loss).all()) and tuple(ro['image_bg'].shape) == (1, H, W, 3)
    after = _snapshot(tr)
    assert all(not torch.equal(a, b) for a, b in zip(after["bg"], before["bg"]))
    assert not torch.equal(after["emb"], before["emb"]) and not torch.equal(after["w0"], before["w0"])
    assert [_group(tr, n).get('t', 0) for n in ('encoder', 'sigma_net', 'bg_net')] == [2, 2, 2]
    assert all(tr.optimizers.buffers.owns_grad(p) for p in _bg_params(tr.model))         # autograd wrote the flat buffer's slices
    m, v = _bg_moments(tr)
    assert float(m.abs().max()) > 0 and float(v.max()) > 0

    # every step turned gray: bg_net sits out -- parameters, moments and step count -- while the field steps
    torch.manual_seed(0)
    tr = _trainer(rand_bg_prob=1.0)
    before = _snapshot(tr)
    for k in range(2):
        _, ro, _, _ = tr.train_step(data, render_kwargs=dict(noises=_t(tc.noises(H * W, k))))
        assert bool((ro['image_bg'] == 0.5).all())
    after = _snapshot(tr)
    assert all(torch.equal(a, b) for a, b in zip(after["bg"], before["bg"]))
    assert not torch.equal(after["emb"], before["emb"]) and not torch.equal(after["w0"], before["w0"])
    assert [_group(tr, n).get('t', 0) for n in ('encoder', 'sigma_net', 'bg_net')] == [2, 2, 0]
    m, v = _bg_moments(tr)
    assert float(m.abs().max()) == 0 and float(v.abs().max()) == 0


def test_the_fp16_step_takes_the_same_route_and_skips_on_inf():
    # the image gradient is small enough that 65536 * G stays inside fp16 where autograd hands the background a half gradient
    torch.manual_seed(0)
    tr = _trainer(fp16=True, diffusion=_StubGuidance(scale=1e-2, bad_steps={2}))
    data = _data()
    before = _snapshot(tr)
    _, ro, _, _ = tr.train_step(data, render_kwargs=dict(noises=_t(tc.noises(H * W, 0))))
    bg = ro['image_bg']
    assert bg.dtype == torch.float32 and torch.equal(bg, bg.half().float()) and tuple(bg.shape) == (1, H, W, 3)   # the f16 kernel ran
    mid = _snapshot(tr)
    assert all(not torch.equal(a, b) for a, b in zip(mid["bg"], before["bg"])) and not torch.equal(mid["emb"], before["emb"])
    assert tr.optimizers['nerf'].device_step_counts() == [1, 1, 1, 1]
    scale = tr.scaler.get_scale()
    tr.train_step(data, render_kwargs=dict(noises=_t(tc.noises(H * W, 1))))                 # trainer step 2: an Inf in the gradient
    after = _snapshot(tr)
    assert all(torch.equal(a, b) for a, b in zip(after["bg"], mid["bg"])) and torch.equal(after["emb"], mid["emb"])
    assert tr.optimizers['nerf'].device_step_counts() == [1, 1, 1, 1] and tr.scaler.get_scale() == scale / 2


# --------------------------------------------------------------------------------------------------------------------------------------
# 8. binding a reference-shaped network
# --------------------------------------------------------------------------------------------------------------------------------------
class _NeRFNetwork(rc._NeRFNetwork):
    """The reference-shaped stand-in of the render tests (it carries the reference's class name: the binding goes by it) with a render()
    of its own, as a reference _NeRFNetwork has."""

    def render(self, data, shading='albedo', bg_mode=None, staged=False, **kwargs):
        return ("orig", shading, bg_mode, staged)


def _ref_network(with_bg):
    from dreamwaltz_g_amd import nerf
    src = tc.make_network(GRID, BOUND)
    net = _NeRFNetwork(src.encoder, grid_size=GRID, bound=BOUND, density_activation='exp', density_prior='gaussian', latent_mode=False,
                       additional_dim_size=0)
    net.sigma_net.load_state_dict(src.sigma_net.state_dict())
    with torch.no_grad():
        net.sigma_scale.copy_(src.sigma_scale)
    _, _, bits, _ = rc.make_scene(1, GRID, 5, seed=1)
    if with_bg:
        net.encoder_bg, net.bg_net = bc.make_bg(C=3, layers=2, hidden=64, seed=4)
    else:
        net.bg_net = None
    net = net.to(DEV)
    net.density_bitfield = _t(bits)
    net.bg_mode, net.rand_bg_prob, net.dmtet = 'nerf', None, False
    net.bg_colors = {'white': torch.tensor([1.0, 1.0, 1.0]), 'black': torch.tensor([0.0, 0.0, 0.0]), 'gray': torch.tensor([0.5, 0.5, 0.5])}
    net.opt.detach_bg_weights_sum = False
    assert nerf.bind_nerf_network(net, shaded_render=True, train_render='shaded') is None
    assert nerf.bind_nerf_view(net) is None
    return net.train()


def test_a_bound_reference_network_renders_the_learned_background_natively():
    from dreamwaltz_g_amd import nerf_view
    data = _data()
    data.pop('body_part')
    net = _ref_network(True)
    assert nerf_view.covered_view(net, data) and nerf_view.covered_view(net, data, bg_mode='nerf')
    net.eval()
    with torch.no_grad():
        got = net.render(data)
        want = nerf_view.render_view(net, data)
    assert isinstance(got, dict) and torch.equal(got['image_nchw'], want['image_nchw']) and torch.equal(got['image_bg'], want['image_bg'])
    assert float(got['image_bg'].min()) > 0 and float(got['image_bg'].max()) < 1 and float(got['image_bg'].std()) > 0
    net.train()
    noises = _t(tc.noises(H * W, 1))
    torch.manual_seed(0)
    a = net.render(data)
    net.local_step = 0
    torch.manual_seed(0)
    b = nerf_view.render_view(net, data)
    assert torch.equal(a['image_nchw'], b['image_nchw']) and a['image_nchw'].requires_grad
    # without bg_net the call goes to the original render
    bare = _ref_network(False)
    assert not nerf_view.covered_view(bare, data)
    assert bare.render(data) == ("orig", 'albedo', None, False)
    assert bare.render(data, bg_mode='gray') != ("orig", 'albedo', 'gray', False)       # ... and only that one does
