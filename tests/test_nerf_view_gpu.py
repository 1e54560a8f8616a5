"""GPU tests of the view around the NeRF render (boundary B20, dreamwaltz_g_amd.nerf_view): the ray kernel against the float64
restatement, the reference's golden rays and raymarch.near_far_from_aabb; the compose kernels against the unfused torch statements (bit
for bit where the issue asks for it) and float64; render_view against the composition of the public pieces it replaces.

THE BOUNDS (the issue's).  rays_d: 16 * 2^-24 per component (tests/test_nerf_view_host.py derives it).  sparsity_loss: 2^-23 relative
(evaluated in double, one rounding).  d_weights_sum: (C + 2) * 2^-24 * (sum_c |bg_c d_c| + |sparsity term|) against float64.  Parameter
gradients of render_view against the composition: relative L2 <= F32_BWD = 1e-4 (two orders of the same fp32 sums)."""
import os

import numpy as np
import pytest
import torch

from tests import nerf_train_cases as tc
from tests import nerf_render_cases as rc
from tests import nerf_view_cases as vc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nv():
    from dreamwaltz_g_amd import nerf_view
    return nerf_view


# --------------------------------------------------------------------------------------------------------------------------------------
# rays
# --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 7), (33, 65), (64, 64)])
def test_rays_against_float64_golden_and_near_far(H, W):
    """(5, 7) is less than one workgroup; (33, 65) has a tail workgroup, an odd W and rays that miss the box."""
    from dreamwaltz_g_amd import raymarch
    c2w, K = vc.camera(H, W)
    aabb = torch.tensor([-1., -1, -1, 1, 1, 1], device=DEV)
    ro, rd, nears, fars = _nv().view_rays(_t(c2w)[None], _t(K)[None], H, W, aabb)
    assert tuple(ro.shape) == (1, H * W, 3) and tuple(rd.shape) == (1, H * W, 3) and tuple(nears.shape) == (H * W,)
    o64, d64 = vc.rays(c2w, K, H, W)
    err = np.abs(rd[0].cpu().numpy() - d64).max()
    print("view_rays %dx%d: error / bound %.3g against float64" % (H, W, err / vc.RAY_BOUND))
    assert err <= vc.RAY_BOUND
    assert np.array_equal(ro[0].cpu().numpy(), o64.astype(f32))
    if (H, W) in vc.SIZES:
        g = np.load(os.path.join(HERE, "golden", "nerf_view.npz"))
        tag = "%dx%d" % (H, W)
        assert np.abs(rd[0].cpu().numpy().astype(np.float64) - g["rays_d_" + tag]).max() <= vc.RAY_BOUND
        assert np.array_equal(ro[0].cpu().numpy(), g["rays_o_" + tag])
    n0, f0 = raymarch.near_far_from_aabb(ro[0], rd[0], aabb)
    assert torch.equal(nears, n0) and torch.equal(fars, f0)
    hit = nears < fars
    assert int(hit.sum()) >= 5 and int((~hit).sum()) >= 5, (int(hit.sum()), int((~hit).sum()))
    assert bool((nears[~hit] == torch.finfo(torch.float32).max).all())
    # the one-camera forms [4, 4] and [1, 4, 4] are the same call
    ro2, rd2, n2, f2 = _nv().view_rays(_t(c2w), _t(K), H, W, aabb, min_near=0.2)
    assert torch.equal(rd, rd2) and torch.equal(nears, n2) and torch.equal(fars, f2)


# --------------------------------------------------------------------------------------------------------------------------------------
# compose
# --------------------------------------------------------------------------------------------------------------------------------------
def _inputs(H, W, C, seed=0):
    r = np.random.RandomState(seed)
    N = H * W
    ws = vc.ws_vector() if N == vc.N_WS else r.rand(N).astype(f32)
    return r.randn(N, C).astype(f32), ws, r.randn(C).astype(f32), r.randn(N, C).astype(f32), r.randn(C, N).astype(f32)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("bg_kind", ["none", "constant", "image"])
@pytest.mark.parametrize("H,W", [(5, 7), (33, 65)])
def test_compose_forward(H, W, bg_kind, C):
    fg, ws, bgc, bgi, _ = _inputs(H, W, C)
    tfg, tws = _t(fg).view(1, H, W, C), _t(ws).view(1, H, W, 1)
    bg = {"none": None, "constant": _t(bgc), "image": _t(bgi).view(1, H, W, C)}[bg_kind]
    lambdas = vc.LAMBDAS["all"] + (20.0,)
    image, loss = _nv().view_compose(tfg, tws, bg, H, W, sparsity=lambdas)
    assert tuple(image.shape) == (1, C, H, W) and image.is_contiguous() and tuple(loss.shape) == ()
    want = tfg if bg is None else tfg + (1 - tws) * bg
    assert torch.equal(image, want.permute(0, 3, 1, 2).contiguous())
    l64 = vc.sparsity_loss(ws, lambdas[:3], lambdas[3])
    print("view_compose %dx%d C=%d %s: loss error / bound %.3g" % (H, W, C, bg_kind, abs(float(loss) - l64) / (2.0 ** -23 * abs(l64))))
    assert abs(float(loss) - l64) <= 2.0 ** -23 * abs(l64)
    image2, loss2 = _nv().view_compose(tfg, tws, bg, H, W, sparsity=lambdas)
    assert torch.equal(image, image2) and torch.equal(loss, loss2)
    if bg is None:
        # the 'normal' shading's branch: the channel slice, no mix
        sl, none = _nv().view_compose(tfg, tws, None, H, W, channels_out=3)
        assert none is None and torch.equal(sl, tfg[..., :3].permute(0, 3, 1, 2).contiguous())


@pytest.mark.parametrize("case", sorted(vc.LAMBDAS))
def test_sparsity_loss_cases_and_the_loss_alone(case):
    ws = vc.ws_vector()
    sp = vc.LAMBDAS[case] + (1.0,)
    l64 = vc.sparsity_loss(ws, sp[:3])
    _, loss = _nv().view_compose(None, _t(ws), None, 33, 65, sparsity=sp)
    assert abs(float(loss) - l64) <= 2.0 ** -23 * abs(l64)
    g = np.load(os.path.join(HERE, "golden", "nerf_view.npz"))
    want = float(g["loss_%s_before" % case])
    assert abs(float(loss) - want) <= vc.N_WS * vc.U * abs(want)               # the reference's fp32 mean over N terms


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("bg_kind", ["none", "constant", "image"])
@pytest.mark.parametrize("detach_ws", [False, True])
def test_compose_backward(detach_ws, bg_kind, C):
    H, W = 33, 65
    N = H * W
    fg, ws, bgc, bgi, G = _inputs(H, W, C, seed=1)
    lambdas, k = vc.LAMBDAS["all"] + (20.0,), 0.75
    tG = _t(G).view(1, C, H, W)

    def leaves():
        a, b = _t(fg).view(1, H, W, C).requires_grad_(True), _t(ws).view(1, H, W, 1).requires_grad_(True)
        c = {"none": None, "constant": _t(bgc), "image": _t(bgi).view(1, H, W, C).requires_grad_(True)}[bg_kind]
        return a, b, c

    def native():
        a, b, c = leaves()
        image, loss = _nv().view_compose(a, b, c, H, W, detach_ws=detach_ws, sparsity=lambdas)
        ((image * tG).sum() + k * loss).backward()
        return a.grad, b.grad, (c.grad if bg_kind == "image" else None)
    d_fg, d_ws, d_bg = native()
    # autograd of the unfused statements (without the sparsity loss: its derivative is checked against float64 below)
    a, b, c = leaves()
    mixw = b.detach() if detach_ws else b
    img = a if c is None else a + (1 - mixw) * c
    (img.permute(0, 3, 1, 2).contiguous() * tG).sum().backward()
    assert torch.equal(d_fg, a.grad)
    if bg_kind == "image":
        assert torch.equal(d_bg, c.grad) and torch.equal(d_bg, (1 - b.detach()) * tG.permute(0, 2, 3, 1))
    d_nhwc = G.T.astype(np.float64)
    bg64 = {"none": np.zeros(C), "constant": bgc, "image": bgi}[bg_kind]
    _, mix_ws, _, mag = vc.mix_grads(d_nhwc, ws, bg64, detach_ws=detach_ws or bg_kind == "none")
    sp64 = k * vc.sparsity_grad(ws, lambdas[:3], lambdas[3])
    if detach_ws or bg_kind == "none":
        mag = np.zeros(N)
    bound = (C + 2) * vc.U * (mag + np.abs(sp64))
    err = np.abs(d_ws.reshape(-1).cpu().numpy() - (mix_ws + sp64))
    print("view_compose backward C=%d %s detach=%s: d_weights_sum error / bound %.3g" % (C, bg_kind, detach_ws, (err / bound).max()))
    assert (err <= bound).all()
    d_fg2, d_ws2, d_bg2 = native()
    assert torch.equal(d_fg, d_fg2) and torch.equal(d_ws, d_ws2) and (d_bg is None or torch.equal(d_bg, d_bg2))
    # without a sparsity loss, detach_ws zeroes the mix term exactly
    a, b, c = leaves()
    image, _ = _nv().view_compose(a, b, c, H, W, detach_ws=detach_ws)
    (image * tG).sum().backward()
    if detach_ws or bg_kind == "none":
        assert b.grad is None or bool((b.grad == 0).all())
    else:
        assert bool((b.grad != 0).any())


def test_compose_backward_details():
    """Channels beyond channels_out get a zero gradient; the entropy term passes no gradient where ws is clamped; under no_grad nothing
    is saved."""
    H, W, C = 33, 65, 4
    fg, ws, _, _, G = _inputs(H, W, C, seed=2)
    a, b = _t(fg).view(1, H, W, C).requires_grad_(True), _t(ws).requires_grad_(True)
    image, loss = _nv().view_compose(a, b, None, H, W, channels_out=3, sparsity=vc.LAMBDAS["entropy"] + (1.0,))
    ((image * _t(G[:3]).view(1, 3, H, W)).sum() + loss).backward()
    assert bool((a.grad[..., 3] == 0).all()) and torch.equal(a.grad[..., :3], _t(G[:3]).view(3, H, W).permute(1, 2, 0)[None])
    clamped = (ws.astype(np.float64) < vc.LO) | (ws.astype(np.float64) > vc.HI)
    gws = b.grad.cpu().numpy()
    assert clamped.sum() >= 120 and (gws[clamped] == 0).all() and (gws[~clamped & (ws != 0.5)] != 0).all()
    with torch.no_grad():
        image2, loss2 = _nv().view_compose(a, b, None, H, W, channels_out=3, sparsity=vc.LAMBDAS["entropy"] + (1.0,))
    assert not image2.requires_grad and not loss2.requires_grad and torch.equal(image2, image.detach()) and torch.equal(loss2, loss.detach())


# --------------------------------------------------------------------------------------------------------------------------------------
# render_view against the composition of the public pieces
# --------------------------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _scene_net(C, Hg, seed):
    """The scene's stand-in network on the device, bound with the native renders, with the render state render() reads."""
    from dreamwaltz_g_amd import nerf
    key = (C, Hg, seed)
    if key not in _NETS:
        _, _, bits, bound = rc.make_scene(C, Hg, 5, seed=seed)
        net = tc.make_network(Hg, bound).to(DEV)
        net.density_bitfield = _t(bits)
        net.bg_mode, net.rand_bg_prob, net.dmtet = 'gray', None, False
        net.bg_colors = {'white': torch.tensor([1.0, 1.0, 1.0]), 'black': torch.tensor([0.0, 0.0, 0.0]), 'gray': torch.tensor([0.5, 0.5, 0.5])}
        net.opt.detach_bg_weights_sum = False
        assert nerf.bind_nerf_network(net, shaded_render=True, train_render='shaded') is None
        net.train()
        _NETS[key] = (net, bound)
    return _NETS[key]


def _params(net):
    return [net.encoder.embeddings, net.sigma_scale] + [p for lin in net.sigma_net.net for p in (lin.weight, lin.bias)]


def _torch_sparsity(ws, lambdas, mult):
    """SparsityLoss's statements (core/nerf/nerf_loss.py:17-56) in fp32 torch."""
    lo, le, lm = lambdas
    loss = 0.0
    if lo > 0:
        loss = loss + lo * torch.sqrt((ws ** 2 + 0.01).mean())
    if le > 0:
        al = ws.clamp(1e-6, 1 - 1e-6)
        loss = loss + le * (- al * torch.log2(al) - (1 - al) * torch.log2(1 - al)).mean()
    if lm > 0:
        loss = loss + lm * (10000 * torch.log(1 + 10 * ws).mean())
    return loss * mult


@pytest.mark.parametrize("shading", ['albedo', 'normal'])
@pytest.mark.parametrize("H,W", [(5, 7), (33, 65)])
@pytest.mark.parametrize("scene", [tc.SCENES[0], tc.SCENES[1]])
def test_render_view_against_the_composition(scene, H, W, shading):
    from dreamwaltz_g_amd import nerf_render, raymarch
    C, Hg, _, seed = scene
    net, bound = _scene_net(C, Hg, seed)
    N = H * W
    c2w, K = vc.camera(H, W, bound)
    data = {'c2w': _t(c2w)[None], 'intrinsics': _t(K)[None], 'image_height': H, 'image_width': W}
    noises = _t(tc.noises(N, seed))
    light_d = _t(np.array([0.3, -0.5, 0.8], f32) / np.linalg.norm([0.3, -0.5, 0.8]).astype(f32))
    G = _t(np.random.RandomState(seed).randn(1, 3, H, W).astype(f32))
    sp = vc.LAMBDAS["all"] + (1.0,)
    ps = _params(net)

    for p in ps:
        p.grad = None
    out = _nv().render_view(net, data, shading=shading, noises=noises, light_d=light_d, sparsity=sp)
    ((out['image_nchw'] * G).sum() + out['sparsity_loss']).backward()
    g_native = [None if p.grad is None else p.grad.detach().clone() for p in ps]

    for p in ps:
        p.grad = None
    ro, rd, _, _ = _nv().view_rays(data['c2w'], data['intrinsics'], H, W, net.aabb_train)
    nears, fars = raymarch.near_far_from_aabb(ro[0], rd[0], net.aabb_train)
    ws, depth, image = nerf_render.render_rays_train(
        ro[0], rd[0], nears, fars, net.density_bitfield, net.cascade, net.grid_size, net.encoder, net.sigma_net, net.sigma_scale, net.bound,
        density_activation=net.opt.density_activation, density_prior=net.density_prior_type, albedo_sigmoid=True, perturb=True, noises=noises,
        **({} if shading == 'albedo' else dict(shading=shading, light_d=light_d, ambient_ratio=1.0)))
    image, ws4 = image.reshape(1, H, W, -1), ws.reshape(1, H, W, 1)
    img = image[..., :3] if shading == 'normal' else image + (1 - ws4) * net.bg_colors['gray'].to(image)
    nchw = img.permute(0, 3, 1, 2).contiguous()
    ((nchw * G).sum() + _torch_sparsity(ws4, sp[:3], sp[3])).backward()
    g_comp = [None if p.grad is None else p.grad.detach().clone() for p in ps]

    assert float(ws.detach().max()) > 0.5 and int((ws == 0).sum()) > 0                  # the view sees the body, and misses it somewhere
    assert torch.equal(out['weights_sum'], ws4) and torch.equal(out['depth'], depth.reshape(1, H, W, 1))
    assert torch.equal(out['image'], img) and torch.equal(out['image_nchw'], nchw)
    assert out['image'].permute(0, 3, 1, 2).contiguous().data_ptr() == out['image_nchw'].data_ptr()      # the guidance's copy is a no-op
    assert tuple(out['mask'].shape) == (1, H, W, 1) and out['alpha'] is out['weights_sum']
    assert torch.equal(out['mask'].reshape(-1), nears < fars)
    for k in ('weights', 'sigmas', 'xyzs', 'rgbs'):
        assert k in out
    if shading == 'albedo':
        assert torch.equal(out['image_fg'], image) and tuple(out['image_bg'].shape) == (1, H, W, 3) and bool((out['image_bg'] == 0.5).all())
    else:
        assert 'image_bg' not in out and tuple(out['image'].shape) == (1, H, W, 3)
    worst = 0.0
    assert [a is None for a in g_native] == [b is None for b in g_comp] and sum(a is not None for a in g_native) >= 7
    for a, b in zip(g_native, g_comp):
        if a is None:                                   # sigma_scale under the 'exp' activation: no gradient on either side
            continue
        den = float(b.double().norm())
        assert den > 0
        worst = max(worst, float((a.double() - b.double()).norm()) / den)
    print("render_view %s %dx%d scene %s: parameter gradients relative L2 %.3g (bound %g)" % (shading, H, W, scene, worst, tc.F32_BWD))
    assert worst <= tc.F32_BWD


def test_render_view_backgrounds_and_evaluation():
    """The other background modes keep the reference's draws, the evaluation view runs the one-launch render, and the learned
    background is refused."""
    import random
    C, Hg, _, seed = tc.SCENES[0]
    net, bound = _scene_net(C, Hg, seed)
    H, W = 5, 7
    c2w, K = vc.camera(H, W, bound)
    data = {'c2w': _t(c2w)[None], 'intrinsics': _t(K)[None], 'image_height': H, 'image_width': W}
    noises = _t(tc.noises(H * W, seed))
    base = _nv().render_view(net, data, bg_mode='none', noises=noises)
    assert 'image_bg' not in base and 'image_fg' not in base and torch.equal(base['image'], base['image_nchw'].permute(0, 2, 3, 1))
    fg, ws4 = base['image'], base['weights_sum']
    torch.manual_seed(7)
    u = torch.rand(3)
    torch.manual_seed(7)
    out = _nv().render_view(net, data, bg_mode='uniform', noises=noises)
    assert torch.equal(out['image'], fg + (1 - ws4) * u.to(fg))
    torch.manual_seed(8)
    torch.randn(3, device=DEV)                                                  # run_cuda's light_d draw comes first, as in the reference
    n = torch.randn_like(fg.contiguous())                                       # the reference draws like its contiguous [B, H, W, C] image
    torch.manual_seed(8)
    out = _nv().render_view(net, data, bg_mode='normal', noises=noises)
    assert torch.equal(out['image'], fg + (1 - ws4) * n) and torch.equal(out['image_bg'], n)
    out = _nv().render_view(net, data, bg_mode='zero', noises=noises)
    assert torch.equal(out['image'], fg + (1 - ws4) * torch.zeros_like(fg))
    net.rand_bg_prob = 1.0                                                     # random() < 1 always: gray whatever the mode
    try:
        random.seed(3)
        out = _nv().render_view(net, data, bg_mode='white', noises=noises)
        state = random.getstate()
        random.seed(3)
        random.random()
        assert random.getstate() == state                                     # exactly one host draw
        assert torch.equal(out['image'], fg + (1 - ws4) * 0.5)
    finally:
        net.rand_bg_prob = None
    with pytest.raises(NotImplementedError, match="'nerf' background"):
        _nv().render_view(net, data, bg_mode='nerf')
    net.eval()
    try:
        with torch.no_grad():
            ev = _nv().render_view(net, data)
        assert tuple(ev['image'].shape) == (1, H, W, 3) and 'weights' not in ev
        assert float(ev['weights_sum'].max()) > 0.5
    finally:
        net.train()
