"""GPU parity of the fused NeRF field (boundary B7, dreamwaltz_g_amd.nerf) against the float64 restatement of tests/nerf_field_cases.py,
and of the bound test-local network against its unbound torch composition.  Reads nothing of the reference."""

import numpy as np
import pytest
import torch

from tests import nerf_field_cases as nc

pytestmark = pytest.mark.gpu

# max |err| / max |ref| of sigma and albedo, exact-f32 mode.  Measured up to 2.9e-5 on MI355X: the grid lookup's cell position
# x01 * scale + 0.5 is an fp32 value (fused multiply-add in the kernels, two roundings in the restatement) and at the finest level
# (scale ~ 4096) one ulp of it moves the interpolation weights by 5e-4; the MLP and the epilogue alone stay at the 1e-7 level.
F32_FWD = 5e-5
F32_BWD = 1e-4          # relative L2 of every gradient, exact-f32 mode


def _nerf():
    from dreamwaltz_g_amd import nerf
    return nerf


def _fused(net, x, raw=False, sigmoid=None, mlp_no_grad=False, precision=None):
    nerf = _nerf()
    return nerf.nerf_field(x, net.encoder, net.sigma_net, net.sigma_scale, net.bound, density_activation=net.opt.density_activation,
                           density_prior=net.density_prior_type, albedo_sigmoid=(not net.latent_mode) if sigmoid is None else sigmoid,
                           raw=raw, mlp_no_grad=mlp_no_grad, precision=precision)


def _params(net):
    ps = {'embeddings': net.encoder.embeddings, 'sigma_scale': net.sigma_scale}
    for l, lin in enumerate(net.sigma_net.net):
        ps['w%d' % l], ps['b%d' % l] = lin.weight, lin.bias
    return ps


def _zero_grads(net):
    for p in net.parameters():
        p.grad = None


def _cot(M, W, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, generator=g).cuda(), torch.randn(M, W - 1, generator=g).to(dtype).cuda()


FWD_CASES = [
    # gridtype, interp, act, prior, raw, latent
    ('tiled', 'smoothstep', 'exp', 'none', False, False),
    ('hash', 'smoothstep', 'softplus', 'gaussian', False, False),
    ('tiled', 'linear', 'scaling', 'sqrt', False, False),
    ('hash', 'linear', 'exp', 'gaussian', False, True),
    ('tiled', 'smoothstep', 'softplus', 'none', True, False),
    ('hash', 'smoothstep', 'scaling', 'none', True, True),
]


@pytest.mark.parametrize("gridtype,interp,act,prior,raw,latent", FWD_CASES)
@pytest.mark.parametrize("M", [1, 63, 64, 65, 4097])
def test_f32_forward_matches_float64(gridtype, interp, act, prior, raw, latent, M):
    net = nc.make_network(gridtype=gridtype, interp=interp, density_activation=act, density_prior=prior, latent_mode=latent,
                          additional_dim_size=1 if latent else 0, seed=M, log2_hashmap_size=15 if gridtype == 'hash' else 19).cuda()
    x = nc.make_points(M, seed=M)
    with torch.no_grad():
        s, a = _fused(net, torch.from_numpy(x).cuda(), raw=raw)
    rs, ra, _ = nc.restate(net, x, raw=raw)
    assert s.dtype == torch.float32 and a.dtype == torch.float32 and a.shape == (M, 4 if latent else 3)
    es, ea = nc.rel_err(s, rs), nc.rel_err(a, ra)
    assert es <= F32_FWD and ea <= F32_FWD, (es, ea)


def test_f32_forward_one_million_points():
    net = nc.make_network(seed=7).cuda()
    x = nc.make_points(1 << 20, seed=7)
    with torch.no_grad():
        s, a = _fused(net, torch.from_numpy(x).cuda())
    rows = np.random.RandomState(0).choice(x.shape[0], 4096, replace=False)
    rows[:2] = [0, x.shape[0] - 1]
    rs, ra, _ = nc.restate(net, x[rows])
    assert nc.rel_err(s[rows], rs) <= F32_FWD and nc.rel_err(a[rows], ra) <= F32_FWD


@pytest.mark.parametrize("gridtype,interp,act,prior,latent", [
    ('tiled', 'smoothstep', 'exp', 'none', False),
    ('hash', 'linear', 'scaling', 'gaussian', False),
    ('tiled', 'smoothstep', 'softplus', 'sqrt', True),
])
@pytest.mark.parametrize("M", [65, 4097])
def test_f32_backward_matches_float64_autograd(gridtype, interp, act, prior, latent, M):
    net = nc.make_network(gridtype=gridtype, interp=interp, density_activation=act, density_prior=prior, latent_mode=latent,
                          additional_dim_size=1 if latent else 0, seed=3 + M, log2_hashmap_size=15 if gridtype == 'hash' else 19).cuda()
    x = nc.make_points(M, seed=M + 1)
    W = net.sigma_net.net[-1].out_features
    ds, da = _cot(M, W, M)
    s, a = _fused(net, torch.from_numpy(x).cuda())
    ((s * ds).sum() + (a * da).sum()).backward()
    rs, ra, leaves = nc.restate(net, x)
    ((rs * ds.cpu().double()).sum() + (ra * da.cpu().double()).sum()).backward()
    ps = _params(net)
    for k, leaf in leaves.items():
        if k == 'sigma_scale' and act != 'scaling':
            assert ps[k].grad is None
            continue
        e = nc.rel_l2(ps[k].grad.reshape(leaf.shape), leaf.grad)
        assert e <= F32_BWD, (k, e)


def test_needs_input_grad_combinations():
    net = nc.make_network(density_activation='scaling', seed=11).cuda()
    x = torch.from_numpy(nc.make_points(1000, seed=11)).cuda()
    ds, da = _cot(1000, 4, 1)
    s, a = _fused(net, x)
    ((s * ds).sum() + (a * da).sum()).backward()
    full = {k: p.grad.clone() for k, p in _params(net).items()}
    # mlp_no_grad: sigma_net gets nothing, the table and sigma_scale the same gradients
    _zero_grads(net)
    s, a = _fused(net, x, mlp_no_grad=True)
    ((s * ds).sum() + (a * da).sum()).backward()
    for k, p in _params(net).items():
        if k.startswith(('w', 'b')):
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, full[k]), k
    # frozen table, only layer 1's weight
    _zero_grads(net)
    net.encoder.embeddings.requires_grad_(False)
    net.sigma_scale.requires_grad_(False)
    for n_, p in net.sigma_net.named_parameters():
        p.requires_grad_(n_ == 'net.1.weight')
    s, a = _fused(net, x)
    ((s * ds).sum() + (a * da).sum()).backward()
    for k, p in _params(net).items():
        if k == 'w1':
            assert torch.equal(p.grad, full[k])
        else:
            assert p.grad is None, k


@pytest.mark.parametrize("gridtype,act,prior,latent", [('tiled', 'exp', 'none', False), ('hash', 'softplus', 'gaussian', True),
                                                       ('tiled', 'scaling', 'sqrt', False)])
def test_f16_error_within_twice_the_autocast_composition(gridtype, act, prior, latent):
    M = 8192
    net = nc.make_network(gridtype=gridtype, density_activation=act, density_prior=prior, latent_mode=latent,
                          additional_dim_size=1 if latent else 0, seed=21, log2_hashmap_size=15 if gridtype == 'hash' else 19).cuda()
    x = nc.make_points(M, seed=21)
    xc = torch.from_numpy(x).cuda()
    W = net.sigma_net.net[-1].out_features
    ds, da = _cot(M, W, 5)
    rs, ra, leaves = nc.restate(net, x)
    ((rs * ds.cpu().double()).sum() + (ra * da.cpu().double()).sum()).backward()
    ref_g = {k: v.grad for k, v in leaves.items()}
    out = {}
    for name in ("fused", "composition"):
        _zero_grads(net)
        with torch.autocast("cuda", dtype=torch.float16):
            s, a = _fused(net, xc) if name == "fused" else net.common_forward(xc)
        assert s.dtype == torch.float32 and a.dtype == torch.float16, (name, s.dtype, a.dtype)
        ((s * ds).sum() + (a.float() * da).sum()).backward()
        out[name] = (s.detach(), a.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in _params(net).items()})
    report = {}
    for i, key in enumerate(("sigma", "albedo")):
        ref = rs if i == 0 else ra
        ef, ec = nc.rel_err(out["fused"][i], ref), nc.rel_err(out["composition"][i], ref)
        report[key] = (ef, ec)
        assert ef <= 2 * ec + 1e-7, (key, ef, ec)
    for k, g in ref_g.items():
        if k == 'sigma_scale' and act != 'scaling':
            continue
        gf, gc = out["fused"][2][k], out["composition"][2][k]
        ef, ec = nc.rel_l2(gf.reshape(g.shape), g), nc.rel_l2(gc.reshape(g.shape), g)
        report[k] = (ef, ec)
        assert ef <= 2 * ec + 1e-7, (k, ef, ec)
    print("f16 errors (fused, composition):", report)


@pytest.mark.parametrize("precision", [0, 1])
def test_two_runs_are_bit_identical(precision):
    net = nc.make_network(density_activation='scaling', density_prior='gaussian', seed=31).cuda()
    x = torch.from_numpy(nc.make_points(300000, seed=31)).cuda()
    ds, da = _cot(300000, 4, 9, torch.float16 if precision else torch.float32)
    runs = []
    for _ in range(2):
        _zero_grads(net)
        s, a = _fused(net, x, precision=precision)
        ((s * ds).sum() + (a.float() * da.float()).sum()).backward()
        runs.append([s.detach().clone(), a.detach().clone()] + [p.grad.clone() for p in _params(net).values()])
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_zero_points_returns_empty_outputs():
    net = nc.make_network(seed=1).cuda()
    x = torch.zeros(0, 3, device="cuda")
    s, a = _fused(net, x)
    assert s.shape == (0,) and a.shape == (0, 3)
    (s.sum() + a.sum()).backward()
    assert float(net.encoder.embeddings.grad.abs().sum()) == 0.0


def test_argument_errors_raise_before_launch():
    net = nc.make_network(seed=1).cuda()
    x = torch.from_numpy(nc.make_points(64, seed=1)).cuda()
    with pytest.raises(RuntimeError):
        _fused(net, x.double())
    with pytest.raises(RuntimeError):
        _fused(net, x.t().contiguous().t())
    with pytest.raises(RuntimeError):
        _fused(net, x.cpu())
    with pytest.raises(RuntimeError):
        _fused(net, x.clone().requires_grad_(True))


# ------------------------------------------------------------------------------------------------------------------------------------
# the bound network
# ------------------------------------------------------------------------------------------------------------------------------------
def _pair(**kw):
    a = nc.make_network(**kw).cuda()
    b = nc.make_network(**kw).cuda()
    assert _nerf().bind_nerf_network(b) is None
    return a, b


def _cmp(ua, ba, tol):
    for u, v in zip(ua, ba):
        assert u.dtype == v.dtype and u.shape == v.shape, (u.dtype, v.dtype, u.shape, v.shape)
        e = nc.rel_err(v, u)
        assert e <= tol, e


@pytest.mark.parametrize("act,prior,latent", [('exp', 'none', False), ('scaling', 'gaussian', True)])
def test_bound_network_matches_unbound(act, prior, latent):
    kw = dict(density_activation=act, density_prior=prior, latent_mode=latent, additional_dim_size=1 if latent else 0, seed=41)
    ub, bd = _pair(**kw)
    assert bd._dwg_nerf_bound and "common_forward" in bd.__dict__
    x = torch.from_numpy(nc.make_points(5000, seed=41)).cuda()
    mask = (torch.rand(5000, device="cuda") > 0.3).float()
    with torch.no_grad():
        du, db = ub.density(x), bd.density(x)
        _cmp((du['sigma'], du['albedo']), (db['sigma'], db['albedo']), F32_FWD)
        _cmp(ub.forward(x, x, shading='albedo'), bd.forward(x, x, shading='albedo'), F32_FWD)
        _cmp(ub.common_forward(x, mask=mask), bd.common_forward(x, mask=mask), F32_FWD)
        _cmp(ub.common_forward(x, return_raw=True), bd.common_forward(x, return_raw=True), F32_FWD)
    # local_geometry_forward(mlp_no_grad=True): the table's gradient matches, sigma_net gets none
    W = ub.sigma_net.net[-1].out_features
    ds, da = _cot(5000, W, 2)
    for m in (ub, bd):
        s, a = m.local_geometry_forward(x, mlp_no_grad=True)
        ((s * ds).sum() + (a * da).sum()).backward()
        assert all(p.grad is None for p in m.sigma_net.parameters())
    assert nc.rel_l2(bd.encoder.embeddings.grad, ub.encoder.embeddings.grad) <= F32_BWD
    # under autocast: dtypes as the reference returns them
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for u, v in zip(ub.common_forward(x), bd.common_forward(x)):
            assert u.dtype == v.dtype
        for u, v in zip(ub.local_geometry_forward(x), bd.local_geometry_forward(x)):
            assert u.dtype == v.dtype


def test_bound_network_falls_back_for_x_requiring_grad():
    ub, bd = _pair(seed=43)
    x = torch.from_numpy(nc.make_points(777, seed=43)).cuda()
    xu, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    su, au = ub.common_forward(xu)
    sb, ab = bd.common_forward(xb)
    assert torch.equal(su, sb) and torch.equal(au, ab)
    (su.sum() + au.sum()).backward()
    (sb.sum() + ab.sum()).backward()
    assert torch.equal(xu.grad, xb.grad)


def test_end_to_end_march_field_composite_128():
    """B6 march -> bound field -> B6 composite -> backward at 128^2 on the body grid: loss and parameter gradients match the unbound
    composition."""
    from dreamwaltz_g_amd import raymarch as rm
    from tests import raymarch_cases as rc
    ub, bd = _pair(density_activation='exp', density_prior='gaussian', seed=51)
    C, Hg = 2, 128
    grid, bitfield = rc.make_grid(C, Hg, nc.BOUND, kind="body")
    bitfield = torch.from_numpy(bitfield).cuda()
    rays_o, rays_d = rc.make_cameras(1, 128, 128, seed=51)
    rays_o, rays_d = torch.from_numpy(rays_o).cuda(), torch.from_numpy(rays_d).cuda()
    aabb = torch.tensor([-nc.BOUND] * 3 + [nc.BOUND] * 3, device="cuda")
    nears, fars = rm.near_far_from_aabb(rays_o, rays_d, aabb, 0.05)
    xyzs, dirs, ts, rays = rm.march_rays_train(rays_o, rays_d, nc.BOUND, bitfield, C, Hg, nears, fars, False, 0.0, 1024)
    assert xyzs.shape[0] > 1000
    losses, grads = [], []
    for m in (ub, bd):
        sigma, rgb = m(xyzs, dirs, shading='albedo')
        weights, weights_sum, depth, image = rm.composite_rays_train(sigma, rgb, ts, rays, 1e-4, False)
        loss = (image ** 2).sum() + weights_sum.sum()
        loss.backward()
        losses.append(float(loss))
        grads.append({k: p.grad.clone() for k, p in _params(m).items() if p.grad is not None})
    assert abs(losses[0] - losses[1]) <= 1e-5 * abs(losses[0]), losses
    assert grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert nc.rel_l2(grads[1][k], grads[0][k]) <= F32_BWD, k
