"""GPU tests of the shaded training render (boundary B19: dreamwaltz_g_amd.nerf_render.render_rays_train with shading 'normal' /
'textureless' / 'lambertian'; csrc/nerf_field.hip k_nf_fwd_fd and the templated k_nf_bwd, csrc/nerf_train.hip's shade kernels over
csrc/shade_math.h) against THE COMPOSITION it replaces, with the same noises and light: raymarch.march_rays_train ->
nerf_shading_cases._NeRFNetwork.forward over the fused field (seven launches, the torch statements of the normal and the shading) ->
raymarch.composite_rays_train, and torch autograd through all of it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dreamwaltz_g_amd import _lib, nerf, nerf_render, pointcloud, raymarch
from tests import nerf_field_cases as nc
from tests import nerf_render_cases as rc
from tests import nerf_shade_train_cases as stc
from tests import nerf_shading_cases as sc
from tests import nerf_train_cases as tc

pytestmark = pytest.mark.gpu

SEED = {n: s for _, _, n, s in tc.SCENES}
GRID = {n: (C, H) for C, H, n, _ in tc.SCENES}
# (shading, f16, latent): every mode for 'normal'; the lambert shadings are f32 only and 'lambertian' is rgb only
CASES = [pytest.param('normal', False, False, id="normal-f32-rgb"), pytest.param('normal', False, True, id="normal-f32-latent"),
         pytest.param('normal', True, False, id="normal-f16-rgb"), pytest.param('normal', True, True, id="normal-f16-latent"),
         pytest.param('textureless', False, False, id="textureless-f32-rgb"), pytest.param('textureless', False, True, id="textureless-f32-latent"),
         pytest.param('lambertian', False, False, id="lambertian-f32-rgb")]
MODES = [pytest.param(False, False, id="f32-rgb"), pytest.param(False, True, id="f32-latent"), pytest.param(True, False, id="f16-rgb"),
         pytest.param(True, True, id="f16-latent")]
EPS = stc.EPS


class _Case:
    pass


def _params(net):
    out = {'embeddings': net.encoder.embeddings}
    for l, lin in enumerate(net.sigma_net.net):
        out['w%d' % l], out['b%d' % l] = lin.weight, lin.bias
    return out


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(n, f16, latent, kind="scene"):
    """A scene on the device, its network (the field bound to the fused kernels, as a bound user's composition runs it), noises, light
    and seeded upstream gradients; the compositions are added once per shading and left unchanged."""
    c = _Case()
    c.max_steps = tc.MAX_STEPS
    if kind == "faces":
        o, d, c.face, bits, bound, noises = stc.face_scene()
        C, H, c.max_steps = 1, 16, 64
    else:
        C, H = GRID[n]
        o, d, bits, bound = rc.make_scene(C, H, n, seed=SEED[n])
        noises = tc.noises(n, SEED[n])
    n = len(o)
    c.n, c.f16, c.latent, c.C, c.H, c.bound, c.kind = n, f16, latent, C, H, bound, kind
    c.ch = 4 if latent else 3
    c.net = (stc.flat_network(H, bound, latent) if kind == "flat" else sc.make_shading_network(H, bound, latent=latent)).cuda()
    with torch.no_grad():
        c.net.density_bitfield.copy_(torch.from_numpy(bits))
    assert nerf.bind_nerf_network(c.net) is None
    c.prior = 'none' if kind == "flat" else 'gaussian'
    c.rays_o, c.rays_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    c.nears, c.fars = raymarch.near_far_from_aabb(c.rays_o, c.rays_d, c.net.aabb_train)
    c.noises = torch.from_numpy(noises).cuda()
    c.light = torch.from_numpy(stc.LIGHT).cuda()
    g = torch.Generator().manual_seed(2000 + n)
    c.g_ws, c.g_depth = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    c.g_image = torch.randn(n, c.ch, generator=g).cuda()
    c.composed = {}
    return c


def _field_kw(c):
    return dict(density_activation='exp', density_prior=c.prior, albedo_sigmoid=not c.latent)


def _composition(c, shading):
    if shading not in c.composed:
        net = c.net
        r = {}
        with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
            xyzs, dirs, ts, rays = raymarch.march_rays_train(c.rays_o, c.rays_d, c.bound, net.density_bitfield, c.C, c.H, c.nears, c.fars,
                                                             True, 0, c.max_steps, noises=c.noises)
            sigmas, color = net(xyzs, dirs, c.light, ratio=stc.AMBIENT, shading=shading)
            rgbs = color.float()
            weights, ws, depth, image = raymarch.composite_rays_train(sigmas, rgbs, ts, rays, tc.T_THRESH)
        names = list(_params(net))
        grads = torch.autograd.grad([ws, depth, image], [_params(net)[k] for k in names] + [sigmas, rgbs], [c.g_ws, c.g_depth, c.g_image])
        r["grads"] = dict(zip(names, grads[:len(names)]))
        r["grad_sigmas"], r["grad_rgbs"] = grads[-2], grads[-1]
        r.update(M=xyzs.shape[0], xyzs=xyzs, ts=ts, rays=rays, sigmas=sigmas.detach(), rgbs=rgbs.detach(), weights=weights.detach(),
                 out=(ws.detach(), depth.detach(), image.detach()))
        c.composed[shading] = r
    return c.composed[shading]


def _native(c, shading, backward=True, **kw):
    net = c.net
    debug = {}
    args = dict(noises=c.noises, max_steps=c.max_steps, T_thresh=tc.T_THRESH, return_weights=True, return_sigmas=True, return_stats=True,
                _debug=debug, shading=shading, light_d=c.light, ambient_ratio=stc.AMBIENT)
    args.update(kw)
    with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
        ws, depth, image, weights, sigmas, stats = nerf_render.render_rays_train(
            c.rays_o, c.rays_d, c.nears, c.fars, net.density_bitfield, c.C, c.H, net.encoder, net.sigma_net, net.sigma_scale, c.bound,
            **_field_kw(c), **args)
    r = dict(out=(ws.detach(), depth.detach(), image.detach()), weights=weights, sigmas=sigmas, stats=stats, debug=debug)
    if backward and ws.requires_grad:
        names = list(_params(net))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                  # the backward makes no host read
        try:
            grads = torch.autograd.grad([ws, depth, image], [_params(net)[k] for k in names], [c.g_ws, c.g_depth, c.g_image])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        r["grads"] = dict(zip(names, grads))
    return r


def _live_rows(rays, rays_live):
    live = rays_live[:, 1].long()
    ray = torch.repeat_interleave(torch.arange(len(live), device=live.device), live)
    r = torch.arange(int(live.sum()), device=live.device) - rays_live[:, 0].long()[ray]
    return rays[:, 0].long()[ray] + r, ray


def _spec(net, f16, prior='gaussian', latent=False, bound=None):
    spec, emb, ss, wb = pointcloud.field_spec(net.encoder, net.sigma_net, net.sigma_scale, net.bound if bound is None else bound, 'exp', prior,
                                              not latent, int(f16))
    return spec, spec.desc(emb, ss, wb), (emb, ss, wb)


def _forward_fd(net, x, f16, prior='gaussian', latent=False, bound=None):
    spec, d, keep = _spec(net, f16, prior, latent, bound)
    M = x.shape[0]
    sigma = torch.full((M,), -1.0, device="cuda")
    albedo = torch.full((M, spec.out_dim - 1), -1.0, dtype=torch.float16 if f16 else torch.float32, device="cuda")
    sigma_fd = torch.full((M, 6), -1.0, device="cuda")
    _lib.check(_lib.lib().dwg_nerf_field_forward_fd(ctypes.byref(d), _lib.ptr(x), M, ctypes.c_float(EPS), _lib.ptr(sigma), _lib.ptr(albedo),
                                                    _lib.ptr(sigma_fd), _stream()), "dwg_nerf_field_forward_fd")
    return sigma, albedo, sigma_fd


def _torch_shifted(x, bound):
    """The six point sets exactly as _NeRFNetwork.normal makes them."""
    out = []
    for a in range(3):
        for sign in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[a] = sign * EPS
            out.append((x + torch.tensor([v], device=x.device)).clamp(-bound, bound))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. forward pieces
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16,latent", MODES)
@pytest.mark.parametrize("M", [1, 63, 64, 65, None])
def test_forward_fd_equals_the_field_at_the_seven_point_sets(M, f16, latent):
    """sigma, albedo and the six columns of sigma_fd are torch.equal to dwg_nerf_field_forward at x and at the six torch-shifted point
    sets; M around the 64-point tile and the 1000-ray scene's whole march (84 333 points, more than one tile per workgroup)."""
    c = _case(1000, f16, latent)
    x = _composition(c, 'normal')["xyzs"]
    x = x if M is None else x[5000:5000 + M].contiguous()
    sigma, albedo, sigma_fd = _forward_fd(c.net, x, f16, latent=latent)
    kw = dict(_field_kw(c), precision=int(f16))
    with torch.no_grad():
        s0, a0 = nerf.nerf_field(x, c.net.encoder, c.net.sigma_net, c.net.sigma_scale, c.bound, **kw)
        assert torch.equal(sigma, s0) and torch.equal(albedo, a0) and albedo.dtype == a0.dtype
        for s, p in enumerate(_torch_shifted(x, c.bound)):
            assert torch.equal(sigma_fd[:, s], nerf.nerf_field(p, c.net.encoder, c.net.sigma_net, c.net.sigma_scale, c.bound, **kw)[0]), s
    if M is None:
        assert int((sigma_fd[:, 0] != sigma_fd[:, 1]).sum()) > 0.99 * x.shape[0]


@pytest.mark.parametrize("shading,f16,latent", CASES)
def test_shade_forward_against_the_compositions_colours(shading, f16, latent):
    """dwg_nerf_train_shade_forward over all samples of the 1000-ray scene against the colours torch computed in the composition: within
    16 ulps of max(1, max |rgb|) (nerf_shading_cases.compare's per-sample figure); a latent colour's fourth channel is exactly 0."""
    c = _case(1000, f16, latent)
    comp = _composition(c, shading)
    sigma, albedo, sigma_fd = _forward_fd(c.net, comp["xyzs"], f16, latent=latent)
    M = comp["M"]
    rgbs = torch.full((M, c.ch), -1.0, device="cuda")
    _lib.check(_lib.lib().dwg_nerf_train_shade_forward(
        nerf_render.SHADINGS[shading], _lib.ptr(sigma_fd), _lib.ptr(albedo) if shading == 'lambertian' else None, int(f16), _lib.ptr(c.light),
        ctypes.c_float(stc.AMBIENT), ctypes.c_float(EPS), M, c.ch, _lib.ptr(rgbs), _stream()), "dwg_nerf_train_shade_forward")
    scale = max(1.0, float(comp["rgbs"].abs().max()))
    err = float((rgbs - comp["rgbs"]).abs().max())
    print("shade_forward %s: max error %.3g ulps of %g" % (shading, err / (rc.ULP * scale), scale))
    assert err <= 16 * rc.ULP * scale
    if latent:
        assert int(rgbs[:, 3].count_nonzero()) == 0
    assert float(rgbs[:, :3].std()) > 0.01


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the seven-point-set field backward alone
# ----------------------------------------------------------------------------------------------------------------------------------
def _grads(emb, wb, fill):
    grads = {'embeddings': torch.zeros_like(emb)}
    for l in range(len(wb) // 2):
        grads['w%d' % l], grads['b%d' % l] = torch.full_like(wb[2 * l], fill), torch.full_like(wb[2 * l + 1], fill)
    return grads, [grads[k] for k in grads if k != 'embeddings']


def _backward_fd(net, x, f16, dsigma, dalbedo, dsigma_fd):
    spec, _, (emb, ss, wb) = _spec(net, f16, prior='none', bound=nc.BOUND)
    grads, g_wb = _grads(emb, wb, 7.0)                                      # overwritten
    nerf.field_backward(spec, emb, ss, wb, x, dsigma, dalbedo, grads['embeddings'], None, g_wb, fd=(EPS, dsigma_fd))
    return grads


def _seven_backwards(net, x, f16, dsigma, dalbedo, dsigma_fd):
    spec, _, (emb, ss, wb) = _spec(net, f16, prior='none', bound=nc.BOUND)
    grads, g_wb = _grads(emb, wb, 0.0)
    zero = torch.zeros(x.shape[0], spec.out_dim - 1, dtype=torch.float16 if f16 else torch.float32, device="cuda")
    sets = [(x, dsigma, zero if dalbedo is None else dalbedo)]
    sets += [(p.contiguous(), dsigma_fd[:, s].contiguous(), zero) for s, p in enumerate(_torch_shifted(x, nc.BOUND))]
    for p, ds, da in sets:
        nerf.field_backward(spec, emb, ss, wb, p, ds, da, grads['embeddings'], None, g_wb, accumulate=1)
    return grads


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("M,with_albedo", [(65, True), (1000, False), (4099, True), ((1 << 20) + 65, True)])
def test_backward_fd_against_seven_field_backwards(M, with_albedo, f16):
    """dwg_nerf_field_backward_fd against seven dwg_nerf_field_backward calls (accumulate = 1) on the torch-shifted points with seeded
    dsigma, dalbedo and dsigma_fd: the same per-row bits in another summation order, so relative L2 <= 1e-4 (nerf_train_cases.F32_BWD)
    for the table and every weight and bias; two runs are bit-identical.  2^20 + 65 points cross the chunk of 2^20: the second chunk's
    seven launches add to the partials of the first (`first` only on the very first launch).  Without dalbedo the reference gets zeros.
    Points include the box's faces (nerf_field_cases.make_points), where the shift is clamped."""
    net = nc.make_network().cuda()
    x = torch.from_numpy(nc.make_points(M, seed=M % 1000)).cuda()
    g = torch.Generator().manual_seed(M)
    dsigma, dsigma_fd = torch.randn(M, generator=g).cuda(), torch.randn(M, 6, generator=g).cuda()
    dalbedo = torch.randn(M, 3, generator=g).cuda().to(torch.float16 if f16 else torch.float32) if with_albedo else None
    got = _backward_fd(net, x, f16, dsigma, dalbedo, dsigma_fd)
    again = _backward_fd(net, x, f16, dsigma, dalbedo, dsigma_fd)
    want = _seven_backwards(net, x, f16, dsigma, dalbedo, dsigma_fd)
    err = {k: nc.rel_l2(got[k], want[k]) for k in want}
    print("backward_fd M %d: relative L2 %s" % (M, err))
    for k in want:
        assert torch.equal(got[k], again[k]), k
        assert float(want[k].abs().max()) > 0 and err[k] <= tc.F32_BWD, (k, err[k])


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. end to end against the composition
# ----------------------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _tolerance(shading, f16, latent):
    """Per parameter, from the 5-ray scene: the float64 oracle linearised at the device's own fp32 sigma_fd, sigmas and albedo
    (nerf_shade_train_cases.oracle_grads), the composition's and the native path's relative L2 from it, and the bound
    max(F32_BWD, 4 x the composition's distance)."""
    c = _case(5, f16, latent)
    comp, nat = _composition(c, shading), _native(c, shading)
    dbg = nat["debug"]
    Ml = dbg["xyzs_live"].shape[0]
    albedo = _np(dbg["albedo_live"]) if dbg["albedo_live"].shape[0] else np.zeros((Ml, c.ch), np.float32)
    oracle = stc.oracle_grads(c.net, shading, _np(dbg["xyzs_live"]), _np(dbg["ts_live"]), _np(dbg["sigmas_live"]), albedo, _np(dbg["sigma_fd_live"]),
                              dbg["rays_live"].cpu().numpy(), _np(c.g_ws), _np(c.g_depth), _np(c.g_image), stc.LIGHT, c.bound, f16=f16,
                              latent=latent)
    dist_comp = {k: nc.rel_l2(comp["grads"][k].double().cpu(), oracle[k]) for k in oracle}
    dist_nat = {k: nc.rel_l2(nat["grads"][k].double().cpu(), oracle[k]) for k in oracle}
    tol = {k: max(tc.F32_BWD, 4 * dist_comp[k]) for k in oracle}
    print("5-ray oracle %s f16=%s latent=%s: composition %s native %s" % (shading, f16, latent, dist_comp, dist_nat))
    return tol, dist_comp, dist_nat


@pytest.mark.parametrize("shading,f16,latent", CASES)
@pytest.mark.parametrize("n", [5, 1000, 3000])
def test_forward_and_gradients_against_the_composition(n, shading, f16, latent):
    """One native forward + backward per case against the composition.

    FORWARD, SAME BITS: weights_sum, depth, weights, sigmas and live are torch.equal (shading touches no geometry; live against the
    'albedo' call of render_rays_train).  IMAGE: per ray within (S + 2 + 16) 2^-23 max(1, max |rgbs|), S the ray's live samples
    (nerf_shading_cases.compare's bound).  The six shifted densities kept for the backward are dwg_nerf_field_forward_fd's rows.
    CULLED ROWS: the composition's grad_rgbs / grad_sigmas are exactly 0 on every culled row; on the live rows they are torch.equal to
    the native composite backward's only when the colours are (they feed d sigma), so that is not asked.
    PARAMETER GRADIENTS: not bit-equal (the shade backward rounds differently from torch, on top of the sum order).  On the 5-ray scene
    the float64 oracle, linearised at the device's own fp32 sigma_fd / sigmas / albedo, gives the composition's relative L2 per
    parameter; the native path must be within max(1e-4, 4 x that) of the oracle.  At 1000 and 3000 rays native against composition must
    be within the same per-parameter bound.
    FAIRNESS from the device's own values at 1000 and 3000 rays: nerf_train_cases.assert_fair; >= 0.9 of the live samples have a
    non-zero normal; for 'textureless' lit and unlit shares each >= 0.25; borderline rays <= 0.5 %.

    Measured on an MI355X (information; the asserted bound is the rule above; DESIGN section 5n has the table).  Relative L2 from the
    oracle at 5 rays, composition / native: 'normal' f32 5.5e-7 .. 4.0e-6 / 4.6e-7 .. 3.5e-6, 'normal' f16 3.6e-5 .. 2.5e-4 / 3.5e-5 ..
    2.5e-4 (the fp16 operands of the field backward, common to both), 'textureless' 1.4e-6 .. 3.9e-6 / 1.2e-6 .. 4.3e-6, 'lambertian'
    2.5e-6 .. 4.4e-6 / 2.4e-6 .. 4.6e-6: the bound is 1e-4 in f32 and 1.4e-4 .. 1.0e-3 in f16.  Native against composition at 1000 / 3000
    rays: table 2.2e-7 .. 1.2e-5, weights and biases up to 4.5e-5 in f32 and 9.1e-5 in f16.  Image: at most 0.014 of its bound.  Device
    figures: M / M_live as B18's; every live sample has a non-zero finite normal; lit share 0.496 .. 0.507; clamp active on none."""
    c = _case(n, f16, latent)
    comp, nat = _composition(c, shading), _native(c, shading)
    ws, depth, image = nat["out"]
    assert torch.equal(ws, comp["out"][0]) and torch.equal(depth, comp["out"][1])
    assert torch.equal(nat["weights"], comp["weights"]) and torch.equal(nat["sigmas"], comp["sigmas"])
    assert image.shape == (n, c.ch) and not nat["weights"].requires_grad and not nat["sigmas"].requires_grad
    st, dbg = nat["stats"], nat["debug"]
    with torch.autocast("cuda", dtype=torch.float16, enabled=f16), torch.no_grad():
        plain = nerf_render.render_rays_train(c.rays_o, c.rays_d, c.nears, c.fars, c.net.density_bitfield, c.C, c.H, c.net.encoder, c.net.sigma_net,
                                              c.net.sigma_scale, c.bound, **_field_kw(c), noises=c.noises, max_steps=c.max_steps,
                                              T_thresh=tc.T_THRESH, return_stats=True)
    assert torch.equal(st["live"], plain[3]["live"]) and st["M_live"] == plain[3]["M_live"] and st["M"] == comp["M"]
    assert torch.equal(ws, plain[0]) and torch.equal(depth, plain[1])
    live = st["live"].cpu().numpy().astype(np.int64)
    # image
    bound = stc.image_bound(live, float(comp["rgbs"].abs().max()) if comp["M"] else 0.0)
    err = (image.double() - comp["out"][2].double()).abs().max(-1)[0].cpu().numpy()
    print("image: max error / bound %.3g" % float((err / bound).max()))
    assert (err <= bound).all()
    # the rows kept for the backward
    assert torch.equal(dbg["rays"], comp["rays"]) and torch.equal(dbg["rays_live"][:, 1], st["live"])
    rows, owner = _live_rows(dbg["rays"], dbg["rays_live"])
    sigma_full, albedo_full, sigma_fd_full = _forward_fd(c.net, comp["xyzs"], f16, latent=latent)
    assert torch.equal(dbg["sigma_fd_live"], sigma_fd_full[rows]) and torch.equal(dbg["xyzs_live"], comp["xyzs"][rows])
    assert torch.equal(dbg["sigmas_live"], comp["sigmas"][rows]) and torch.equal(dbg["ts_live"], comp["ts"][rows])
    if shading == 'lambertian':
        assert torch.equal(dbg["albedo_live"], albedo_full[rows])
    # culled rows
    culled = torch.ones(comp["M"], dtype=torch.bool, device="cuda")
    culled[rows] = False
    assert int(culled.sum()) == st["M"] - st["M_live"]
    assert int(comp["grad_sigmas"][culled].count_nonzero()) == 0 and int(comp["grad_rgbs"][culled].count_nonzero()) == 0
    assert int(dbg["grad_sigmas_live"].count_nonzero()) > 0 and int(dbg["dsigma_fd_live"].count_nonzero()) > 0
    if latent:
        assert int(comp["grad_rgbs"][:, 3].count_nonzero()) > 0          # the pad's gradient exists and is dropped
    # fairness
    counts = comp["rays"][:, 1].cpu().numpy().astype(np.int64)
    _, margin = tc.stops(_np(comp["sigmas"]), _np(comp["ts"]), counts)
    fig = tc.figures(live, counts, margin)
    sfig = stc.sample_figures(_np(dbg["xyzs_live"]), _np(dbg["sigma_fd_live"]), c.bound)
    print("device figures:", fig, sfig)
    if n >= 1000:
        tc.assert_fair(fig, n)
        assert sfig["nonzero_normal"] >= 0.9 and sfig["non_finite"] == 0, sfig
        if shading == 'textureless':
            assert sfig["lit"] >= 0.25 and sfig["unlit"] >= 0.25, sfig
    # parameter gradients
    tol, dist_comp, dist_nat = _tolerance(shading, f16, latent)
    assert nat["grads"].keys() == comp["grads"].keys() == tol.keys()
    if n == 5:
        for k in tol:
            assert dist_nat[k] <= tol[k], (k, dist_nat[k], dist_comp[k])
    err = {k: nc.rel_l2(nat["grads"][k], comp["grads"][k]) for k in tol}
    print("parameter gradients, native against composition, relative L2:", err)
    for k in tol:
        assert float(comp["grads"][k].abs().max()) > 0, k
        if n >= 1000:
            assert err[k] <= tol[k], (k, err[k], tol[k])


@pytest.mark.parametrize("shading", ['normal', 'textureless'])
def test_crafted_face_rays_reach_the_clamp_of_the_shifted_points(shading):
    """(a): 96 rays just inside the six faces of the box on a dense bitfield, perturbed.  From the device's own live rows the clamp of a
    shifted point is active on at least one live sample of every face (the CPU check gave about 591 per face); results against the
    composition as in the scene test: an unclamped shift leaves the encoder's domain and shows at full scale."""
    c = _case(96, False, False, kind="faces")
    comp, nat = _composition(c, shading), _native(c, shading)
    dbg = nat["debug"]
    rows, owner = _live_rows(dbg["rays"], dbg["rays_live"])
    per_face = stc.face_active(_np(dbg["xyzs_live"]), c.face[owner.cpu().numpy()], c.bound)
    print("live samples with the clamp active per face:", per_face)
    assert (per_face >= 1).all()
    assert torch.equal(nat["out"][0], comp["out"][0]) and torch.equal(nat["out"][1], comp["out"][1])
    live = nat["stats"]["live"].cpu().numpy()
    err = (nat["out"][2].double() - comp["out"][2].double()).abs().max(-1)[0].cpu().numpy()
    assert (err <= stc.image_bound(live, float(comp["rgbs"].abs().max()))).all()
    tol = _tolerance(shading, False, False)[0]
    for k in tol:
        e = nc.rel_l2(nat["grads"][k], comp["grads"][k])
        assert float(comp["grads"][k].abs().max()) > 0 and e <= tol[k], (k, e, tol[k])


@pytest.mark.parametrize("shading", ['normal', 'textureless'])
def test_crafted_flat_field_takes_the_below_clamp_branch_everywhere(shading):
    """(b): prior 'none' and a zeroed density row: the six shifted densities of every live sample are equal, every normal is zero and
    every gradient goes through dn / 1e-10, the reference's huge value.  f32 only: an fp16 field backward cannot hold it."""
    c = _case(5, False, False, kind="flat")
    comp, nat = _composition(c, shading), _native(c, shading)
    sfd = nat["debug"]["sigma_fd_live"]
    assert sfd.shape[0] > 0 and torch.equal(sfd, sfd[:, :1].expand(-1, 6))
    assert float(nat["debug"]["dsigma_fd_live"].abs().max()) > 1e6
    assert torch.equal(nat["out"][0], comp["out"][0]) and torch.equal(nat["out"][2], comp["out"][2])    # the colours are constants
    # the density hangs on the last layer's bias alone (its weight row is zero), so only that layer's weight and bias get a gradient,
    # in both paths; the weight's is the huge one: sum over the shifted points of +-0.5 (dn / 1e-10) / eps times the hidden activations
    tol = _tolerance(shading, False, False)[0]
    last = len(c.net.sigma_net.net) - 1
    for k in tol:
        if k in ('w%d' % last, 'b%d' % last):
            e = nc.rel_l2(nat["grads"][k], comp["grads"][k])
            assert float(comp["grads"][k].abs().max()) > 0 and e <= tol[k], (k, e, tol[k])
        else:
            assert int(comp["grads"][k].count_nonzero()) == 0 and int(nat["grads"][k].count_nonzero()) == 0, k
    assert float(comp["grads"]['w%d' % last][0].abs().max()) > 1e6


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. binding
# ----------------------------------------------------------------------------------------------------------------------------------
def _train_step(net, c, seed, shading, light_d=None):
    net.train()
    net.local_step = 0
    with torch.no_grad():
        net.step_counter.fill_(5)
    torch.cuda.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
        out = net.run_cuda(c.rays_o[None], c.rays_d[None], light_d=light_d, ambient_ratio=stc.AMBIENT, shading=shading, perturb=True,
                           max_steps=tc.MAX_STEPS, T_thresh=tc.T_THRESH)
    after = torch.randn(3, device="cuda")                       # the device generator's next draw: the call consumed it identically
    names = list(_params(net))
    grads = torch.autograd.grad([out["weights_sum"][0], out["depth"][0], out["image"][0]], [_params(net)[k] for k in names],
                                [c.g_ws, c.g_depth, c.g_image])
    net.eval()
    return out, dict(zip(names, grads)), (net.local_step, net.step_counter.clone()), after


@pytest.mark.parametrize("shading,f16", [('normal', False), ('normal', True), ('textureless', False)])
def test_binding(shading, f16):
    """train_render='shaded': a shaded training run_cuda is the native render's (the class method is not reached), with B18's key set,
    the original's step-counter statements and the original's consumption of the device generator (light_d None: the same seed gives
    the same light, seen in the 'textureless' image, and the same next draw).  train_render=True alone, and the lambert shadings under
    autocast, reach the original.  After unbind_nerf_network nothing the binding installed is left."""
    c = _case(1000, f16, False)
    net = c.net
    ro, rd = c.rays_o[None], c.rays_d[None]
    try:
        nerf.unbind_nerf_network(net)
        assert nerf.bind_nerf_network(net, shaded_render=True, train_render=True) is None
        del net.run_calls[:]
        want, want_grads, (step0, counter0), after0 = _train_step(net, c, 21, shading)
        assert net.run_calls == [(True, shading, True)]          # with train_render=True only, a shaded training call is the original's
        nerf.unbind_nerf_network(net)
        assert nerf.bind_nerf_network(net, shaded_render=True, train_render='shaded') is None
        del net.run_calls[:]
        got, got_grads, (step1, counter1), after1 = _train_step(net, c, 21, shading)
        assert net.run_calls == []
        assert set(got) == {"image", "depth", "weights_sum", "mask", "weights", "xyzs", "sigmas", "rgbs"}
        assert torch.equal(after0, after1)
        for k in ("depth", "weights_sum", "mask"):
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
        assert torch.equal(got["weights"], want["weights"]) and torch.equal(got["sigmas"], want["sigmas"])
        assert not got["weights"].requires_grad and not got["sigmas"].requires_grad and got["xyzs"] is None and got["rgbs"] is None
        M = got["sigmas"].shape[0]
        # the image bound with S = the ray's samples that got a weight (its live samples; the run_cuda results carry no counts)
        err = (got["image"][0].detach().double() - want["image"][0].detach().double()).abs().max(-1)[0].cpu().numpy()
        with torch.autocast("cuda", dtype=torch.float16, enabled=f16), torch.no_grad():
            torch.cuda.manual_seed(21)
            torch.randn(3, device="cuda")                        # the call's draws in their order: the light, then the march's noises
            noises = torch.rand(c.n, device="cuda")
            rays = raymarch.march_rays_train(c.rays_o, c.rays_d, c.bound, net.density_bitfield, c.C, c.H, c.nears, c.fars, True, 0, tc.MAX_STEPS,
                                             noises=noises)[3]
        assert int(rays[:, 1].sum()) == M
        assert (err <= stc.image_bound(rays[:, 1].cpu().numpy(), float(want["rgbs"].detach().abs().max()))).all()
        tol = _tolerance(shading, f16, False)[0]
        for k in tol:
            e = nc.rel_l2(got_grads[k], want_grads[k])
            assert e <= tol[k], (k, e, tol[k])
        assert step0 == step1 == 1
        assert counter0[0].tolist() == [0, 0] and counter1[0].tolist() == [M, 0]
        assert torch.equal(counter0[1:], counter1[1:]) and int((counter1[1:] != 5).sum()) == 0
        # the 'albedo' training call is B18's, and evaluation views are B14 / B15's
        net.train()
        with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
            net.run_cuda(ro, rd, max_steps=tc.MAX_STEPS)
            # the lambert shadings under autocast go to the original
            with torch.autocast("cuda", dtype=torch.float16):
                net.run_cuda(ro, rd, light_d=c.light, shading='textureless', max_steps=tc.MAX_STEPS)
        net.eval()
        assert net.run_calls == [(True, 'textureless', False)]
        nerf.unbind_nerf_network(net)
        left = sorted(k for k in net.__dict__ if k.startswith("_dwg_"))
        assert left == ["_dwg_nerf_bound", "_dwg_nerf_unbound"] and not net._dwg_nerf_bound, left
        assert "run_cuda" not in net.__dict__ and "common_forward" not in net.__dict__
    finally:
        net.eval()
        nerf.unbind_nerf_network(net)
        assert nerf.bind_nerf_network(net) is None               # the cached case's state


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. other checks
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shading,f16,latent", CASES)
def test_two_runs_give_the_same_bits(shading, f16, latent):
    c = _case(3000, f16, latent)
    a, b = _native(c, shading), _native(c, shading)
    for x, y in zip(a["out"] + (a["weights"], a["sigmas"], a["stats"]["live"]), b["out"] + (b["weights"], b["sigmas"], b["stats"]["live"])):
        assert torch.equal(x, y)
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("mode", [torch.no_grad, torch.inference_mode])
@pytest.mark.parametrize("shading,f16,latent", CASES[:1] + CASES[3:5] + CASES[6:])
def test_without_grad_nothing_is_gathered_or_saved(shading, f16, latent, mode):
    c = _case(1000, f16, latent)
    want = _native(c, shading, backward=False)
    with mode():
        got = _native(c, shading, backward=False)
    for a, b in zip(got["out"], want["out"]):
        assert torch.equal(a, b) and not a.requires_grad
    assert got["debug"] == {} and want["debug"].keys() >= {"rays", "rays_live", "sigma_fd_live"}
    assert got["stats"]["M_live"] == want["stats"]["M_live"]


def test_refusals_come_before_any_launch():
    c = _case(1000, False, False)
    lat = _case(1000, False, True)
    net = c.net

    def call(cc=c, **kw):
        n = cc.net
        return nerf_render.render_rays_train(cc.rays_o, cc.rays_d, cc.nears, cc.fars, n.density_bitfield, cc.C, cc.H, n.encoder, n.sigma_net,
                                             n.sigma_scale, cc.bound, **_field_kw(cc), noises=cc.noises, **kw)
    with pytest.raises(RuntimeError, match="shading must be one of"):
        call(shading='phong')
    with pytest.raises(RuntimeError, match="latent"):
        call(lat, shading='lambertian', light_d=c.light)
    for shading in ('textureless', 'lambertian'):
        with pytest.raises(RuntimeError, match="light_d"):
            call(shading=shading)
        with pytest.raises(RuntimeError, match="light_d"):
            call(shading=shading, light_d=c.light[:2])
        with pytest.raises(RuntimeError, match="light_d"):
            call(shading=shading, light_d=c.light.cpu())
        with pytest.raises(RuntimeError, match="light_d"):
            call(shading=shading, light_d=c.light.double())
        with pytest.raises(RuntimeError, match="f16"):
            with torch.autocast("cuda", dtype=torch.float16):
                call(shading=shading, light_d=c.light)
    for eps in (0.0, -1e-3, float("nan")):
        with pytest.raises(RuntimeError, match="epsilon"):
            call(shading='normal', epsilon=eps)
    # 'normal' needs no light, and the default arguments are the 'albedo' render's
    a = call(shading='normal')
    b = call()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])
