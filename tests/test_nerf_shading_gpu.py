"""GPU tests of the shaded one-launch inference render (boundary B15, dreamwaltz_g_amd.nerf_render with shading 'normal' / 'textureless'
/ 'lambertian', csrc/nerf_field.hip k_nf_render_shaded) against the composition a bound network ran before it:
tests/nerf_shading_cases._NeRFNetwork.run_cuda, the reference's loop of march_rays -> forward (seven launches of the fused field, the
torch statements of the normal and the shading) -> composite_rays over the package's own kernels."""
import functools

import numpy as np
import pytest
import torch

from dreamwaltz_g_amd import nerf, nerf_render, raymarch
from tests import nerf_render_cases as rc
from tests import nerf_shading_cases as sc
from tests import raymarch_cases as rmc

pytestmark = pytest.mark.gpu

SEEDS = {5: 1, 1000: 9, 3000: 3}            # B14's scenes
SHADINGS = ("normal", "textureless", "lambertian")


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(C, H, n, f16, latent, kind="body"):
    """A scene on the device and its network bound with shaded_render; the compositions are computed once per shading and left unchanged."""
    c = _Case()
    if kind == "faces":
        o, d, c.face = sc.face_rays()
        _, bits = rmc.make_grid(C, H, 1.0, "dense")
        bound = 1.0
    else:
        o, d, bits, bound = rc.make_scene(C, H, n, seed=SEEDS[n], kind=kind)
    c.n, c.f16, c.latent, c.C, c.H, c.bound = len(o), f16, latent, C, H, bound
    c.o, c.d, c.bits = o, d, bits
    c.net = sc.make_shading_network(H, bound, latent=latent).cuda().eval()
    with torch.no_grad():
        c.net.density_bitfield.copy_(torch.from_numpy(bits))
    assert nerf.bind_nerf_network(c.net, shaded_render=True) is None
    c.rays_o, c.rays_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    c.nears, c.fars = raymarch.near_far_from_aabb(c.rays_o, c.rays_d, c.net.aabb_infer)
    c.light = c.rays_o[0] / torch.sqrt(torch.sum(c.rays_o[0] * c.rays_o[0]))
    c.composed = {}
    return c


def _composition(c, shading, max_steps=rc.MAX_STEPS):
    """(weights_sum, depth, image), mask, records and trace of the composition for this shading."""
    if shading not in c.composed:
        c.net.record = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
            out = c.net.run_cuda.__wrapped__(c.rays_o[None], c.rays_d[None], light_d=c.light, ambient_ratio=sc.AMBIENT, shading=shading,
                                             max_steps=max_steps, T_thresh=rc.T_THRESH)
        records, c.net.record = c.net.record, None
        c.composed[shading] = (tuple(out[k][0].float().cpu().numpy() for k in ("weights_sum", "depth", "image")), out["mask"][0].cpu().numpy(),
                               records, rc.trace(records, c.n, rc.T_THRESH))
    return c.composed[shading]


def _native(c, shading, max_workgroups=0, max_steps=rc.MAX_STEPS, **kw):
    net = c.net
    args = dict(density_activation='exp', density_prior='gaussian', albedo_sigmoid=not c.latent, max_steps=max_steps, T_thresh=rc.T_THRESH,
                return_counts=True, max_workgroups=max_workgroups, shading=shading, light_d=c.light, ambient_ratio=sc.AMBIENT)
    args.update(kw)
    with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
        return nerf_render.render_rays(c.rays_o, c.rays_d, c.nears, c.fars, net.density_bitfield, net.cascade, net.grid_size, net.encoder,
                                       net.sigma_net, net.sigma_scale, net.bound, **args)


def _parity(c, shading, max_workgroups, max_steps=rc.MAX_STEPS):
    composed, mask, records, tr = _composition(c, shading, max_steps)
    native = tuple(t.cpu().numpy() for t in _native(c, shading, max_workgroups, max_steps))
    assert native[2].shape == (c.n, 4 if c.latent else 3)
    return sc.compare(native, composed, tr, mask, c.fars.cpu().numpy(), records)


SIZES = [(1, 16, 5), (2, 32, 1000), (2, 64, 3000)]
# (shading, f16, latent): f32 for the three shadings, fp16 autocast for 'normal'; latent at 1000 rays for 'normal' and 'textureless'
KINDS = [("normal", False, False), ("textureless", False, False), ("lambertian", False, False), ("normal", True, False)]
LATENT = [("normal", False, True), ("textureless", False, True), ("normal", True, True)]
PARITY = [(C, H, n) + k for (C, H, n) in SIZES for k in KINDS] + [(2, 32, 1000) + k for k in LATENT]


@pytest.mark.parametrize("max_workgroups", [0, 2])
@pytest.mark.parametrize("C,H,n,shading,f16,latent", PARITY)
def test_parity_with_the_composition(C, H, n, shading, f16, latent, max_workgroups):
    """The shaded native render against the composition, by nerf_shading_cases.compare: on non-borderline rays (B14's definition and its
    0.5 % cap) the counts equal the float32 trace's, weights_sum and depth agree within (S + 2) 2^-23 scale and the image within
    (S + 2 + 16) 2^-23 max(1, max |rgbs|); borderline rays by B14's rule.  The 16 is derived in compare()'s docstring.
    ambient_ratio 0.1 (at 1.0 the lambert term is constant), light_d = rays_o[0] normalised.  max_workgroups 2 puts 1000 and 3000 rays
    above slots x workgroups = 512, so every workgroup refills its slots.

    FAIR SCENE (asserted at 1000 and 3000 rays from the composition's own records): B14's assert_fair; of the composited samples at
    least 90 % have a non-zero normal ('normal' cases) and at least 25 % are lit and 25 % unlit ('textureless' cases, whose colour is
    the lambert term itself).  The issue's CPU check at these seeds (float64 field at the seven points of every composited sample)
    gave 19 327 / 18 985 (latent) / 41 254 / 19 composited samples at 1000 / 1000 / 3000 / 5 rays, all with a non-zero normal, and
    47.6 % / 47.4 % / 49.8 % / 10 of 19 lit.

    MEASURED on an MI355X (compare() prints both; information, not a threshold): the largest image error was 0.029 of the bound
    ('normal', latent, 1000 rays); weights_sum, depth and counts were bit-equal to the composition on every ray, and all four outputs on
    646 / 815 / 571 of 1000 rays ('normal' / 'textureless' / 'lambertian', f32), 654 ('normal', f16), 2096 / 2501 / 1862 / 2086 of 3000,
    662 / 839 / 626 of the latent 1000 and 3-4 of 5.  The scene figures were the CPU check's exactly."""
    c = _case(C, H, n, f16, latent)
    composed, mask, records, tr = _composition(c, shading)
    if n >= 1000:
        fair = rc.fairness(tr, c.n)
        print("fair scene:", fair)
        rc.assert_fair(fair, c.n)
        if shading != "lambertian":
            sfair = sc.shading_fairness(records, c.n, shading)
            print("fair shading:", sfair)
            sc.assert_shading_fair(sfair)
    else:
        assert tr["count"].max() < rc.MAX_STEPS
    _parity(c, shading, max_workgroups)


@pytest.mark.parametrize("C,H,n,shading,f16,latent", [p for p in PARITY if p[2] >= 1000])
def test_shading_does_not_touch_geometry(C, H, n, shading, f16, latent):
    """weights_sum, depth and counts of a shaded render are those of the albedo render of the same rays, bit for bit."""
    c = _case(C, H, n, f16, latent)
    ws, dep, _, cnt = _native(c, shading)
    ws0, dep0, _, cnt0 = _native(c, "albedo", light_d=None)
    assert torch.equal(ws, ws0) and torch.equal(dep, dep0) and torch.equal(cnt, cnt0)
    assert int(cnt.sum()) > 0


def test_the_shifted_points_are_clamped_at_the_box_faces():
    """No camera scene reaches the clamp, so: 96 rays on a dense bitfield (C = 1, H = 16, bound 1), 16 parallel to each of the six faces at
    most 5e-4 inside it (nerf_shading_cases.face_rays).  The CPU march (tests/test_nerf_shading_host.py) gives 37 samples on every ray and
    the clamp active on all 3552 of them.  'normal' shading against the composition by the parity rule: an unclamped shift leaves the
    encoder's domain, so that bug shows at full scale."""
    c = _case(1, 16, 96, False, False, kind="faces")
    composed, mask, records, tr = _composition(c, "normal", max_steps=64)
    assert mask.all() and (tr["count"] == 37).all(), (mask.sum(), tr["count"].min(), tr["count"].max())
    fig = _parity(c, "normal", 0, max_steps=64)
    assert fig["borderline"] == 0
    sfair = sc.shading_fairness(records, c.n, "normal")
    assert sfair["samples"] == 96 * 37 and sfair["nonzero_normal"] >= 0.9, sfair


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_two_runs_and_any_number_of_workgroups_give_the_same_bits(f16):
    c = _case(2, 32, 1000, f16, False)
    for shading in ("normal", "lambertian"):
        first = _native(c, shading)
        for mw in (0, 2, 1):
            for a, b in zip(first, _native(c, shading, max_workgroups=mw)):
                assert torch.equal(a, b), (shading, mw)


def _sync_free(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_binding_with_shaded_render_runs_the_native_render():
    c = _case(2, 32, 1000, False, False)
    net = c.net
    ro, rd = c.rays_o[None], c.rays_d[None]
    kw = dict(light_d=c.light, ambient_ratio=sc.AMBIENT, max_steps=rc.MAX_STEPS, T_thresh=rc.T_THRESH)
    net.run_cuda(ro, rd, max_steps=rc.MAX_STEPS)                 # the encoder's offsets are read to the host once, here or earlier
    del net.run_calls[:]
    for shading, f16 in (("normal", False), ("normal", True), ("textureless", False), ("lambertian", False)):
        with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
            want = nerf_render.render_rays(c.rays_o, c.rays_d, c.nears, c.fars, net.density_bitfield, net.cascade, net.grid_size, net.encoder,
                                           net.sigma_net, net.sigma_scale, net.bound, density_activation='exp', density_prior='gaussian',
                                           albedo_sigmoid=True, max_steps=rc.MAX_STEPS, T_thresh=rc.T_THRESH, shading=shading, light_d=c.light,
                                           ambient_ratio=sc.AMBIENT)
            out = _sync_free(lambda: net.run_cuda(ro, rd, shading=shading, **kw))
        assert net.run_calls == [], shading                      # the class method was not reached
        assert out["xyzs"] is None and out["sigmas"] is None and out["rgbs"] is None
        assert out["image"].shape == (1, c.n, 3)
        assert torch.equal(out["weights_sum"][0], want[0]) and torch.equal(out["depth"][0], want[1]) and torch.equal(out["image"][0], want[2])
        assert torch.equal(out["mask"][0], c.nears < c.fars)
    # light_d=None: the draw advances the device generator exactly as the original does, and nothing returns to the host
    for shading in ("normal", "lambertian"):
        torch.cuda.manual_seed(5)
        start = torch.cuda.get_rng_state()
        _sync_free(lambda: net.run_cuda(ro, rd, shading=shading, light_d=None, ambient_ratio=sc.AMBIENT, max_steps=rc.MAX_STEPS))
        after_native = torch.cuda.get_rng_state()
        torch.cuda.manual_seed(5)
        net.run_cuda.__wrapped__(ro, rd, shading=shading, light_d=None, ambient_ratio=sc.AMBIENT, max_steps=rc.MAX_STEPS)
        after_original = torch.cuda.get_rng_state()
        assert torch.equal(after_native, after_original) and not torch.equal(after_native, start)
    # calls the native render does not take
    del net.run_calls[:]
    with torch.autocast("cuda", dtype=torch.float16):
        net.run_cuda(ro, rd, shading='lambertian', **kw)
    net.run_cuda(ro, rd, shading='normal', perturb=True, **kw)
    net.train()
    try:
        net.run_cuda(ro, rd, shading='normal', **kw)
    finally:
        net.eval()
    assert net.run_calls == [(False, 'lambertian', False), (False, 'normal', True), (True, 'normal', False)]
    lat = _case(2, 32, 1000, False, True)
    del lat.net.run_calls[:]
    with pytest.raises(RuntimeError):                            # ill-formed in the reference: five channels into a four-channel image
        lat.net.run_cuda(ro, rd, shading='lambertian', light_d=lat.light, ambient_ratio=sc.AMBIENT, max_steps=rc.MAX_STEPS)
    assert lat.net.run_calls == [(False, 'lambertian', False)]
    nerf.unbind_nerf_network(net)
    try:
        assert "run_cuda" not in net.__dict__
        del net.run_calls[:]
        for shading in SHADINGS + ("albedo",):
            net.run_cuda(ro, rd, shading=shading, **kw)
        assert net.run_calls == [(False, s, False) for s in SHADINGS + ("albedo",)]
    finally:
        assert nerf.bind_nerf_network(net, shaded_render=True) is None


def test_degenerate_calls():
    c = _case(2, 32, 1000, False, False)
    net = c.net
    field = (net.encoder, net.sigma_net, net.sigma_scale, net.bound)
    e3, e1 = torch.empty((0, 3), device="cuda"), torch.empty(0, device="cuda")
    o = torch.full((300, 3), 10.0, device="cuda")                # every ray misses the box: near = far = FLT_MAX
    d = torch.tensor([[1.0, 0.0, 0.0]], device="cuda").repeat(300, 1)
    nears, fars = raymarch.near_far_from_aabb(o, d, net.aabb_infer)
    assert not bool((nears < fars).any())
    empty = torch.zeros_like(net.density_bitfield)               # every ray crosses the box and finds nothing
    for shading in SHADINGS:
        kw = dict(density_activation='exp', density_prior='gaussian', albedo_sigmoid=True, max_steps=rc.MAX_STEPS, return_counts=True,
                  shading=shading, light_d=c.light, ambient_ratio=sc.AMBIENT)
        ws, dep, img, cnt = nerf_render.render_rays(e3, e3, e1, e1, net.density_bitfield, net.cascade, net.grid_size, *field, **kw)
        assert ws.shape == (0,) and dep.shape == (0,) and img.shape == (0, 3) and cnt.shape == (0,)
        for out in nerf_render.render_rays(o, d, nears, fars, net.density_bitfield, net.cascade, net.grid_size, *field, **kw):
            assert int(out.count_nonzero()) == 0
        for out in nerf_render.render_rays(c.rays_o, c.rays_d, c.nears, c.fars, empty, net.cascade, net.grid_size, *field, **kw):
            assert int(out.count_nonzero()) == 0


def test_render_rays_refuses_what_the_c_entry_refuses():
    c = _case(2, 32, 1000, False, False)
    with pytest.raises(RuntimeError, match="light_d"):
        _native(c, "textureless", light_d=None)
    with pytest.raises(RuntimeError, match="light_d"):
        _native(c, "lambertian", light_d=c.light.double())
    with pytest.raises(RuntimeError, match="normal_epsilon"):
        _native(c, "normal", normal_epsilon=0.0)
    lat = _case(2, 32, 1000, False, True)
    with pytest.raises(RuntimeError, match="lambertian"):
        _native(lat, "lambertian")
    _native(c, "normal", light_d=None)                           # 'normal' reads no light


def test_distance_from_the_float64_normal_view_is_printed():
    """Information, not a threshold: the largest difference between the native 'normal' image at 1000 rays and the float64 restatement
    of nerf_shading_cases.exact_normal_image.  It documents how far fp32 finite differences of the density sit from the exact ones; no
    bound for it can be derived."""
    c = _case(2, 32, 1000, False, False)
    ws, dep, img, cnt = (t.cpu().numpy() for t in _native(c, "normal"))
    net = sc.make_shading_network(c.H, c.bound)
    want = sc.exact_normal_image(net, c.o, c.d, c.bits, c.bound, c.C, c.H, cnt)
    diff = np.abs(img.astype(np.float64) - want)
    print("normal view, native fp32 against the float64 restatement: max |difference| = %.3g, mean = %.3g" % (diff.max(), diff.mean()))
    assert np.isfinite(diff).all()
