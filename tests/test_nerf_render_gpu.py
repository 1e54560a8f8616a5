"""GPU tests of the one-launch inference render (boundary B14, dreamwaltz_g_amd.nerf_render / csrc/nerf_field.hip k_nf_render) against
the composition a bound network ran before it: tests/nerf_render_cases._NeRFNetwork.run_cuda, the reference's loop of march_rays ->
field -> composite_rays over the package's own kernels."""
import functools

import numpy as np
import pytest
import torch

from dreamwaltz_g_amd import nerf, nerf_render, raymarch
from tests import nerf_render_cases as rc

pytestmark = pytest.mark.gpu

# seeds chosen on the CPU with nerf_render_cases.host_counts (see test_parity_with_the_composition)
SEEDS = {5: 1, 1000: 9, 3000: 3}


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(C, H, n, f16, latent, prior="gaussian", kind="body", seed=None):
    """A scene on the device, its bound network and -- computed once and left unchanged -- the composition's result, records and trace."""
    c = _Case()
    o, d, bits, bound = rc.make_scene(C, H, n, seed=SEEDS[n] if seed is None else seed, kind=kind)
    c.n, c.f16, c.latent, c.prior = n, f16, latent, prior
    c.net = rc.make_render_network(H, bound, density_prior=prior, latent=latent).cuda().eval()
    with torch.no_grad():
        c.net.density_bitfield.copy_(torch.from_numpy(bits))
    assert nerf.bind_nerf_network(c.net) is None
    c.rays_o, c.rays_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    c.nears, c.fars = raymarch.near_far_from_aabb(c.rays_o, c.rays_d, c.net.aabb_infer)
    return c


def _composition(c, max_steps=rc.MAX_STEPS):
    if not hasattr(c, "composed"):
        c.net.record = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
            out = c.net.run_cuda.__wrapped__(c.rays_o[None], c.rays_d[None], light_d=c.rays_o[0], max_steps=max_steps, T_thresh=rc.T_THRESH)
        c.records, c.net.record = c.net.record, None
        c.composed = tuple(out[k][0].cpu().numpy() for k in ("weights_sum", "depth", "image"))
        c.mask = out["mask"][0].cpu().numpy()
        c.trace = rc.trace(c.records, c.n, rc.T_THRESH)
    return c


def _native(c, max_workgroups=0, max_steps=rc.MAX_STEPS):
    net = c.net
    with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
        return nerf_render.render_rays(c.rays_o, c.rays_d, c.nears, c.fars, net.density_bitfield, net.cascade, net.grid_size, net.encoder,
                                       net.sigma_net, net.sigma_scale, net.bound, density_activation='exp', density_prior=c.prior,
                                       albedo_sigmoid=not c.latent, max_steps=max_steps, T_thresh=rc.T_THRESH, return_counts=True,
                                       max_workgroups=max_workgroups)


PARITY = [(1, 16, 5, False, 0), (2, 32, 1000, False, 0), (2, 32, 1000, False, 2), (2, 32, 1000, True, 0), (2, 32, 1000, True, 2),
          (2, 64, 3000, False, 0), (2, 64, 3000, False, 2)]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("C,H,n,latent,max_workgroups", PARITY)
def test_parity_with_the_composition(C, H, n, latent, max_workgroups, f16):
    """The native render against the composition, by the rule of nerf_render_cases.compare: on rays with no transmittance test within
    1e-6 of T_thresh the counts equal the float32 trace's and weights_sum / depth / image agree within (S + 2) 2^-23 scale (S the ray's
    count; scale 1, max(fars), max(1, max |rgbs|)): the two kernels may contract ws + alpha * T-style statements differently, one rounding
    of a quantity <= scale per sample, and the feedback through T contracts.  Borderline rays (at most 0.5 %) may differ by one sample and
    agree within T_thresh scale.  5 rays: below one 64-ray block; 1000: not a multiple of 64; max_workgroups 2 puts 1000 and 3000 rays
    above slots x workgroups = 512, so every workgroup refills its slots.  latent: four channels, no sigmoid.

    ROUNDING PATH.  The f16 cases fail if the albedo is not rounded through half before it is composited: that error is 2^-11 per
    sample, about 100 times this bound.

    FAIR SCENE (asserted at 1000 and 3000 rays from the composition's own records; 5 rays cannot hold the floors): >= 50 rays end by
    T_thresh, >= 50 at far with samples, >= 10 have no sample, the largest count is below max_steps, borderline share under the cap.
    The seeds were chosen ON THE CPU, without a device, with nerf_render_cases.host_counts: raymarch_cases' numpy march for the samples,
    nerf_field_cases.restate (float64, fp16 rounding points) for the density, the float32 trace for the counts.  It gave, as
    (by T_thresh, at far, no sample, largest count, borderline): 1000 rays seed 9: rgb (129, 743, 128, 48, 1), latent (146, 726, 128, 48,
    3); 3000 rays seed 3: (139, 2197, 664, 54, 3); 5 rays seed 1: (1, 1, 3, 15, 0).  Seeds 0-8 at 1000 rays gave 16-57 rays by T_thresh
    and were passed over.  The device figures, and how many rays were bit-equal in all four outputs, are printed by compare().
    On an MI355X the scene figures were the CPU check's exactly, and in all fourteen cases every ray (5 / 1000 / 3000 of them, the 1-3
    borderline ones included) was bit-equal to the composition in weights_sum, depth, image and count.  Information, not a threshold."""
    c = _composition(_case(C, H, n, f16, latent))
    if n >= 1000:
        fair = rc.fairness(c.trace, n)
        print("fair scene:", fair)
        rc.assert_fair(fair, n)
    else:
        assert c.trace["count"].max() < rc.MAX_STEPS
    ws, dep, img, cnt = (t.cpu().numpy() for t in _native(c, max_workgroups))
    assert img.shape == (n, 4 if latent else 3)
    rc.compare((ws, dep, img, cnt), c.composed, c.trace, c.mask, c.fars.cpu().numpy(), c.records)


def test_a_ray_stops_after_exactly_max_steps_samples():
    """The documented difference from the loop: a fully occupied bitfield, a field without the prior (density near 1) and max_steps 16.
    bound 4 with the eye within radius 2: every ray has more than 16 x dt = 3.46 of box in front of it, so every ray composites exactly
    16 samples and none more, and weights_sum is the float32 composite of the first 16 samples of the training march."""
    c = _case(3, 32, 1000, False, False, prior="none", kind="dense")
    ws, dep, img, cnt = (t.cpu().numpy() for t in _native(c, max_steps=16))
    assert (cnt == 16).all(), (cnt.min(), cnt.max())
    xyzs, dirs, ts, rays = raymarch.march_rays_train(c.rays_o, c.rays_d, c.net.bound, c.net.density_bitfield, c.net.cascade, c.net.grid_size,
                                                     c.nears, c.fars, False, 0, 16)
    rays = rays.cpu().numpy()
    assert (rays[:, 1] == 16).all()
    with torch.no_grad():
        sigmas = c.net.common_forward(xyzs)[0]
    want, used = rc.composite_first(sigmas.cpu().numpy(), ts.cpu().numpy(), rays, 16)
    assert (used == 16).all()
    err = np.abs(ws.astype(np.float64) - want)
    print("cap: max |weights_sum - composite| = %.3g (bound %.3g)" % (err.max(), 18 * rc.ULP))
    assert (err <= 18 * rc.ULP).all(), err.max()
    assert (ws > 0.5).all() and (ws < 1.0).all()


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_two_runs_and_any_number_of_workgroups_give_the_same_bits(f16):
    c = _case(2, 32, 1000, f16, False)
    first = _native(c)
    for mw in (0, 2, 1):
        again = _native(c, max_workgroups=mw)
        for a, b in zip(first, again):
            assert torch.equal(a, b), mw
    c = _case(2, 64, 3000, f16, False)
    for a, b in zip(_native(c), _native(c, max_workgroups=2)):
        assert torch.equal(a, b)


def test_binding_runs_the_native_render_in_eval_and_the_original_elsewhere():
    c = _case(2, 32, 1000, False, False)
    net = c.net
    ro, rd = c.rays_o[None], c.rays_d[None]
    want = _native(c)
    net.run_cuda(ro, rd, max_steps=rc.MAX_STEPS)                 # the encoder's offsets are read to the host once, here or earlier
    del net.run_calls[:]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = net.run_cuda(ro, rd, light_d=None, max_steps=rc.MAX_STEPS, T_thresh=rc.T_THRESH)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert net.run_calls == []                                   # the class method was not reached
    assert set(out) == {"image", "depth", "weights_sum", "mask", "xyzs", "sigmas", "rgbs"}
    assert out["xyzs"] is None and out["sigmas"] is None and out["rgbs"] is None
    assert out["image"].shape == (1, c.n, 3) and out["depth"].shape == (1, c.n) and out["weights_sum"].shape == (1, c.n)
    assert torch.equal(out["weights_sum"][0], want[0]) and torch.equal(out["depth"][0], want[1]) and torch.equal(out["image"][0], want[2])
    assert out["mask"].dtype == torch.bool and torch.equal(out["mask"][0], c.nears < c.fars)
    # the light_d draw advances the device generator exactly as the original does
    torch.cuda.manual_seed(5)
    start = torch.cuda.get_rng_state()
    net.run_cuda(ro, rd, light_d=None, max_steps=rc.MAX_STEPS)
    after_native = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(5)
    net.run_cuda.__wrapped__(ro, rd, light_d=None, max_steps=rc.MAX_STEPS)
    after_original = torch.cuda.get_rng_state()
    assert torch.equal(after_native, after_original) and not torch.equal(after_native, start)
    # calls the native render does not take
    del net.run_calls[:]
    net.run_cuda(ro, rd, shading='normal', max_steps=rc.MAX_STEPS)
    net.run_cuda(ro, rd, perturb=True, max_steps=rc.MAX_STEPS)
    net.train()
    try:
        net.run_cuda(ro, rd, max_steps=rc.MAX_STEPS)
    finally:
        net.eval()
    assert net.run_calls == [(False, 'normal', False), (False, 'albedo', True), (True, 'albedo', False)]
    nerf.unbind_nerf_network(net)
    try:
        assert "run_cuda" not in net.__dict__
        net.run_cuda(ro, rd, max_steps=rc.MAX_STEPS)
        assert net.run_calls[-1] == (False, 'albedo', False)
    finally:
        assert nerf.bind_nerf_network(net) is None


def test_degenerate_calls():
    c = _case(2, 32, 1000, False, False)
    net = c.net
    kw = dict(density_activation='exp', density_prior='gaussian', albedo_sigmoid=True, max_steps=rc.MAX_STEPS, return_counts=True)
    field = (net.encoder, net.sigma_net, net.sigma_scale, net.bound)
    e3, e1 = torch.empty((0, 3), device="cuda"), torch.empty(0, device="cuda")
    ws, dep, img, cnt = nerf_render.render_rays(e3, e3, e1, e1, net.density_bitfield, net.cascade, net.grid_size, *field, **kw)
    assert ws.shape == (0,) and dep.shape == (0,) and img.shape == (0, 3) and cnt.shape == (0,)
    # every ray misses the box: near = far = FLT_MAX
    o = torch.full((300, 3), 10.0, device="cuda")
    d = torch.tensor([[1.0, 0.0, 0.0]], device="cuda").repeat(300, 1)
    nears, fars = raymarch.near_far_from_aabb(o, d, net.aabb_infer)
    assert not bool((nears < fars).any())
    for out in nerf_render.render_rays(o, d, nears, fars, net.density_bitfield, net.cascade, net.grid_size, *field, **kw):
        assert int(out.count_nonzero()) == 0
    # an empty bitfield: every ray crosses the box and finds nothing
    empty = torch.zeros_like(net.density_bitfield)
    for out in nerf_render.render_rays(c.rays_o, c.rays_d, c.nears, c.fars, empty, net.cascade, net.grid_size, *field, **kw):
        assert int(out.count_nonzero()) == 0
