"""GPU tests of the training render (boundary B18, dreamwaltz_g_amd.nerf_render.render_rays_train; csrc/raymarch.hip
k_composite_fwd<NC, true>, csrc/nerf_train.hip) against THE COMPOSITION it replaces, with the same noises:
raymarch.march_rays_train -> nerf.nerf_field -> raymarch.composite_rays_train."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dreamwaltz_g_amd import nerf, nerf_render, raymarch
from tests import nerf_field_cases as nc
from tests import nerf_render_cases as rc
from tests import nerf_train_cases as tc
from tests import raymarch_cases as rmc

pytestmark = pytest.mark.gpu

SEED = {n: s for _, _, n, s in tc.SCENES}
GRID = {n: (C, H) for C, H, n, _ in tc.SCENES}
MODES = [pytest.param(False, False, id="f32-rgb"), pytest.param(False, True, id="f32-latent"), pytest.param(True, False, id="f16-rgb"),
         pytest.param(True, True, id="f16-latent")]


class _Case:
    pass


def _params(net):
    out = {'embeddings': net.encoder.embeddings, 'sigma_scale': net.sigma_scale}
    for l, lin in enumerate(net.sigma_net.net):
        out['w%d' % l], out['b%d' % l] = lin.weight, lin.bias
    return out


@functools.lru_cache(maxsize=None)
def _case(n, f16, latent, act='exp', opaque=False, empty=False):
    """A scene on the device with its network, noises and seeded upstream gradients; the composition's results are added once by
    _composition and left unchanged."""
    c = _Case()
    C, H = GRID[n]
    o, d, bits, bound = rc.make_scene(C, H, n, seed=SEED[n])
    c.n, c.f16, c.latent, c.act, c.C, c.H, c.bound = n, f16, latent, act, C, H, bound
    c.ch = 4 if latent else 3
    c.net = tc.make_network(H, bound, latent, act, opaque).cuda()
    with torch.no_grad():
        c.net.density_bitfield.copy_(torch.from_numpy(bits))
        if empty:
            c.net.density_bitfield.zero_()
    c.rays_o, c.rays_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    c.nears, c.fars = raymarch.near_far_from_aabb(c.rays_o, c.rays_d, c.net.aabb_train)
    c.noises = torch.from_numpy(tc.noises(n, SEED[n])).cuda()
    g = torch.Generator().manual_seed(1000 + n)
    c.g_ws, c.g_depth = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    c.g_image = torch.randn(n, c.ch, generator=g).cuda()
    c.composed = {}
    return c


def _field_kw(c):
    return dict(density_activation=c.act, density_prior='gaussian', albedo_sigmoid=not c.latent)


def _composition(c, T_thresh=tc.T_THRESH):
    """march_rays_train -> nerf_field -> composite_rays_train and its backward with the case's upstream gradients, once per T_thresh."""
    if T_thresh not in c.composed:
        net = c.net
        r = {}
        with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
            xyzs, dirs, ts, rays = raymarch.march_rays_train(c.rays_o, c.rays_d, c.bound, net.density_bitfield, c.C, c.H, c.nears, c.fars,
                                                             True, 0, tc.MAX_STEPS, noises=c.noises)
            sigmas, albedo = nerf.nerf_field(xyzs, net.encoder, net.sigma_net, net.sigma_scale, c.bound, **_field_kw(c))
            rgbs = albedo.float()
            weights, ws, depth, image = raymarch.composite_rays_train(sigmas, rgbs, ts, rays, T_thresh)
        names = [k for k, p in _params(net).items() if k != 'sigma_scale' or c.act == 'scaling']
        if xyzs.shape[0]:
            grads = torch.autograd.grad([ws, depth, image], [_params(net)[k] for k in names] + [sigmas, rgbs], [c.g_ws, c.g_depth, c.g_image])
            r["grads"] = dict(zip(names, grads[:len(names)]))
            r["grad_sigmas"], r["grad_rgbs"] = grads[-2], grads[-1]
        r.update(M=xyzs.shape[0], ts=ts, rays=rays, sigmas=sigmas.detach(), weights=weights.detach(), out=(ws.detach(), depth.detach(), image.detach()))
        c.composed[T_thresh] = r
    return c.composed[T_thresh]


def _native(c, T_thresh=tc.T_THRESH, backward=True, **kw):
    """render_rays_train and its backward -> dict(out, weights, sigmas, stats, grads, debug)."""
    net = c.net
    debug = {}
    with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
        ws, depth, image, weights, sigmas, stats = nerf_render.render_rays_train(
            c.rays_o, c.rays_d, c.nears, c.fars, net.density_bitfield, c.C, c.H, net.encoder, net.sigma_net, net.sigma_scale, c.bound,
            **_field_kw(c), noises=c.noises, max_steps=tc.MAX_STEPS, T_thresh=T_thresh, return_weights=True, return_sigmas=True,
            return_stats=True, _debug=debug, **kw)
    r = dict(out=(ws.detach(), depth.detach(), image.detach()), weights=weights, sigmas=sigmas, stats=stats, debug=debug)
    if backward and ws.requires_grad:
        names = [k for k, p in _params(net).items() if p.requires_grad and (k != 'sigma_scale' or c.act == 'scaling')]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                  # the backward makes no host read
        try:
            grads = torch.autograd.grad([ws, depth, image], [_params(net)[k] for k in names], [c.g_ws, c.g_depth, c.g_image])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        r["grads"] = dict(zip(names, grads))
    return r


def _live_rows(rays, rays_live):
    """Row index, in the full arrays, of every live row in the order of the live arrays."""
    live = rays_live[:, 1].long()
    ray = torch.repeat_interleave(torch.arange(len(live), device=live.device), live)
    r = torch.arange(int(live.sum()), device=live.device) - rays_live[:, 0].long()[ray]
    return rays[:, 0].long()[ray] + r


@pytest.mark.parametrize("f16,latent", MODES)
@pytest.mark.parametrize("n", [5, 1000, 3000])
def test_forward_live_and_gradients_against_the_composition(n, f16, latent):
    """One native forward + backward per case against the composition.

    FORWARD: weights_sum, depth, image and weights are torch.equal: the same kernels on the same inputs.
    LIVE: off the borderline rays (a transmittance test within 1e-7 of T_thresh, float64 on the device's own sigmas and ts) live equals
    `used` of raymarch_cases.composite_forward; for every ray the composition's weights at or beyond live are exactly 0, and for every cut
    ray the row live - 1 is the last one written.
    PREMISE AND COMPOSITE BACKWARD: the composition's grad_sigmas / grad_rgbs are exactly 0 on every culled row and torch.equal to the
    native path's gradients on the live rows.
    PARAMETER GRADIENTS: relative L2 <= 1e-4 for the table and every weight and bias: the per-row terms are the same bits, the fp32
    summation order differs (fewer rows per chunk of the field backward).

    FAIR SCENE (asserted at 1000 and 3000 rays from the device's own live): >= 100 rays cut, >= 100 whole, >= 100 without a sample, culled
    share >= 0.03, rays longer than 64 samples on both sides of a cut and a stop inside a later chunk, borderline rays <= 0.5 %.  The CPU
    check (nerf_train_cases.host_figures: numpy march, nerf_field_cases.restate, float64 stop rule; no device) gave, as (M, M_live, cut,
    whole, no sample, longest, borderline): 1000 rays seed 9: f32 rgb (84333, 76689, 130, 745, 125, 190, 0), f32 latent (84333, 75260,
    148, 727, 125, 190, 1), f16 rgb (84333, 76689, 130, 745, 125, 190, 2), f16 latent (84333, 75259, 148, 727, 125, 190, 2); 3000 rays
    seed 3: f32 rgb (172556, 164269, 138, 2203, 659, 212, 2), f32 latent (172556, 162985, 157, 2184, 659, 212, 1), f16 rgb (172556,
    164268, 138, 2203, 659, 212, 3), f16 latent (172556, 162985, 157, 2184, 659, 212, 0); 5 rays seed 1: (163, 69, 1, 1, 3, 148, 0), latent
    M_live 65.  In every case rays longer than 64 samples are cut (>= 130), whole (>= 471) and stop in a later chunk (>= 77).
    On an MI355X the device's figures (M_live among them) were the CPU check's exactly in all twelve cases, and the
    parameter gradients' relative L2 was at most 1.2e-6 (3.3e-11 for the table).  Information, not a threshold."""
    c = _case(n, f16, latent)
    comp, nat = _composition(c), _native(c)
    # forward
    for a, b in zip(nat["out"], comp["out"]):
        assert torch.equal(a, b)
    assert nat["out"][2].shape == (n, c.ch)
    assert torch.equal(nat["weights"], comp["weights"]) and torch.equal(nat["sigmas"], comp["sigmas"])
    assert not nat["weights"].requires_grad and not nat["sigmas"].requires_grad and nat["sigmas"].dtype == torch.float32
    # live
    st = nat["stats"]
    rays = comp["rays"].cpu().numpy()
    live = st["live"].cpu().numpy().astype(np.int64)
    counts = rays[:, 1].astype(np.int64)
    sig, ts = comp["sigmas"].cpu().numpy(), comp["ts"].cpu().numpy()
    assert st["M"] == comp["M"] == counts.sum() and st["M_live"] == live.sum()
    used = rmc.composite_forward(sig, np.zeros((len(sig), c.ch)), ts, rays, tc.T_THRESH)[4]
    _, margin = tc.stops(sig, ts, counts)
    border = margin <= tc.BORDER
    fig = tc.figures(live, counts, margin)
    print("device figures:", fig)
    assert (live[~border] == used[~border]).all() and (np.abs(live[border] - used[border]) <= 1).all()
    if n >= 1000:
        tc.assert_fair(fig, n)
    w = comp["weights"].cpu().numpy()
    written = np.zeros(len(w), bool)
    for k in range(n):
        written[rays[k, 0]:rays[k, 0] + live[k]] = True
    assert (w[~written] == 0).all()
    cut = live < counts
    assert (w[rays[cut, 0] + live[cut] - 1] > 0).all()
    # premise and composite backward
    dbg = nat["debug"]
    assert torch.equal(dbg["rays"], comp["rays"]) and torch.equal(dbg["rays_live"][:, 1], st["live"])
    assert torch.equal(dbg["rays_live"][:, 0].long(), torch.cumsum(st["live"].long(), 0) - st["live"].long())
    rows = _live_rows(dbg["rays"], dbg["rays_live"])
    culled = torch.ones(comp["M"], dtype=torch.bool, device="cuda")
    culled[rows] = False
    assert int(culled.sum()) == st["M"] - st["M_live"]
    assert comp["grad_rgbs"].dtype == torch.float32
    assert int(comp["grad_sigmas"][culled].count_nonzero()) == 0 and int(comp["grad_rgbs"][culled].count_nonzero()) == 0
    assert torch.equal(comp["grad_sigmas"][rows], dbg["grad_sigmas_live"]) and torch.equal(comp["grad_rgbs"][rows], dbg["grad_rgbs_live"])
    assert int(dbg["grad_sigmas_live"].count_nonzero()) > 0
    # parameter gradients
    assert nat["grads"].keys() == comp["grads"].keys() and 'sigma_scale' not in nat["grads"]
    err = {k: nc.rel_l2(nat["grads"][k], comp["grads"][k]) for k in comp["grads"]}
    print("parameter gradients, relative L2:", err)
    for k, e in err.items():
        assert e <= tc.F32_BWD, (k, e)
        assert float(comp["grads"][k].abs().max()) > 0, k


@pytest.mark.parametrize("f16,latent", MODES)
def test_sigma_scale_gradient_under_scaling(f16, latent):
    """density_activation 'scaling': sigma_scale gets a gradient too, compared like the others."""
    c = _case(1000, f16, latent, act='scaling')
    comp, nat = _composition(c), _native(c)
    for a, b in zip(nat["out"], comp["out"]):
        assert torch.equal(a, b)
    assert 'sigma_scale' in nat["grads"] and nat["grads"]['sigma_scale'].shape == c.net.sigma_scale.shape
    for k in comp["grads"]:
        e = nc.rel_l2(nat["grads"][k], comp["grads"][k])
        assert e <= tc.F32_BWD, (k, e)
    assert float(comp["grads"]['sigma_scale'].abs().max()) > 0


@pytest.mark.parametrize("f16,latent", MODES)
def test_nothing_culled_gives_the_compositions_gradients_bit_for_bit(f16, latent):
    """T_thresh = 0: no ray stops, M_live == M, the gather is the identity and the backward is the composition's."""
    c = _case(1000, f16, latent)
    comp, nat = _composition(c, 0.0), _native(c, 0.0)
    assert nat["stats"]["M_live"] == nat["stats"]["M"] == comp["M"] > 0
    assert torch.equal(nat["stats"]["live"], comp["rays"][:, 1])
    for a, b in zip(nat["out"], comp["out"]):
        assert torch.equal(a, b)
    for k in comp["grads"]:
        assert torch.equal(nat["grads"][k], comp["grads"][k]), k


@pytest.mark.parametrize("f16,latent", MODES)
def test_two_runs_give_the_same_bits(f16, latent):
    c = _case(3000, f16, latent)
    a, b = _native(c), _native(c)
    for x, y in zip(a["out"] + (a["weights"], a["sigmas"], a["stats"]["live"]), b["out"] + (b["weights"], b["sigmas"], b["stats"]["live"])):
        assert torch.equal(x, y)
    assert a["stats"]["M_live"] == b["stats"]["M_live"]
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("f16,latent", MODES)
def test_every_ray_cut(f16, latent):
    """'scaling' with sigma_scale 6 and a raised density bias (nerf_train_cases.make_network, opaque): every ray with samples is spent
    within three of them.  The CPU check gave, f32 and f16, three and four channels alike: M 84333, M_live 875 (one sample for each of the 875 rays that have
    any), 868 rays longer than three samples, all of them cut."""
    c = _case(1000, f16, latent, act='scaling', opaque=True)
    comp, nat = _composition(c), _native(c)
    live, counts = nat["stats"]["live"].cpu().numpy(), comp["rays"][:, 1].cpu().numpy()
    assert (live[counts > 0] >= 1).all() and live.max() <= 3 and (live[counts > 3] < counts[counts > 3]).all()
    assert (counts > 3).sum() >= 800 and nat["stats"]["M_live"] <= 3 * (counts > 0).sum() < nat["stats"]["M"] // 10
    for a, b in zip(nat["out"], comp["out"]):
        assert torch.equal(a, b)
    assert torch.equal(nat["weights"], comp["weights"])
    for k in comp["grads"]:
        e = nc.rel_l2(nat["grads"][k], comp["grads"][k])
        assert e <= tc.F32_BWD, (k, e)


@pytest.mark.parametrize("f16,latent", MODES)
def test_no_rays_and_no_samples(f16, latent):
    c = _case(1000, f16, latent)
    net = c.net
    args = (net.density_bitfield, c.C, c.H, net.encoder, net.sigma_net, net.sigma_scale, c.bound)
    e3, e1 = torch.empty((0, 3), device="cuda"), torch.empty(0, device="cuda")
    with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
        ws, depth, image, weights, sigmas, st = nerf_render.render_rays_train(e3, e3, e1, e1, *args, **_field_kw(c), return_weights=True,
                                                                             return_sigmas=True, return_stats=True)
    assert ws.shape == (0,) and depth.shape == (0,) and image.shape == (0, c.ch) and weights.shape == (0,) and sigmas.shape == (0,)
    assert st["M"] == 0 and st["M_live"] == 0 and st["live"].shape == (0,)
    # a bitfield of zeros: every ray crosses the box and finds nothing; the backward hands out zeros
    c = _case(1000, f16, latent, empty=True)
    nat = _native(c)
    assert set(nat["grads"]) == set(_params(c.net)) - {'sigma_scale'}              # the backward ran, through its M_live = 0 return
    assert nat["stats"]["M"] == 0 and nat["stats"]["M_live"] == 0 and int(nat["stats"]["live"].count_nonzero()) == 0
    for t in nat["out"]:
        assert int(t.count_nonzero()) == 0
    assert nat["weights"].shape == (0,) and nat["sigmas"].shape == (0,)
    for k, g in nat["grads"].items():
        assert g.shape == _params(c.net)[k].shape and int(g.count_nonzero()) == 0, k


@pytest.mark.parametrize("f16,latent", MODES)
@pytest.mark.parametrize("mode", [torch.no_grad, torch.inference_mode])
def test_without_grad_nothing_is_gathered_or_saved(mode, f16, latent):
    c = _case(1000, f16, latent)
    want = _native(c)
    with mode():
        got = _native(c, backward=False)
    for a, b in zip(got["out"], want["out"]):
        assert torch.equal(a, b) and not a.requires_grad
    assert got["debug"] == {} and want["debug"].keys() >= {"rays", "rays_live"}          # the gather did not run
    assert got["stats"]["M_live"] == want["stats"]["M_live"]


@pytest.mark.parametrize("f16,latent", MODES)
def test_needs_input_grad_combinations(f16, latent):
    c = _case(1000, f16, latent, act='scaling')
    full = _native(c)["grads"]
    params = _params(c.net)
    try:
        # the table and sigma_scale only
        for k, p in params.items():
            p.requires_grad_(k in ('embeddings', 'sigma_scale'))
        got = _native(c)["grads"]
        assert set(got) == {'embeddings', 'sigma_scale'}
        for k in got:
            assert torch.equal(got[k], full[k]), k
        # a frozen table, only layer 1's weight
        for k, p in params.items():
            p.requires_grad_(k == 'w1')
        got = _native(c)["grads"]
        assert set(got) == {'w1'} and torch.equal(got['w1'], full['w1'])
        # nothing requires grad: nothing is saved
        for p in params.values():
            p.requires_grad_(False)
        r = _native(c)
        assert not r["out"][0].requires_grad and r["debug"] == {}
    finally:
        for p in params.values():
            p.requires_grad_(True)


@pytest.mark.parametrize("f16,latent", MODES)
def test_counter_and_the_perturbation_draw(f16, latent):
    """counter receives what march_rays_train adds (the sample count); without `noises` the draw is march_rays_train's torch.rand(N)."""
    c = _case(1000, f16, latent)
    cast = lambda: torch.autocast("cuda", dtype=torch.float16, enabled=f16)  # noqa: E731
    net = c.net
    args = (c.rays_o, c.rays_d, c.nears, c.fars, net.density_bitfield, c.C, c.H, net.encoder, net.sigma_net, net.sigma_scale, c.bound)
    counter = torch.tensor([7, 3], dtype=torch.int32, device="cuda")
    torch.cuda.manual_seed(11)
    with cast():
        ws, depth, image, st = nerf_render.render_rays_train(*args, **_field_kw(c), perturb=True, counter=counter, return_stats=True)
    assert counter.tolist() == [7 + st["M"], 3]
    torch.cuda.manual_seed(11)
    xyzs, dirs, ts, rays = raymarch.march_rays_train(c.rays_o, c.rays_d, c.bound, net.density_bitfield, c.C, c.H, c.nears, c.fars, True, 0, 1024)
    assert st["M"] == xyzs.shape[0]
    with cast():
        sigmas, rgbs = nerf.nerf_field(xyzs, net.encoder, net.sigma_net, net.sigma_scale, c.bound, **_field_kw(c))
        want = raymarch.composite_rays_train(sigmas, rgbs, ts, rays, 1e-4)
    assert torch.equal(ws, want[1]) and torch.equal(depth, want[2]) and torch.equal(image, want[3])
    # perturb False: the march of zeros
    with cast():
        ws0 = nerf_render.render_rays_train(*args, **_field_kw(c), perturb=False)[0]
        ws1 = nerf_render.render_rays_train(*args, **_field_kw(c), noises=torch.zeros(c.n, device="cuda"))[0]
    assert torch.equal(ws0, ws1) and not torch.equal(ws0, ws)


def test_argument_errors_raise_before_any_launch():
    """Every refusal comes before the precision or the channel count is looked at and before any launch, so one mode covers them."""
    c = _case(1000, False, False)
    net = c.net
    good = [c.rays_o, c.rays_d, c.nears, c.fars, net.density_bitfield, c.C, c.H, net.encoder, net.sigma_net, net.sigma_scale, c.bound]
    kw = _field_kw(c)

    def bad(i, v, **more):
        a = list(good)
        a[i] = v
        with pytest.raises(RuntimeError):
            nerf_render.render_rays_train(*a, **dict(kw, **more))
    bad(0, c.rays_o.cpu())
    bad(1, c.rays_d.double())
    bad(1, c.rays_d[:-1])
    bad(2, c.nears[:-1])
    bad(3, c.fars.cpu())
    bad(0, c.rays_o.clone().requires_grad_(True))
    bad(4, net.density_bitfield[:-1])
    bad(4, net.density_bitfield.int())
    bad(6, 48)                                                   # not a power of two
    bad(5, 9)
    bad(0, c.rays_o, noises=c.noises[:-1])
    bad(0, c.rays_o, noises=c.noises.cpu())
    bad(0, c.rays_o, counter=torch.zeros(1, device="cuda"))      # not int32
    bad(0, c.rays_o, max_steps=0)
    bad(0, c.rays_o, density_prior='smpl')


@pytest.mark.parametrize("N", [1, 255, 1023, 1024, 1025, 4097, 1024 * 1024 + 5])
def test_compact_offsets_against_cumsum(N):
    """dwg_nerf_train_compact_offsets on its own: the pairs are (exclusive cumsum, max(live, 0)) and total is overwritten with the sum.
    Sizes around the scan block of 1024 rays; the last one has more than 1024 blocks, so the scan of the block sums takes a second
    trip and carries the first trip's total across.  Integers: exact.  The sum is at most 70 N < 7.4e7."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    live = torch.randint(-3, 71, (N,), generator=torch.Generator().manual_seed(N), dtype=torch.int32).cuda()
    rays_live = torch.full((N, 2), -1, dtype=torch.int32, device="cuda")
    total = torch.tensor([12345], dtype=torch.int32, device="cuda")
    nbytes = int(L.dwg_nerf_train_workspace_bytes(N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.dwg_nerf_train_compact_offsets(_lib.ptr(live), N, _lib.ptr(rays_live), _lib.ptr(total), _lib.ptr(ws), nbytes, stream),
               "dwg_nerf_train_compact_offsets")
    want = live.clamp(min=0)
    if N > 1:
        assert int((live < 0).sum()) > 0 and int((live > 0).sum()) > 0
    assert torch.equal(rays_live[:, 1], want)
    csum = torch.cumsum(want.long(), 0)
    assert torch.equal(rays_live[:, 0], (csum - want.long()).to(torch.int32))
    assert total.tolist() == [int(csum[-1])]


def test_gather_entry_points_against_torch_indexing():
    """dwg_nerf_train_gather_live and dwg_nerf_train_gather_live_rows on their own, torch.equal to torch indexing: bit copies.  Nine
    rays: two waves of four and a tail of one; counts of 70 and 130 take more than one trip of a wave's 64 lanes.  Ray 1 has live == 0,
    ray 2 live == count, ray 7's source range ends past M and is skipped, so its four live rows keep the fill, as every row no ray
    owns would.  Odd offsets on both sides (5, 79, 83 / 3, 73, 75) put the 6-byte f16 rgb rows on odd half-words.  Colours f32 with 3
    and 4 channels, f16 with 3 (half-word slot) and 4 (two-word slot); some arrays NULL; rows of 6 floats and of 1."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    counts, live = [5, 3, 70, 1, 4, 130, 2, 6, 7], [3, 0, 70, 1, 1, 65, 2, 4, 5]
    N, M, M_live = len(counts), sum(counts), sum(live)
    rays = torch.tensor([[sum(counts[:i]), c] for i, c in enumerate(counts)], dtype=torch.int32)
    rays[7, 0] = M - 2                                              # 6 rows from M - 2: past the end
    rays_live = torch.tensor([[sum(live[:i]), c] for i, c in enumerate(live)], dtype=torch.int32)
    src_rows = torch.cat([torch.arange(o, o + c) for n, ((o, _), c) in enumerate(zip(rays.tolist(), live)) if n != 7])
    dst_rows = torch.cat([torch.arange(o, o + c) for n, (o, c) in enumerate(rays_live.tolist()) if n != 7])
    assert len(dst_rows) == M_live - 4
    rays, rays_live, src_rows, dst_rows = rays.cuda(), rays_live.cuda(), src_rows.cuda(), dst_rows.cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(9)

    def pair(width, dtype=torch.float32):
        shape = (M,) if width == 0 else (M, width)
        src = torch.randn(*shape, generator=g).to(dtype).cuda()
        dst = torch.full((M_live,) + shape[1:], -7.0, dtype=dtype, device="cuda")
        want = dst.clone()
        want[dst_rows] = src[src_rows]
        return src, dst, want

    for ch, f16, absent in [(3, False, ()), (4, False, ("ts",)), (3, True, ("xyzs", "sigmas")), (4, True, ()), (3, False, ("rgbs",))]:
        arrays = {"xyzs": pair(3), "ts": pair(2), "sigmas": pair(0), "rgbs": pair(ch, torch.float16 if f16 else torch.float32)}
        args = []
        for name in ("xyzs", "ts", "sigmas", "rgbs"):
            args += [None, None] if name in absent else [_lib.ptr(arrays[name][0]), _lib.ptr(arrays[name][1])]
        _lib.check(L.dwg_nerf_train_gather_live(_lib.ptr(rays), _lib.ptr(rays_live), N, M, M_live, *args, ch, int(f16), stream),
                   "dwg_nerf_train_gather_live")
        for name, (src, dst, want) in arrays.items():
            assert torch.equal(dst, torch.full_like(dst, -7.0) if name in absent else want), (ch, f16, name)
    for width in (6, 1):
        src, dst, want = pair(width)
        _lib.check(L.dwg_nerf_train_gather_live_rows(_lib.ptr(rays), _lib.ptr(rays_live), N, M, M_live, _lib.ptr(src), _lib.ptr(dst), width,
                                                     stream), "dwg_nerf_train_gather_live_rows")
        assert torch.equal(dst, want), width


def _bound_net(c, **kw):
    nerf.unbind_nerf_network(c.net)
    assert nerf.bind_nerf_network(c.net, **kw) is None
    return c.net


def _train_step(net, c, seed):
    """One training call of run_cuda and its backward -> (results, gradients, the step counter's state)."""
    net.train()
    net.local_step = 0
    with torch.no_grad():
        net.step_counter.fill_(5)
    torch.cuda.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.float16, enabled=c.f16):
        out = net.run_cuda(c.rays_o[None], c.rays_d[None], perturb=True, max_steps=tc.MAX_STEPS, T_thresh=tc.T_THRESH)
    names = [k for k in _params(net) if k != 'sigma_scale']
    grads = torch.autograd.grad([out["weights_sum"][0], out["depth"][0], out["image"][0]], [_params(net)[k] for k in names],
                                [c.g_ws, c.g_depth, c.g_image])
    net.eval()
    return out, dict(zip(names, grads)), (net.local_step, net.step_counter.clone())


@pytest.mark.parametrize("f16,latent", MODES)
def test_binding(f16, latent):
    c = _case(1000, f16, latent)
    ro, rd = c.rays_o[None], c.rays_d[None]
    try:
        net = _bound_net(c, shaded_render=True)
        want, want_grads, (step0, counter0) = _train_step(net, c, 21)
        assert net.run_calls[-1] == (True, 'albedo', True)               # without train_render a training call is the original's
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=f16):
            ev = [net.run_cuda(ro, rd, max_steps=tc.MAX_STEPS), net.run_cuda(ro, rd, shading='normal', max_steps=tc.MAX_STEPS)]

        net = _bound_net(c, shaded_render=True, train_render=True)
        del net.run_calls[:]
        got, got_grads, (step1, counter1) = _train_step(net, c, 21)
        assert net.run_calls == []                                       # the class method was not reached
        assert set(got) == {"image", "depth", "weights_sum", "mask", "weights", "xyzs", "sigmas", "rgbs"}
        for k in ("image", "depth", "weights_sum", "mask"):
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
        assert torch.equal(got["weights"], want["weights"]) and not got["weights"].requires_grad
        assert torch.equal(got["sigmas"], want["sigmas"]) and got["sigmas"].dtype == torch.float32 and not got["sigmas"].requires_grad
        assert got["xyzs"] is None and got["rgbs"] is None
        for k in want_grads:
            e = nc.rel_l2(got_grads[k], want_grads[k])
            assert e <= tc.F32_BWD, (k, e)
        # the step counter's statements: the row local_step % 16 is zeroed and local_step advances, as in the original; the march adds
        # its sample count into that row's first element, the other rows stay
        M = got["sigmas"].shape[0]
        assert step0 == step1 == 1
        assert counter0[0].tolist() == [0, 0] and counter1[0].tolist() == [M, 0]
        assert torch.equal(counter0[1:], counter1[1:]) and int((counter1[1:] != 5).sum()) == 0
        # eval() calls are the B14 / B15 results bit for bit
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=f16):
            ev1 = [net.run_cuda(ro, rd, max_steps=tc.MAX_STEPS), net.run_cuda(ro, rd, shading='normal', max_steps=tc.MAX_STEPS)]
        assert net.run_calls == []
        for a, b in zip(ev, ev1):
            for k in ("image", "depth", "weights_sum", "mask"):
                assert torch.equal(a[k], b[k]), k
        # calls the training render does not take go to the original
        net.train()
        with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
            net.run_cuda(ro, rd, shading='normal', max_steps=tc.MAX_STEPS)
        net.eval()
        assert net.run_calls == [(True, 'normal', False)]
        nerf.unbind_nerf_network(net)
        for name in ("run_cuda", "common_forward", "_dwg_train_render", "_dwg_shaded_render"):
            assert name not in net.__dict__, name
        net.train()
        net.run_cuda(ro, rd, max_steps=tc.MAX_STEPS)
        net.eval()
        assert net.run_calls[-1] == (True, 'albedo', False)
    finally:
        c.net.eval()
        nerf.unbind_nerf_network(c.net)
