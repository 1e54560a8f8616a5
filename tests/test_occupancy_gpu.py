"""GPU tests of the occupancy-grid update (boundary B13, dreamwaltz_g_amd.occupancy): the cell points against the reference's torch
statements on the device and against the points recorded from the reference's own update_extra_state (tests/golden/occupancy.npz); the
density pass against the field kernel on the materialised points scattered by morton3D; the EMA, statistics, threshold and bitfield
against the recorded arrays and against the torch statements on the device, with planted invalid and NaN cells; the binding end to end
against the composition it replaces; determinism; no host synchronisation in update().  Reads nothing of the reference.

Sizes (grid_size, bound): (8, 1) one cascade of 8 tiles, fewer tiles than workgroups and one partial of the statistics; (8, 2) two
cascades; (16, 2) the recipe's cascade structure; (32, 3) three cascades, min(2 ** c, bound) clamps the last, 96 partials."""
import types

import numpy as np
import pytest
import torch

from tests import nerf_field_cases as nc
from tests import occupancy_cases as occ

pytestmark = pytest.mark.gpu

SHAPES = [(8, 1), (8, 2), (16, 2), (32, 3)]
FIELDS = [('tiled', 'linear', 'exp', 'none'), ('hash', 'smoothstep', 'softplus', 'gaussian')]


def _m():
    from dreamwaltz_g_amd import occupancy
    return occupancy


def _rm():
    from dreamwaltz_g_amd import raymarch
    return raymarch


_NETS = {}


def _network(gridtype, interp, act, prior, bound=2):
    """The test-local network of tests/test_pointcloud_gpu.py (seed 3), with the field's bound set to the grid's."""
    key = (gridtype, interp, act, prior, bound)
    if key not in _NETS:
        net = nc.make_network(gridtype=gridtype, interp=interp, density_activation=act, density_prior=prior, seed=3,
                              log2_hashmap_size=15 if gridtype == 'hash' else 19).cuda()
        net.bound = float(bound)
        _NETS[key] = net
    return _NETS[key]


def _field(net, precision=0):
    from dreamwaltz_g_amd import pointcloud
    return pointcloud.field_spec(net.encoder, net.sigma_net, net.sigma_scale, net.bound, net.opt.density_activation, net.density_prior_type,
                                 True, precision)


def _tables(H, bound):
    m = _m()
    C = m.cascades(bound)
    return (C, m.axis_table(H, "cuda")) + m.cascade_tables(bound, C, H, "cuda")


def _noise(C, H, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((C, H ** 3, 3), device="cuda", generator=g)


def _statement_points(noise, H, bound, C):
    """The reference's statements :108-128 on the device with the given draws (tests/occupancy_cases.restate_update, density unused)."""
    grid = torch.zeros((C, H ** 3), device="cuda")
    out = occ.restate_update(lambda x: {'sigma': torch.zeros(x.shape[0], device=x.device)}, noise, grid,
                             torch.zeros(C * H ** 3 // 8, dtype=torch.uint8, device="cuda"), H, bound, C, 10.0, _rm().morton3D, _rm().packbits)
    return out["points"]


def _morton(H):
    xs = torch.arange(H, dtype=torch.int32, device="cuda")
    coords = torch.stack(torch.meshgrid(xs, xs, xs, indexing='ij'), -1).reshape(-1, 3)
    return _rm().morton3D(coords).long()


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. points
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,bound", SHAPES)
def test_points_equal_the_torch_statements_on_the_device(H, bound):
    m = _m()
    C, axis, scale, half = _tables(H, bound)
    noise = _noise(C, H)
    got = m.lattice_points(axis, noise, scale, half)
    want = _statement_points(noise, H, bound, C)
    assert got.shape == (C, H ** 3, 3) and torch.equal(got, want)


def test_points_against_the_points_recorded_on_the_cpu():
    """The reference's statements evaluated on the CPU (the fixture) round 2 i / (H - 1) as a true division, torch on the device as a
    product with the inverse: one differently rounded division of a value <= 1, scaled by <= bound -> within 2 ulps of bound."""
    m = _m()
    fx = occ.load_fixture()
    worst = 0.0
    for name in ("first", "second", "above", "blob"):
        H, bound = int(fx[name + ".args"][0]), int(fx[name + ".args"][1])
        C, axis, scale, half = _tables(H, bound)
        got = m.lattice_points(axis, torch.from_numpy(fx[name + ".noise"]).cuda(), scale, half).cpu().numpy()
        worst = max(worst, float(np.abs(got.astype(np.float64) - fx[name + ".points"]).max()))
    ulp = float(np.spacing(np.float32(2.0)))
    print("max |device point - CPU-recorded point| = %.3e = %.2f ulps of bound" % (worst, worst / ulp))
    assert worst <= 2 * ulp


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. densities
# ------------------------------------------------------------------------------------------------------------------------------------
def _want_tmp(net, pts, H, precision):
    from dreamwaltz_g_amd import pointcloud
    C = pts.shape[0]
    s, _ = pointcloud.field_forward(*_field(net, precision), pts.reshape(-1, 3))
    want = torch.empty((C, H ** 3), device="cuda")
    want[:, _morton(H)] = s.view(C, H ** 3)
    return want, s.view(C, H ** 3)


DENSITY_RUNS = [f + s + (0,) for f in FIELDS for s in SHAPES] + [FIELDS[1] + (16, 2, 1)]


@pytest.mark.parametrize("gridtype,interp,act,prior,H,bound,precision", DENSITY_RUNS)
def test_density_pass_equals_the_field_kernel_on_the_materialised_points(gridtype, interp, act, prior, H, bound, precision):
    m = _m()
    net = _network(gridtype, interp, act, prior, bound)
    C, axis, scale, half = _tables(H, bound)
    noise = _noise(C, H, seed=5)
    pts = m.lattice_points(axis, noise, scale, half)
    got = m.lattice_sigma(*_field(net, precision), axis, noise, scale, half)
    want, _ = _want_tmp(net, pts, H, precision)
    assert torch.equal(got, want)


def test_density_pass_under_autocast_through_the_python_layer():
    m = _m()
    H, bound = 16, 2
    net = _network(*FIELDS[0], bound)
    grid = m.OccupancyGrid(H, bound, 10.0, device="cuda")
    noise = _noise(grid.cascade, H, seed=6)
    with torch.autocast("cuda", dtype=torch.float16):
        grid.update(net.encoder, net.sigma_net, net.sigma_scale, net.opt.density_activation, net.density_prior_type, noise=noise)
    want16 = m.lattice_sigma(*_field(net, 1), grid.axis, noise, grid.scale, grid.half)
    want32 = m.lattice_sigma(*_field(net, 0), grid.axis, noise, grid.scale, grid.half)
    assert torch.equal(grid.tmp_grid, want16) and not torch.equal(want16, want32)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(RuntimeError, match="fp16 autocast"):
            grid.update(net.encoder, net.sigma_net, net.sigma_scale, net.opt.density_activation, net.density_prior_type, noise=noise)


@pytest.mark.parametrize("H,bound", [(8, 1), (16, 2), (32, 3)])
def test_random_sigmas_adds_the_blob_of_the_torch_statement(H, bound):
    """sigmas += 1.0 * torch.exp(-(x ** 2).sum(-1) / (2 * 0.2 ** 2)) on the device.  Measured on an MI355X: BIT-EQUAL (the kernel's expf and
    torch.exp agree on every argument met, torch multiplies by the fp32 inverse of the scalar and sums the squares in order), so that
    is what is required; the issue's bound of 4 ulps of the added term is implied."""
    m = _m()
    net = _network(*FIELDS[1], bound)
    C, axis, scale, half = _tables(H, bound)
    noise = _noise(C, H, seed=7)
    pts = m.lattice_points(axis, noise, scale, half)
    got = m.lattice_sigma(*_field(net), axis, noise, scale, half, random_sigmas=True)
    _, s = _want_tmp(net, pts, H, 0)
    term = 1.0 * torch.exp(-(pts ** 2).sum(-1) / (2 * 0.2 ** 2))
    s = s.clone()
    s += term
    want = torch.empty_like(got)
    want[:, _morton(H)] = s
    tm = torch.empty_like(got)
    tm[:, _morton(H)] = term
    ulps = ((got.double() - want.double()).abs() / torch.from_numpy(np.spacing(tm.cpu().numpy().clip(1e-38))).cuda().double())
    print("cells that differ: %d of %d; max difference %.2f ulps of the added term" % (int((got != want).sum()), got.numel(), float(ulps.max())))
    assert float(tm.max()) > 0.5                # the blob is there
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. update against the recorded reference
# ------------------------------------------------------------------------------------------------------------------------------------
def _stats_dict(stats):
    raw = stats.cpu().numpy()
    return {"mean_density": float(raw[0]), "min": float(raw[1]), "max": float(raw[2]), "min_density": float(raw[3]), "max_density": float(raw[4]),
            "density_thresh": float(raw[5]), "valid_count": int(raw[6:8].view(np.uint32)[0]) | (int(raw[6:8].view(np.uint32)[1]) << 32)}


@pytest.mark.parametrize("name", ["first", "second", "above", "blob"])
def test_update_against_the_recorded_reference(name):
    m = _m()
    fx = occ.load_fixture()
    H, bound, thresh, decay, _ = fx[name + ".args"]
    H = int(H)
    grid = torch.from_numpy(fx[name + ".grid_before"].copy()).cuda()
    tmp = torch.from_numpy(fx[name + ".tmp"]).cuda()
    bits = torch.zeros(grid.numel() // 8, dtype=torch.uint8, device="cuda")
    got = _stats_dict(m.update_grid(grid, tmp, H, float(decay), float(thresh), bits))
    after = fx[name + ".grid_after"]
    assert np.array_equal(grid.cpu().numpy(), after)
    want = dict(zip(("mean_density", "min_density", "max_density", "density_thresh"), fx[name + ".stats"]))
    print(name, "mean rel", abs(got["mean_density"] - want["mean_density"]) / want["mean_density"], "log-min abs",
          abs(got["min_density"] - want["min_density"]), "log-max abs", abs(got["max_density"] - want["max_density"]))
    occ.check_stats(got, want, name)
    assert abs(got["min"] - float(after.min())) <= occ.REL_STATS * float(after.min()) and abs(got["max"] - float(after.max())) <= occ.REL_STATS * float(after.max())
    assert got["valid_count"] == after.size
    if want["density_thresh"] == thresh:
        assert got["density_thresh"] == float(np.float32(thresh))
    else:
        assert got["density_thresh"] == got["mean_density"]
    n = occ.bitfield_excuse(bits.cpu().numpy(), fx[name + ".bitfield"], after, got["density_thresh"], float(np.float32(want["density_thresh"])))
    print(name, "cells excused:", n)
    # the last stage on its own
    alone = m.packbits_dev(grid, torch.tensor([got["density_thresh"]], device="cuda"), torch.zeros_like(bits))
    assert torch.equal(alone, bits)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. update against the torch statements on the device, with planted cells
# ------------------------------------------------------------------------------------------------------------------------------------
def _planted(case):
    H, C = 32, 3
    g = torch.Generator(device="cuda").manual_seed(21)
    grid = torch.exp(torch.randn((C, H ** 3), device="cuda", generator=g) - 1.0)           # log-normal densities
    tmp = torch.exp(torch.randn((C, H ** 3), device="cuda", generator=g) - 1.0)
    thresh = 10.0
    if case in ("invalid", "nan_tmp"):
        grid.view(-1)[torch.arange(5, grid.numel(), 1013, device="cuda")] = -1.0               # never seen: left untouched, out of the statistics
        grid.view(-1)[torch.arange(9, grid.numel(), 4099, device="cuda")] = float("nan")       # NaN in the grid: not valid, left
    if case == "nan_tmp":
        tmp[1, 777] = float("nan")                                                              # at a valid cell
        assert bool(grid[1, 777] >= 0)
    if case == "zero":
        grid.zero_(); tmp.zero_()
    if case == "above":
        thresh = 0.01
    return H, C, grid, tmp, thresh


@pytest.mark.parametrize("case", ["plain", "invalid", "above", "zero", "nan_tmp"])
def test_update_against_the_torch_statements_on_the_device(case):
    m = _m()
    H, C, grid, tmp, thresh = _planted(case)
    ref_grid = grid.clone()
    want = occ.restate_ema(ref_grid, tmp, torch.zeros(C * H ** 3 // 8, dtype=torch.uint8, device="cuda"), thresh, _rm().packbits)
    bits = torch.zeros(C * H ** 3 // 8, dtype=torch.uint8, device="cuda")
    before = grid.clone()
    got = _stats_dict(m.update_grid(grid, tmp, H, 0.95, thresh, bits))
    invalid = ~(before >= 0)
    assert _bits_equal(grid[invalid], before[invalid])                       # -1 and NaN cells keep their bits
    assert got["valid_count"] == int((before >= 0).sum())
    if case == "nan_tmp":
        assert bool(torch.isnan(grid[1, 777])) and torch.equal(torch.isnan(grid), torch.isnan(ref_grid))
        keep = ~torch.isnan(grid)
        assert torch.equal(grid[keep], ref_grid[keep])
        assert all(np.isnan(got[k]) for k in ("mean_density", "min", "max", "min_density", "max_density", "density_thresh"))
        assert np.isnan(want["mean_density"]) and np.isnan(want["density_thresh"])
        assert int(bits.sum()) == 0 and int(want["bitfield"].sum()) == 0        # no bit is set
        return
    assert _bits_equal(grid, ref_grid)
    occ.check_stats(got, want, case)
    assert got["density_thresh"] == (float(np.float32(thresh)) if want["density_thresh"] == thresh else got["mean_density"])
    n = occ.bitfield_excuse(bits.cpu().numpy(), want["bitfield"].cpu().numpy(), grid.cpu().numpy(), got["density_thresh"],
                            float(np.float32(want["density_thresh"])))
    print(case, "mean", got["mean_density"], want["mean_density"], "cells excused:", n)
    if case == "zero":
        assert got["min_density"] == -15.0 and got["max_density"] == -15.0 and got["mean_density"] == 0.0 and int(bits.sum()) == 0
    if case == "above":
        assert want["density_thresh"] == thresh and int(bits.sum()) > 0


def test_stats_raises_the_reference_error_without_a_valid_cell():
    m = _m()
    net = _network(*FIELDS[0])
    grid = m.OccupancyGrid(8, 2, 10.0, device="cuda")
    grid.density_grid.fill_(-1.0)
    grid.update(net.encoder, net.sigma_net, net.sigma_scale, net.opt.density_activation, net.density_prior_type)
    with pytest.raises(RuntimeError, match=r"min\(\): Expected reduction dim"):
        grid.stats()
    with pytest.raises(RuntimeError, match=r"min\(\): Expected reduction dim"):
        torch.min(grid.density_grid[grid.density_grid >= 0])
    assert bool((grid.density_grid == -1).all()) and int(grid.density_bitfield.sum()) == 0
    assert grid.reset().iter_density == 0 and bool((grid.density_grid == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. end to end on a bound test-local network
# ------------------------------------------------------------------------------------------------------------------------------------
def _bound_pair():
    from dreamwaltz_g_amd import nerf
    nets = []
    for _ in range(2):
        net = occ.make_occ_network(16, bound=2, gridtype='hash', interp='smoothstep', density_activation='exp', density_prior='gaussian',
                                   density_thresh=10.0).cuda()
        assert nerf.bind_nerf_network(net) is None
        nets.append(net)
    native, composed = nets
    assert "update_extra_state" in native.__dict__ and native.update_extra_state.__wrapped__.__func__ is occ.OccNetwork.update_extra_state
    del composed.__dict__["update_extra_state"]             # the bound field under the class method: what the binding ran before
    return native, composed


def test_bound_update_extra_state_equals_the_composition_it_replaces():
    from dreamwaltz_g_amd import nerf
    rm = _rm()
    native, composed = _bound_pair()
    for net in (native, composed):
        torch.manual_seed(7)
        net.local_step = 3
        net.step_counter[:3, 0] = torch.tensor([10, 20, 33], dtype=torch.int32)
        net.update_extra_state()
        net.update_extra_state(random_sigmas=True)
    assert native.calls == [] and len(composed.calls) == 2
    assert torch.equal(native.density_grid, composed.density_grid)          # the same draws, the same field kernel
    assert native.iter_density == 2 and composed.iter_density == 2
    assert native.mean_count == composed.mean_count == 21 and native.local_step == 0
    occ.check_stats({k: getattr(native, k) for k in ("mean_density", "min_density", "max_density")},
                    {k: getattr(composed, k) for k in ("mean_density", "min_density", "max_density")}, "end to end")
    t_n, t_c = min(native.mean_density, native.density_thresh), min(composed.mean_density, composed.density_thresh)
    n = occ.bitfield_excuse(native.density_bitfield.cpu().numpy(), composed.density_bitfield.cpu().numpy(), native.density_grid.cpu().numpy(), t_n, t_c)
    print("mean", native.mean_density, composed.mean_density, "cells excused:", n)
    assert int(native.density_bitfield.sum()) > 0
    if n == 0:
        g = torch.Generator().manual_seed(3)
        N = 512
        rays_o = (torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 2.5])).cuda()
        d = torch.randn(N, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -1.0])
        rays_d = (d / d.norm(dim=-1, keepdim=True)).cuda()
        aabb = torch.tensor([-2.0, -2, -2, 2, 2, 2], device="cuda")
        nears, fars = rm.near_far_from_aabb(rays_o, rays_d, aabb, 0.2)
        outs = [rm.march_rays_train(rays_o, rays_d, 2.0, net.density_bitfield, net.cascade, net.grid_size, nears, fars) for net in (native, composed)]
        assert torch.equal(outs[0][3], outs[1][3]) and int(outs[0][3][:, 1].sum()) > 0      # identical sample counts per ray
    # a chunked call goes to the original method
    native.update_extra_state(S=4)
    assert native.calls == [(0.95, 4, False)]
    nerf.unbind_nerf_network(native)
    assert "update_extra_state" not in native.__dict__ and "_dwg_occupancy" not in native.__dict__
    native.update_extra_state()
    assert len(native.calls) == 2                                           # the class method shows through again


def test_bound_export_runs_the_native_update_once(monkeypatch):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dropin"))
    import dwg_bind
    from dreamwaltz_g_amd import pointcloud
    m = _m()
    native, _ = _bound_pair()
    count = {"n": 0}
    real = m.OccupancyGrid.update

    def counted(self, *a, **k):
        count["n"] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(m.OccupancyGrid, "update", counted)

    def unreachable(*a, **k):
        raise AssertionError("the reference path ran")
    mod = types.ModuleType("to_point_cloud_stand_in")
    mod.export_point_cloud, mod.remove_points_inside_bboxes = unreachable, unreachable
    mod.BasicPointCloud = pointcloud.BasicPointCloud
    mod.logger = types.SimpleNamespace(info=lambda s: None)
    dwg_bind._patch_pointcloud_module(mod)
    got = mod.export_point_cloud(native, split_size=128)
    assert count["n"] == 1 and native.calls == [] and native.iter_density == 1 and native.mean_density > 0
    assert isinstance(got, pointcloud.BasicPointCloud)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. determinism, 7. no host synchronisation
# ------------------------------------------------------------------------------------------------------------------------------------
def test_two_updates_from_the_same_state_are_bit_identical():
    m = _m()
    H, bound = 32, 3
    net = _network(*FIELDS[1], bound)
    start = torch.exp(torch.randn((3, H ** 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) - 1.0)
    outs = []
    for _ in range(2):
        grid = m.OccupancyGrid(H, bound, 10.0, device="cuda")
        grid.density_grid.copy_(start)
        g = torch.Generator(device="cuda").manual_seed(99)
        grid.update(net.encoder, net.sigma_net, net.sigma_scale, net.opt.density_activation, net.density_prior_type, generator=g)
        outs.append((grid.density_grid.clone(), grid.density_bitfield.clone(), grid.stats_dev.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and _bits_equal(outs[0][2], outs[1][2])
    assert not torch.equal(outs[0][0], start)


def test_update_makes_no_host_synchronisation():
    m = _m()
    net = _network(*FIELDS[0])
    grid = m.OccupancyGrid(16, 2, 10.0, device="cuda")
    grid.update(net.encoder, net.sigma_net, net.sigma_scale, net.opt.density_activation, net.density_prior_type)      # caches the encoder's host offsets
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            grid.stats_dev.sum().item()              # this torch build honours the mode
        grid.update(net.encoder, net.sigma_net, net.sigma_scale, net.opt.density_activation, net.density_prior_type)
        grid.update(net.encoder, net.sigma_net, net.sigma_scale, net.opt.density_activation, net.density_prior_type, random_sigmas=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert grid.iter_density == 3 and grid.stats()["mean_density"] > 0
