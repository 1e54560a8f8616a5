"""GPU tests of the point-cloud export (boundary B12, dreamwaltz_g_amd.pointcloud): the order and the selection against the arrays recorded
from the reference's own functions (tests/golden/pointcloud_order.npz), bit-equality with the reference's export loop restated over the
bound test-local network (tests/pointcloud_cases.py), the exported set against the float64 restatement of the field, the edge cases of
the selection, the bounding boxes against the float64 loop, determinism, the binding and the hand-off to the avatar constructor's
nearest-triangle search.  Reads nothing of the reference."""
import types

import numpy as np
import pytest
import torch

from tests import nerf_field_cases as nc
from tests import pointcloud_cases as pcc

pytestmark = pytest.mark.gpu

F32_FWD = 5e-5          # the field's forward bound of tests/test_nerf_field_gpu.py: max |err| / max |ref| against float64
SHAPES = [(10, 4), (33, 16), (20, 128)]          # 27 chunks with a partial tile; chunk lengths 16, 16, 1 and 18 selection blocks; one chunk


def _pc():
    from dreamwaltz_g_amd import pointcloud
    return pointcloud


def _network(gridtype, interp, act, prior, latent, seed=3):
    return nc.make_network(gridtype=gridtype, interp=interp, density_activation=act, density_prior=prior, latent_mode=latent,
                           additional_dim_size=1 if latent else 0, seed=seed, log2_hashmap_size=15 if gridtype == 'hash' else 19).cuda()


def _field(net, precision=None):
    return _pc().field_spec(net.encoder, net.sigma_net, net.sigma_scale, net.bound, net.opt.density_activation, net.density_prior_type,
                            not net.latent_mode, precision)


def _export(net, R, split, thr, precision=None):
    return _pc().export_point_cloud(net.encoder, net.sigma_net, net.sigma_scale, net.bound, resolution=R, split_size=split, density_thresh=thr,
                                    density_activation=net.opt.density_activation, density_prior=net.density_prior_type,
                                    albedo_sigmoid=not net.latent_mode, precision=precision)


def _lattice(net, R, split, precision=None):
    """(sigma of the lattice pass, the lattice points, minmax partials) through the low-level functions."""
    pc = _pc()
    ax = pc.axis_table(R, "cuda")
    sigma, minmax = pc.lattice_sigma(*_field(net, precision), ax, ax, ax, min(split, R))
    pts = pc.lattice_points(torch.arange(R ** 3, dtype=torch.int32, device="cuda"), ax, ax, ax, min(split, R))
    return sigma, pts, minmax


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. order and selection against the recorded arrays
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["r10s4", "r5s8"])
def test_order_and_selection_match_the_recorded_reference(case):
    pc = _pc()
    fx = pcc.load_fixture()
    R, split = (int(v) for v in fx[case + ".resolution_split"])
    ax = pc.axis_table(R, "cuda")
    pts = pc.lattice_points(torch.arange(R ** 3, dtype=torch.int32, device="cuda"), ax, ax, ax, min(split, R))
    assert np.array_equal(pts.cpu().numpy(), fx[case + ".lattice"])
    sigma = torch.from_numpy(fx[case + ".sigma"]).cuda()
    idx, count = pc.select_above(sigma, float(fx["thresh"][0]))
    n = int(count.item())
    assert n == len(fx[case + ".points"])
    sel = pcc.u32(idx[:n])
    assert np.array_equal(pts[sel].cpu().numpy().astype(np.float64), fx[case + ".points"])
    assert np.array_equal(sigma[sel].cpu().numpy().astype(np.float64), fx[case + ".alphas"][:, 0])
    # the recorded cloud through outside_boxes + select_flags, and through remove_points_inside_bboxes on both containers
    cloud = pc.PointCloud(*(torch.from_numpy(fx[case + "." + k].astype(np.float32)).cuda() for k in ("points", "colors", "normals", "alphas")))
    keep = pc.outside_boxes(cloud.points, torch.from_numpy(pc.parse_boxes(fx["box"].tolist())).cuda())
    kidx, kcount = pc.select_flags(keep)
    kn = int(kcount.item())
    assert kn == len(fx[case + ".removed.points"])
    for k in ("points", "colors", "normals", "alphas"):
        assert np.array_equal(getattr(cloud, k)[pcc.u32(kidx[:kn])].cpu().numpy().astype(np.float64), fx[case + ".removed." + k]), k
    basic = cloud.to_basic()
    out = pc.remove_points_inside_bboxes(cloud, fx["box"].tolist())
    assert out is cloud and len(cloud) == kn and cloud.info["n_points"] == kn
    outb = pc.remove_points_inside_bboxes(basic, fx["box"].tolist())
    assert outb is basic
    for k in ("points", "colors", "normals", "alphas"):
        assert np.array_equal(getattr(cloud, k).cpu().numpy().astype(np.float64), fx[case + ".removed." + k]), k
        assert getattr(basic, k).dtype == np.float64 and np.array_equal(getattr(basic, k), fx[case + ".removed." + k]), k


def test_lattice_points_past_two_to_the_31():
    """Flat indices of a 1300^3 lattice (2.197e9 points): the decode's 32-bit products and the index's top bit."""
    pc = _pc()
    R, split = 1300, 256
    flat = [0, 1, 256 * R * R - 1, 256 * R * R, (1 << 31) - 1, 1 << 31, (1 << 31) + 12345, R ** 3 - 1301, R ** 3 - 1]
    ax = pc.axis_table(R, "cuda")
    idx32 = torch.from_numpy(np.array(flat, np.uint32).view(np.int32)).cuda()
    pts = pc.lattice_points(idx32, ax, ax, ax, split).cpu().numpy()
    axh = ax.cpu().numpy()
    want = np.array([[axh[i] for i in pc.lattice_index(f, R, R, R, split)] for f in flat], np.float32)
    assert np.array_equal(pts, want)
    # an index at or past the lattice reads nothing and writes NaN
    bad = pc.lattice_points(torch.from_numpy(np.array([R ** 3, 0xFFFFFFFF], np.uint32).view(np.int32)).cuda(), ax, ax, ax, split)
    assert torch.isnan(bad).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. bit-equality with the reference's loop over the bound network
# ------------------------------------------------------------------------------------------------------------------------------------
EXPORT_CASES = [
    # gridtype, interp, act, prior, latent, f16      (rows 2, 3, 4 and 1 of test_nerf_field_gpu.FWD_CASES)
    ('hash', 'smoothstep', 'softplus', 'gaussian', False, False),
    ('tiled', 'linear', 'scaling', 'sqrt', False, False),
    ('hash', 'linear', 'exp', 'gaussian', True, False),          # latent: four albedo channels through the colour matrix
    ('tiled', 'smoothstep', 'exp', 'none', False, True),
]


def _run_export_case(gridtype, interp, act, prior, latent, f16, R, split):
    from dreamwaltz_g_amd import nerf
    pc = _pc()
    net = _network(gridtype, interp, act, prior, latent)
    assert nerf.bind_nerf_network(net) is None
    with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
        sigma, pts, minmax = _lattice(net, R, split)
        thr = float(torch.quantile(sigma, 0.8))
        got = _export(net, R, split, thr)
        want = pcc.restate_export(net, R, split, thr)
        # the lattice pass is the forward kernel on the materialised points, bit for bit
        s_fwd, _ = pc.field_forward(*_field(net), pts)
    return net, got, want, sigma, s_fwd, minmax, thr


# the three f32 fields at the three shapes, and the one f16 case at the shape with several chunks and selection blocks
EXPORT_RUNS = [c + s for c in EXPORT_CASES[:3] for s in SHAPES] + [EXPORT_CASES[3] + (33, 16)]


@pytest.mark.parametrize("gridtype,interp,act,prior,latent,f16,R,split", EXPORT_RUNS)
def test_export_equals_the_reference_loop_over_the_bound_network(gridtype, interp, act, prior, latent, f16, R, split):
    net, got, want, sigma, s_fwd, minmax, thr = _run_export_case(gridtype, interp, act, prior, latent, f16, R, split)
    points, colors, normals, alphas, (lo, hi) = want
    assert torch.equal(sigma, s_fwd)
    n = points.shape[0]
    print("R", R, "split", split, "survivors", n, "of", R ** 3, "max |normal diff|",
          float((got.normals - normals).abs().max()) if n and got.normals.shape == normals.shape else None)
    assert 0 < n < R ** 3 and len(got) == n
    assert got.points.dtype == got.colors.dtype == got.normals.dtype == got.alphas.dtype == torch.float32
    assert got.alphas.shape == (n, 1) and got.colors.shape == (n, 3) and got.normals.shape == (n, 3)
    assert torch.equal(got.points, points)
    assert torch.equal(got.alphas, alphas)
    assert torch.equal(got.colors, colors)
    # the six densities are bit-equal; the summation order of three squares and the roundings of the square root and of the division
    # differ: a few ulp of values <= 1
    assert float((got.normals - normals).abs().max()) <= 1e-6
    assert got.info["n_lattice"] == R ** 3 and got.info["n_points"] == n and got.info["density_thresh"] == float(np.float32(thr))
    assert got.info["min_density"] == lo == float(sigma.min()) and got.info["max_density"] == hi == float(sigma.max())
    assert float(minmax[:, 0].min()) == lo and float(minmax[:, 1].max()) == hi


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. against float64
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,split", [(10, 4), (33, 16)])
@pytest.mark.parametrize("gridtype,interp,act,prior,q", [
    ('hash', 'smoothstep', 'softplus', 'gaussian', 0.8),
    ('tiled', 'smoothstep', 'exp', 'none', 0.8),
    ('tiled', 'linear', 'scaling', 'sqrt', 0.95),
])
def test_exported_set_against_float64(gridtype, interp, act, prior, q, R, split):
    pc = _pc()
    net = _network(gridtype, interp, act, prior, False, seed=3)
    sigma, pts, _ = _lattice(net, R, split)
    rs, ra, _ = nc.restate(net, pts.cpu().numpy())
    rs, ra = rs.detach(), ra.detach()
    thr = float(torch.quantile(rs, q))
    band = F32_FWD * float(rs.abs().max())
    share = float(((rs - thr).abs() <= band).double().mean())
    print("thr", thr, "band", band, "share inside the band", share)
    assert share <= 0.005                                   # the cap, on the oracle's side: the comparison below means something
    got = _export(net, R, split, thr)
    idx, count = pc.select_above(sigma, thr)
    sel = pcc.u32(idx[:int(count.item())]).cpu()
    assert torch.equal(got.points.cpu(), pts.cpu()[sel]) and torch.equal(got.alphas[:, 0].cpu(), sigma.cpu()[sel])
    exported = torch.zeros(R ** 3, dtype=torch.bool)
    exported[sel] = True
    assert bool(exported[rs > thr + band].all())            # every point clearly above is exported
    assert not bool(exported[rs < thr - band].any())        # no point clearly below is
    assert float((got.alphas[:, 0].cpu().double() - rs[sel]).abs().max()) <= band
    assert float((got.colors.cpu().double() - ra[sel]).abs().max()) <= F32_FWD * float(ra.abs().max())


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. edge cases
# ------------------------------------------------------------------------------------------------------------------------------------
def test_thresholds_outside_the_density_range():
    net = _network('tiled', 'smoothstep', 'exp', 'none', False)
    R, split = 10, 4
    sigma, pts, _ = _lattice(net, R, split)
    empty = _export(net, R, split, float(sigma.max()))      # strict: the maximum itself is not above the threshold
    assert [tuple(getattr(empty, k).shape) for k in ("points", "colors", "normals", "alphas")] == [(0, 3), (0, 3), (0, 3), (0, 1)]
    assert len(empty) == 0 and empty.info["n_points"] == 0 and empty.points.is_cuda and empty.alphas.dtype == torch.float32
    eb = empty.to_basic()
    assert len(eb) == 0 and eb.alphas.shape == (0, 1) and eb.alphas.dtype == np.float64
    full = _export(net, R, split, float(sigma.min()) - 1.0)
    assert len(full) == R ** 3 and torch.equal(full.points, pts) and torch.equal(full.alphas[:, 0], sigma)


@pytest.mark.parametrize("M", [1, 255, 2048, 2049, 5000, 2048 * 1024 + 5])
def test_select_above_sizes_nan_and_order(M):
    """One entry, a partial round, exactly one block, one entry more, three blocks with a partial one, and more blocks than the scan of
    the block counts takes at once (1024).  NaN is never selected, whatever the threshold."""
    pc = _pc()
    g = torch.Generator().manual_seed(M)
    v = torch.rand(M, generator=g)
    v[torch.rand(M, generator=g) < 0.05] = float('nan')
    v[-1] = 0.99
    v = v.cuda()
    for thr in (0.5, float('-inf')):
        idx, count = pc.select_above(v, thr)
        want = torch.nonzero(v > thr).flatten()
        assert int(count.item()) == want.numel()
        assert torch.equal(pcc.u32(idx[:want.numel()]), want)
        assert not torch.isnan(v[want]).any()
    flags = (v > 0.25).to(torch.uint8) * 3                  # any non-zero byte counts
    idx, count = pc.select_flags(flags)
    want = torch.nonzero(flags).flatten()
    assert int(count.item()) == want.numel() and torch.equal(pcc.u32(idx[:want.numel()]), want)


def test_select_above_compares_in_fp32_and_strictly():
    pc = _pc()
    v = torch.tensor([0.1, np.nextafter(np.float32(0.1), np.float32(1)), 4.5, float('inf'), float('nan')], dtype=torch.float32).cuda()
    idx, count = pc.select_above(v, 0.1)                    # float32(0.1) > 0.1 is False in torch: the threshold is rounded to fp32
    assert int(count.item()) == 3 and pcc.u32(idx[:3]).tolist() == [1, 2, 3]
    assert torch.equal(torch.nonzero(v > 0.1).flatten().cpu(), torch.tensor([1, 2, 3]))


def test_select_capacity_below_the_count():
    pc = _pc()
    v = torch.rand(5000, generator=torch.Generator().manual_seed(1)).cuda()
    want = torch.nonzero(v > 0.5).flatten()
    cap = 100
    assert want.numel() > cap
    guard = torch.full((cap + 64,), -7, dtype=torch.int32, device="cuda")
    L, lib = pc._lib.lib(), pc._lib
    ws = torch.empty(int(L.dwg_pc_select_workspace_bytes(5000)) // 4, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.check(L.dwg_pc_select_above(5000, lib.ptr(v), 0.5, lib.ptr(guard), cap, lib.ptr(count), lib.ptr(ws), ws.numel() * 4, None), "select")
    torch.cuda.synchronize()
    assert int(count.item()) == want.numel()                # the full count
    assert torch.equal(guard[:cap].long(), want[:cap]) and bool((guard[cap:] == -7).all())       # only the first `capacity` are written
    idx, count = pc.select_above(v, 0.5, capacity=cap)
    assert idx.numel() == cap and int(count.item()) == want.numel() and torch.equal(idx.long(), want[:cap])
    idx, count = pc.select_above(v, 0.5, capacity=0)
    assert idx.numel() == 0 and int(count.item()) == want.numel()


def test_fd_points_and_finish_against_their_torch_statements():
    pc = _pc()
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(1000, 3, generator=g) * 2 - 1)
    x[:10] = torch.tensor([1.0, -1.0, 0.9995])              # on the bound and within epsilon of it: the clamp acts
    x[10, 0] = float('nan')
    x = x.cuda()
    eps, bound = 1e-3, 1.0
    got = pc.fd_points(x, eps, bound)
    for s, d in enumerate(([eps, 0.0, 0.0], [-eps, 0.0, 0.0], [0.0, eps, 0.0], [0.0, -eps, 0.0], [0.0, 0.0, eps], [0.0, 0.0, -eps])):
        want = (x + torch.tensor([d], device="cuda")).clamp(-bound, bound)
        assert torch.equal(torch.nan_to_num(got[s], nan=123.0), torch.nan_to_num(want, nan=123.0)), s
    sig6 = torch.rand(6, 1000, generator=g).cuda() * 50
    sig6[:, 0] = 1.0                                        # a zero gradient: 0 / sqrt(1e-20)
    sig6[0, 1], sig6[1, 1] = float('inf'), float('inf')     # inf - inf
    sig6[2, 2] = float('inf')                               # an infinite component
    sig6[4, 3] = float('nan')
    sig6[:, 4] = torch.tensor([1e-14, 0.0, 0.0, 0.0, 0.0, 0.0])       # |v|^2 below 1e-20: the clamp of safe_normalize acts
    alb = torch.rand(1000, 3, generator=g).cuda()
    colors, normals = pc.finish(alb, sig6, eps)
    n = -0.5 * torch.stack([sig6[0] - sig6[1], sig6[2] - sig6[3], sig6[4] - sig6[5]], -1) / eps
    want = torch.nan_to_num(pcc.safe_normalize(n))
    assert torch.equal(colors, alb)
    assert torch.isfinite(normals).all() and float((normals - want).abs().max()) <= 1e-6
    assert normals[0].tolist() == [0.0, 0.0, 0.0] and normals[1, 0] == 0.0 and normals[3, 2] == 0.0
    lat = (torch.rand(1000, 4, generator=g) * 4 - 2).cuda()
    colors4, _ = pc.finish(lat, sig6, eps)
    ref = lat.double() @ torch.tensor(pcc.DECODE, dtype=torch.float32).double().cuda()
    # four products below 1 (half an ulp: 2^-25 each) and three partial sums below 2 (2^-24 each)
    assert float((colors4.double() - ref).abs().max()) <= 5 * 2.0 ** -24
    assert torch.equal(colors4, pcc.latent_to_rgb(lat))
    assert float((colors4 - lat.matmul(torch.tensor(pcc.DECODE, device="cuda"))).abs().max()) <= 2 * 5 * 2.0 ** -24       # the reference's own matmul


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. bounding boxes against the float64 loop
# ------------------------------------------------------------------------------------------------------------------------------------
def test_outside_boxes_against_the_float64_loop():
    pc = _pc()
    f01 = float(np.float32(0.1))                            # 0.100000001490116...: above the double 0.1
    boxes = [[[0.1, -0.5, -0.5], [0.5, 0.5, 0.25]],         # min corner 0.1: float32(0.1) is inside
             [[-0.75, 0.5, 0.1], [-1.0, -0.25, -0.5]]]      # corners in swapped order; max z 0.1: float32(0.1) is outside
    pts = [[0.1, 0.0, 0.0], [f01, 0.0, 0.0], [0.5, 0.0, 0.0], [0.3, -0.5, 0.0], [0.3, 0.5, 0.0], [0.3, 0.0, -0.5], [0.3, 0.0, 0.25],      # faces of box 0
           [0.3, 0.0, 0.2500001], [0.5000001, 0.0, 0.0], [0.3, -0.5000001, 0.0],                                                            # just outside it
           [-0.9, 0.0, f01], [-0.9, 0.0, 0.0999999], [-1.0, -0.25, -0.5], [-0.75, 0.5, 0.0], [-0.7499999, 0.0, 0.0],                      # box 1
           [0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [float('nan'), 0.0, 0.0]]
    g = np.random.RandomState(0)
    pts = np.concatenate([np.array(pts, np.float32), (g.rand(3000, 3) * 2.4 - 1.2).astype(np.float32)])
    x = torch.from_numpy(pts).cuda()
    keep = pc.outside_boxes(x, torch.from_numpy(pc.parse_boxes(boxes)).cuda()).cpu().numpy().astype(bool)
    mask, _ = pcc.remove_inside(pts.astype(np.float64), [], boxes)
    assert np.array_equal(keep, mask)
    assert not keep[1] and keep[10] and 0 < keep.sum() < len(keep)
    # overlapping boxes: a point in both goes once
    both = [[[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]], [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]]
    keep2 = pc.outside_boxes(x, torch.from_numpy(pc.parse_boxes(both)).cuda()).cpu().numpy().astype(bool)
    assert np.array_equal(keep2, pcc.remove_inside(pts.astype(np.float64), [], both)[0])
    assert not keep2[15]
    # no box keeps everything
    assert bool(pc.outside_boxes(x, torch.empty((0, 2, 3), dtype=torch.float64, device="cuda")).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. determinism, 7. binding, 8. hand-off
# ------------------------------------------------------------------------------------------------------------------------------------
def test_two_exports_are_bit_identical():
    net = _network('hash', 'smoothstep', 'softplus', 'gaussian', False)
    sigma, _, _ = _lattice(net, 33, 16)
    thr = float(torch.quantile(sigma, 0.8))
    a, b = _export(net, 33, 16, thr), _export(net, 33, 16, thr)
    assert len(a) > 0
    for k in ("points", "colors", "normals", "alphas"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_bound_export_returns_the_reference_container():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dropin"))
    import dwg_bind
    pc = _pc()
    net = _network('tiled', 'smoothstep', 'exp', 'none', False)
    sigma, _, _ = _lattice(net, 20, 128)
    thr = float(torch.quantile(sigma, 0.8))
    lines, state = [], {"updated": 0}
    # what the reference's preamble reads of its network
    net.update_extra_state = lambda: state.__setitem__("updated", state["updated"] + 1)
    net.grid_size, net.cuda_ray, net.mean_density, net.density_thresh, net.max_density = 20, True, thr, 2 * thr + 1, 1e9

    class BasicPointCloud(pc.BasicPointCloud):
        pass

    def unreachable(*a, **k):
        raise AssertionError("the reference path ran")
    mod = types.ModuleType("to_point_cloud_stand_in")
    mod.export_point_cloud, mod.remove_points_inside_bboxes = unreachable, unreachable
    mod.BasicPointCloud = BasicPointCloud
    mod.logger = types.SimpleNamespace(info=lines.append)
    dwg_bind._patch_pointcloud_module(mod)
    assert mod.export_point_cloud.__wrapped__ is unreachable and mod.remove_points_inside_bboxes.__wrapped__ is unreachable
    got = mod.export_point_cloud(net, split_size=128)                  # resolution and threshold from the network: min(mean_density, density_thresh)
    want = _export(net, 20, 128, thr).to_basic()
    assert isinstance(got, BasicPointCloud) and state["updated"] == 1 and len(got) == len(want) > 0
    for k in ("points", "colors", "normals", "alphas"):
        assert getattr(got, k).dtype == np.float64 and np.array_equal(getattr(got, k), getattr(want, k)), k
    assert lines[0] == 'Extracting point cloud from NeRF...' and lines[1] == 'Extracting point cloud done! Obtain %d points!' % len(want)
    assert lines[2] == '    density thresh: %s (%s ~ %s)' % (thr, float(sigma.min()), float(sigma.max()))
    box = [[-0.5, -0.5, -0.5], [0.5, 0.5, 0.1]]
    mask, kept = pcc.remove_inside(want.points, [want.points, want.alphas], box)
    out = mod.remove_points_inside_bboxes(got, box)
    assert out is got and np.array_equal(got.points, kept[0]) and np.array_equal(got.alphas, kept[1]) and 0 < len(got) < len(want)
    # a network the field kernels do not cover goes to the reference's function
    net.density_prior_type = 'smpl'
    with pytest.raises(AssertionError, match="reference path"):
        mod.export_point_cloud(net, split_size=128)


def test_points_feed_the_nearest_triangle_search_on_the_device():
    from dreamwaltz_g_amd import avatar_init
    from tests import avatar_init_cases as ac
    net = _network('tiled', 'smoothstep', 'exp', 'none', False)
    sigma, _, _ = _lattice(net, 20, 128)
    cloud = _export(net, 20, 128, float(torch.quantile(sigma, 0.8)))
    V, F = ac.make_sphere()
    n = len(cloud)
    assert n > 0 and cloud.points.is_cuda and cloud.points.is_contiguous()
    ntb = avatar_init.find_nearest_triangles(cloud.points, torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda())
    assert ntb['squared_distances'].shape == (n,) and ntb['squared_distances'].is_cuda
    assert ntb['barycentric_coords'].shape == (n, 3) and ntb['vertex_indices'].shape == (n, 3) and ntb['triangle_indices'].shape == (n,)
    assert int(ntb['triangle_indices'].min()) >= 0 and int(ntb['triangle_indices'].max()) < len(F)
    assert bool(torch.isfinite(ntb['squared_distances']).all())
