"""-m gpu tests of the avatar construction on the device (boundary B11: csrc/avatar_init.hip through the C-ABI, dreamwaltz_g_amd.avatar_init,
DreamWaltzG.from_point_cloud) against the float64 oracles of tests/avatar_init_cases.py."""
import functools

import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from tests import avatar_init_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _sphere():
    return ac.make_sphere()


@functools.lru_cache(maxsize=None)
def _cloud_knn(K):
    """Oracle neighbours of the uniform cloud (query = reference), shared by the KNN and the smoothing tests."""
    C = ac.uniform_cloud()
    return ac.knn(C, C, K)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. nearest triangles
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_nearest_triangles_interior_points():
    from dreamwaltz_g_amd import avatar_init as ai
    V, F = _sphere()
    assert V.shape == (288, 3) and F.shape == (528, 3)
    P, face, bary = ac.interior_points(V, F, 600)
    o = ac.nearest_triangles(P, V, F)
    # the oracle first: every point qualifies (its generating face, its generating barycentrics up to the fp32 rounding of the point
    # [6e-8 of a 0.1-sized face], and a clear runner-up)
    assert (o['face'] == face).all()
    assert np.abs(o['bary'] - bary).max() < 2e-6
    assert (o['runner_up_d2'] >= 1.037 * o['d2']).all()
    assert o['bary'].min() >= 0.1 - 2e-6 and np.abs(o['bary'][:, [0, 1, 2]] - o['bary'][:, [1, 2, 0]]).min() >= 0.02 - 4e-6
    r = ai.find_nearest_triangles(_t(P), _t(V), _t(F), device=DEV)
    assert set(r) == {'squared_distances', 'triangle_indices', 'vertex_indices', 'nearest_vertex_indices', 'barycentric_coords'}
    for k in ('triangle_indices', 'vertex_indices', 'nearest_vertex_indices'):
        assert r[k].dtype == torch.int64 and r[k].device.type == 'cpu', k
    for k in ('squared_distances', 'barycentric_coords'):
        assert r[k].dtype == torch.float32 and r[k].is_cuda, k
    assert (r['triangle_indices'].numpy() == o['face']).all()
    d2 = r['squared_distances'].cpu().double().numpy()
    assert (np.abs(d2 - o['d2']) <= 1e-6 * (1 + o['d2'])).all(), np.abs(d2 - o['d2']).max()
    b = r['barycentric_coords'].cpu().double().numpy()
    assert np.abs(b - o['bary']).max() <= 1e-4, np.abs(b - o['bary']).max()
    assert (r['vertex_indices'].numpy() == F[o['face']]).all()
    assert (r['nearest_vertex_indices'].numpy() == F[o['face'], np.argmin(o['bary'], 1)]).all()
    # default placement: the points' device
    assert ai.find_nearest_triangles(_t(P[:7]), _t(V), _t(F))['squared_distances'].is_cuda
    assert ai.find_nearest_triangles(_t(P[:7]), _t(V), _t(F), device='cpu')['barycentric_coords'].device.type == 'cpu'


def test_nearest_triangles_over_edges_and_corners():
    from dreamwaltz_g_amd import avatar_init as ai
    V, F = _sphere()
    P, feet = ac.edge_and_corner_points(V, F, 200)
    o = ac.nearest_triangles(P, V, F)
    # the oracle first: the closest point is the generating foot (up to the fp32 rounding of the point) and lies on an edge or a corner
    assert np.abs(o['closest'] - feet).max() < 1e-7 and np.abs(o['bary']).min(1).max() < 1e-6
    r = ai.find_nearest_triangles(_t(P), _t(V), _t(F))
    d2 = r['squared_distances'].cpu().double().numpy()
    assert (np.abs(d2 - o['d2']) <= 1e-6 * (1 + o['d2'])).all(), np.abs(d2 - o['d2']).max()
    vi, b = r['vertex_indices'].numpy(), r['barycentric_coords'].cpu().double().numpy()
    assert (vi == F[r['triangle_indices'].numpy()]).all()
    closest = np.einsum('nk,nkc->nc', b, V.astype(np.float64)[vi])
    assert np.abs(closest - o['closest']).max() <= 1e-5, np.abs(closest - o['closest']).max()
    assert np.abs(b.sum(1) - 1).max() <= 1e-6


def test_nearest_triangles_empty_and_single_face():
    from dreamwaltz_g_amd import avatar_init as ai
    V, F = _sphere()
    r = ai.find_nearest_triangles(torch.zeros(0, 3, device=DEV), _t(V), _t(F))
    assert r['triangle_indices'].shape == (0,) and r['vertex_indices'].shape == (0, 3) and r['barycentric_coords'].shape == (0, 3)
    assert r['squared_distances'].shape == (0,) and r['nearest_vertex_indices'].shape == (0,)
    V1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    F1 = np.array([[0, 1, 2]], np.int64)
    P = np.array([[0.2, 0.3, 0.5], [0.6, 0.1, -0.25], [-1, -1, 0], [2, 0, 1]], np.float32)
    o = ac.nearest_triangles(P, V1, F1)
    r = ai.find_nearest_triangles(_t(P), _t(V1), _t(F1))
    assert (r['triangle_indices'].numpy() == 0).all() and (r['vertex_indices'].numpy() == [0, 1, 2]).all()
    assert np.abs(r['squared_distances'].cpu().double().numpy() - o['d2']).max() <= 1e-6 * (1 + o['d2'].max())
    assert np.abs(r['barycentric_coords'].cpu().double().numpy() - o['bary']).max() <= 1e-6
    assert r['nearest_vertex_indices'].tolist() == [1, 2, 1, 0]      # argmin bary, the first minimum winning: (.5,.2,.3) (.3,.6,.1) (1,0,0) (0,1,0)


def test_barycentric_kernel_marks_missing_faces():
    from dreamwaltz_g_amd import avatar_init as ai
    V, F = _sphere()
    cp = torch.zeros(3, 3, device=DEV)
    cf = torch.tensor([-1, 5, 528], dtype=torch.int32, device=DEV)
    b, vi, nv = ai.barycentric(cp, cf, _t(V), _t(F, torch.int32))
    assert vi.cpu().tolist() == [[-1, -1, -1], F[5].tolist(), [-1, -1, -1]] and nv.cpu().tolist()[::2] == [-1, -1]
    assert float(b[0].abs().max()) == 0.0 and float(b[2].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. / 3. K nearest neighbours
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_knn_lattice_ties_are_ordered_by_index():
    from dreamwaltz_g_amd import avatar_init as ai
    L = ac.lattice(9, 1.0 / 64)
    assert L.shape == (729, 3)
    oi, od = ac.knn(L, L, 30)
    centre = 4 * 81 + 4 * 9 + 4
    assert (od[centre] * 4096 == [0] + [1] * 6 + [2] * 12 + [3] * 8 + [4] * 3).all()       # the 30th place falls inside the fourth shell
    idx, d2 = ai.knn(_t(L), _t(L), 30)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32
    assert (idx.cpu().numpy() == oi).all()
    assert (d2.cpu().numpy() == od.astype(np.float32)).all() and (od.astype(np.float32).astype(np.float64) == od).all()


def _check_knn_general(Q, R, K, oi, od):
    from dreamwaltz_g_amd import avatar_init as ai
    idx, d2 = ai.knn(_t(Q), _t(R), K)
    idx, d2 = idx.cpu().numpy(), d2.cpu().double().numpy()
    assert (np.abs(d2 - od[:, :K]) <= 1e-6 * od[:, :K]).all(), (np.abs(d2 - od[:, :K]) / np.maximum(od[:, :K], 1e-30)).max()
    assert (np.diff(d2, axis=1) >= 0).all()
    gaps = np.diff(od[:, :K + 2], axis=1) < 1e-5 * od[:, 1:K + 2]
    skip = gaps.any(1)
    assert skip.mean() <= 0.01, skip.mean()
    assert (idx[~skip] == oi[~skip, :K]).all()
    assert ((idx >= 0) & (idx < len(R))).all()
    return skip.mean()


def test_knn_uniform_cloud():
    C = ac.uniform_cloud(4096, 0)
    oi, od = _cloud_knn(10)
    _check_knn_general(C, C, 8, oi, od)
    assert (oi[:, 0] == np.arange(4096)).all()


def test_knn_query_differs_from_reference():
    g = torch.Generator().manual_seed(1)
    Q = (torch.rand(1000, 3, generator=g) * 2 - 1).numpy()
    R = (torch.rand(3000, 3, generator=g) * 2 - 1).numpy()
    oi, od = ac.knn(Q, R, 10)
    _check_knn_general(Q, R, 8, oi, od)


def test_knn_limits_and_knn_points_container():
    from dreamwaltz_g_amd import _lib, avatar_init as ai
    g = torch.Generator().manual_seed(2)
    R = (torch.rand(40, 3, generator=g) * 2 - 1)
    oi, od = ac.knn(R.numpy(), R.numpy(), 40)
    idx, d2 = ai.knn(R.to(DEV), R.to(DEV), 40)                         # K = Nr: every reference point, in order
    assert (np.sort(idx.cpu().numpy(), 1) == np.arange(40)).all()
    assert (np.abs(d2.cpu().double().numpy() - od) <= 1e-6 * od).all()
    big = (torch.rand(100, 3, generator=g) * 2 - 1).to(DEV)
    idx, _ = ai.knn(big, big, 64)
    assert (idx[:, 0].cpu().numpy() == np.arange(100)).all()
    L = _lib.lib()
    out_i, out_d = torch.empty(100, 65, dtype=torch.int32, device=DEV), torch.empty(100, 65, device=DEV)
    assert L.dwg_avinit_knn(100, _lib.ptr(big), 100, _lib.ptr(big), 65, _lib.ptr(out_i), _lib.ptr(out_d), None) == -1
    assert L.dwg_avinit_knn(40, _lib.ptr(big), 40, _lib.ptr(big), 41, _lib.ptr(out_i), _lib.ptr(out_d), None) == -1
    with pytest.raises(RuntimeError):
        ai.knn(big, big, 65)
    with pytest.raises(RuntimeError):
        ai.knn(big[:10], big[:10], 11)
    res = ai.knn_points(big[None], big[None, :50], K=3)
    assert type(res).__name__ == '_KNN' and res._fields == ('dists', 'idx', 'knn') and res.knn is None
    assert res.dists.shape == (1, 100, 3) and res.idx.shape == (1, 100, 3) and res.idx.dtype == torch.int64 and res.dists.is_cuda
    oi, _ = ac.knn(big.cpu().numpy(), big[:50].cpu().numpy(), 3)
    assert (res.idx[0].cpu().numpy() == oi).all()
    assert ai.knn_points(big[None], big[None], K=2, device='cpu').idx.device.type == 'cpu'


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. smoothing
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_smoothing_sweeps_against_float64():
    from dreamwaltz_g_amd import _lib, avatar_init as ai
    K, J, N = 8, 55, 4096
    C = _t(ac.uniform_cloud(N, 0))
    idx, d2 = ai.knn(C, C, K + 1)
    idx, d2 = idx[:, 1:].contiguous(), d2[:, 1:].contiguous()         # columns 1..8
    rng = np.random.default_rng(5)
    mesh_d2 = rng.uniform(1e-3, 5.1e-2, N).astype(np.float32)
    w0 = ac.sparse_table(N, J, seed=6)
    kw, u = ai.knn_weights(idx, d2, _t(mesh_d2), use_sqrt=True, low=0.15)
    # the oracle is fed the kernel's own fp32 neighbours and squared distances
    a64, u64 = ac.smoothing_weights(idx.cpu().numpy(), d2.cpu().numpy(), mesh_d2, use_sqrt=True, low=0.15)
    un = u.cpu().numpy()
    assert set(np.unique(un)) == {0.0, 1.0} and (un == u64).all() and 100 < (un == 0).sum() < N - 100
    assert np.abs(kw.cpu().double().numpy() - a64).max() <= (K + 3) * 2.0 ** -24
    L = _lib.lib()
    w_in = _t(w0)
    keep = w_in.clone()
    results = {}
    for n in (0, 1, 2, 7, 50):
        tmp, out = torch.full_like(w_in, 7.0), torch.full_like(w_in, 9.0)
        rc = L.dwg_avinit_smooth(N, J, K, _lib.ptr(idx), _lib.ptr(kw), _lib.ptr(u), _lib.ptr(w_in), _lib.ptr(tmp), _lib.ptr(out), n, None)
        assert rc == 0
        results[n] = out
        ref = ac.smooth(w0, idx.cpu().numpy(), a64, u64, n)
        err = np.abs(out.cpu().double().numpy() - ref).max()
        tol = n * (2 * K + 8) * 2.0 ** -24
        assert err <= tol, "n = %d sweeps: max |error| %.3e, bound %.3e" % (n, err, tol)
        assert torch.equal(out[u == 0], w_in[u == 0]), n              # fails for an in-place sweep or a skipped copy
        assert torch.equal(w_in, keep), n
        out2 = torch.empty_like(w_in)
        assert L.dwg_avinit_smooth(N, J, K, _lib.ptr(idx), _lib.ptr(kw), _lib.ptr(u), _lib.ptr(w_in), _lib.ptr(tmp), _lib.ptr(out2), n, None) == 0
        assert torch.equal(out, out2), n                              # two runs, the same bits
    assert torch.equal(results[0], w_in)
    assert not torch.equal(results[1], results[2])
    # the public function: odd and even sweep counts land in the returned tensor, without a caller-side scratch buffer
    for n in (1, 7, 50):
        assert torch.equal(ai.smooth_sweeps(w_in, idx, kw, u, n), results[n]), n
    assert torch.equal(ai.smooth_sweeps(w_in, idx, kw, u, 0), w_in)
    # a ramp between two thresholds, and the squared-distance form
    kw2, u2 = ai.knn_weights(idx, d2, _t(mesh_d2), use_sqrt=False, low=0.01, high=0.03)
    a2, uo2 = ac.smoothing_weights(idx.cpu().numpy(), d2.cpu().numpy(), mesh_d2, use_sqrt=False, low=0.01, high=0.03)
    # thresholds rounded to fp32 and three roundings on values <= 0.051, divided by the ramp's width
    assert np.abs(u2.cpu().double().numpy() - uo2).max() <= 8 * 2.0 ** -24 * 0.051 / 0.02 and ((uo2 > 0) & (uo2 < 1)).sum() > 100
    assert np.abs(kw2.cpu().double().numpy() - a2).max() <= (K + 3) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. initialize_lbs_weights end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [False, True])
def test_initialize_lbs_weights_end_to_end(smooth):
    from dreamwaltz_g_amd import avatar_init as ai
    V, F = _sphere()
    # 2000 shell points with ONE closest face: over a shared edge, or where a neighbouring face is closer by less than the distance kernel's
    # tie margin of 5e-7 (1 + d), the lowest face index wins there and the exact minimum in float64 -- with different closest points
    # ... and at least 2 mm off the mesh: the smoothing weights are 1 / distance, and fp32 resolves a distance d to about 6e-8 / d
    P = ac.shell_points(2800, seed=3)
    P = P[(ac.faces_within(P, V, F, 2e-6).sum(1) == 1) & (ac.nearest_triangles(P, V, F)['d2'] >= 0.002 ** 2)][:2000]
    assert len(P) == 2000
    table = ac.sparse_table(len(V), 55, seed=4)
    K, n = 6, 10
    o = ac.nearest_triangles(P, V, F)
    ref = ac.interp(table, F[o['face']], o['bary'])
    if smooth:
        oi, od = ac.knn(P, P, K + 1)
        a, u = ac.smoothing_weights(oi[:, 1:], od[:, 1:], o['d2'], use_sqrt=True, low=0.01)
        assert 100 < (u == 0).sum() < 1900
        ref = ac.smooth(ref, oi[:, 1:], a, u, n)
    ntb = ai.find_nearest_triangles(_t(P), _t(V), _t(F), device='cpu')         # the reference's placement
    got = ai.initialize_lbs_weights(_t(table), ntb, positions=_t(P), smooth=smooth, smooth_K=K, smooth_N=n)
    assert got.shape == (2000, 55) and got.dtype == torch.float32 and got.is_cuda
    # three corners x the barycentric bound of the nearest-triangle test (1e-4) on table entries <= 1, plus the sweeps' bound; a sweep is a
    # convex combination and does not amplify what it is given
    tol = 3e-4 + (n * (2 * K + 8) * 2.0 ** -24 if smooth else 0.0)
    err = np.abs(got.cpu().double().numpy() - ref).max()
    assert err <= tol, "max |error| %.3e, bound %.3e" % (err, tol)
    assert np.abs(got.sum(1).cpu().numpy() - 1).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. from_point_cloud
# ---------------------------------------------------------------------------------------------------------------------------------------
def _glbs_on_sphere():
    """The body of tests/test_animate_gpu.py (oracle.animate.SyntheticBody -> GeneralLinearBlendSkinning) with the sphere as its template."""
    from dreamwaltz_g_amd import avatar as av
    from oracle import animate as oa
    V, F = _sphere()
    body = oa.SyntheticBody(V=len(V), F_=len(F), seed=0)
    bd = {k: getattr(body, k) for k in ("v_template", "shapedirs", "expr_dirs", "posedirs", "J_regressor", "lbs_weights", "betas",
                                        "expression", "pose_mean", "jaw_pose", "leye_pose", "reye_pose")}
    bd["v_template"] = torch.from_numpy(V)
    bd = {k: v.to(DEV) for k, v in bd.items()}              # derived buffers (J_template, joint_shape_dirs) are computed where the tensors live;
    bd["parents"] = torch.from_numpy(body.parents)         # from_reference computes them on the device, and the bits are compared below
    return av.GeneralLinearBlendSkinning(bd).to(DEV), V, F


def test_from_point_cloud_builds_a_rendering_avatar():
    from dreamwaltz_g_amd import avatar as av, camera, configs, scene as sc, synth
    glbs, V, F = _glbs_on_sphere()
    cnl = dict(body_pose=torch.zeros(1, 63), global_orient=torch.zeros(1, 3), left_hand_pose=torch.zeros(1, 45),
               right_hand_pose=torch.zeros(1, 45), expression=torch.zeros(1, 100))
    # "hands": the first three bands of the sphere (faces 0..143 on the vertex rings 0..3)
    hand_faces = np.arange(144)
    hands = av.MeshBindingGaussianModel(torch.from_numpy(V[:96]), torch.from_numpy(F[:144]), torch.arange(96))
    hands.predefined_triangle_indices = torch.from_numpy(hand_faces)
    P = ac.shell_points(3000, seed=7, lo=0.002, hi=0.2)
    # keep the points whose prune decision does not hang on a closest-face tie across the hands' rim (over a shared edge two faces are
    # equally close, and which one wins is the distance kernel's tie rule) or on the threshold itself
    near = ac.faces_within(P, V, F, 2e-6)
    d = np.sqrt(ac.nearest_triangles(P, V, F)['d2'])
    clear = ~(near[:, :144].any(1) & near[:, 144:].any(1)) & (np.abs(d - 0.1) > 1e-5)
    assert clear.sum() >= 2900
    P, near = P[clear], near[clear]
    N0 = len(P)
    cfg = configs.TrainConfig(); cfg.device = DEV
    cfg.render.learn_scales, cfg.render.learn_quaternions, cfg.render.learn_lbs_weights = False, True, False
    cfg.render.init_scale = 0.002
    cfg.render.lbs_weight_smooth, cfg.render.lbs_weight_smooth_K, cfg.render.lbs_weight_smooth_N = True, 6, 5
    assert cfg.render.prune_points_close_to_mesh and cfg.render.prune_dists_close_to_mesh == 0.01
    # the oracle's prune: closest face among the hands' and closer than 10 x 0.01
    o = ac.nearest_triangles(P, V, F)
    pruned = np.isin(o['face'], hand_faces) & (o['d2'] < 0.1 ** 2)
    assert 100 < pruned.sum() < 1500
    a = av.DreamWaltzG.from_point_cloud(glbs, _t(P), _t(V), _t(F), cnl, {"hands": hands}, cfg=cfg)
    n = N0 - int(pruned.sum())
    assert a._n_points == n and a._positions.shape == (n, 3) and a._scales.shape == (n, 3) and a._quaternions.shape == (n, 4)
    assert a._lbs_weights.shape == (n, 55)
    assert a._positions.requires_grad and not a._scales.requires_grad and a._quaternions.requires_grad and not a._lbs_weights.requires_grad
    assert not a.learn_betas and a.init_scale == 0.002 and a.init_offset == cfg.render.init_offset
    assert torch.allclose(a.get_scales(), torch.full((n, 3), 0.002, device=DEV), rtol=1e-5, atol=0)
    assert torch.equal(a._quaternions.detach(), torch.tensor([1.0, 0, 0, 0], device=DEV).expand(n, 4))
    ntb = a.nearest_triangles_buffer
    assert all(ntb[k].shape[0] == n for k in ('squared_distances', 'triangle_indices', 'vertex_indices', 'nearest_vertex_indices',
                                               'barycentric_coords'))
    assert near[~pruned][np.arange(n), ntb['triangle_indices'].numpy()].all()          # a closest face, whichever of equally close ones
    kept = _t(P[~pruned])
    with torch.no_grad():
        back = a.lbs_transform(a._positions, a.lbs_model.forward(**a.smpl_canonical_inputs)[-1])
    assert float((back - kept).abs().max()) <= 1e-5, float((back - kept).abs().max())
    # a learn flag given by keyword overrides cfg
    b = av.DreamWaltzG.from_point_cloud(glbs, _t(P[:200]), _t(V), _t(F), cnl, None, cfg=cfg, learn_positions=False)
    assert b._n_points == 200 and not b._positions.requires_grad
    # it animates and renders
    cfg.render.bg_color = (0.5, 0.5, 0.5)
    scene = sc.Scene(cfg, a).to(DEV).eval()
    data = camera.make_camera(radius=2.0, azimuth=20.0, elevation=80.0, fovy=55.0, height=128, width=128, device=torch.device(DEV))
    pose = synth.random_smpl_inputs(seed=5, device=torch.device(DEV))
    with torch.no_grad():
        g = a.animate(pose)
        out = scene.forward(data, smpl_observed_inputs=pose, use_densifier=False, bg_mode=None)
    for f in ("positions", "opacities", "colors", "quaternions", "scales"):
        assert torch.isfinite(getattr(g, f)).all(), f
    assert g.positions.shape[0] == n + hands._n_points
    assert torch.isfinite(out["image"]).all() and float(out["alpha"].max()) > 0

    # an object with the reference avatar's attribute names carrying this avatar's tensors: from_reference renders the same bits
    class RefLike(torch.nn.Module):
        pass
    RefLike.__name__ = "DreamWaltzG"
    lbs = torch.nn.Module(); lbs.__class__ = type("GeneralLinearBlendSkinning", (torch.nn.Module,), {})
    for k in ("v_template", "posedirs", "J_regressor", "lbs_weights", "betas", "expression", "pose_mean", "jaw_pose", "leye_pose", "reye_pose"):
        setattr(lbs, k, torch.nn.Parameter(getattr(glbs, k).clone(), requires_grad=False))
    lbs.shapedirs = torch.nn.Parameter(glbs.shapedirs_all[..., :300].clone(), requires_grad=False)
    lbs.expr_dirs = torch.nn.Parameter(glbs.shapedirs_all[..., 300:].clone(), requires_grad=False)
    lbs.parents, lbs.use_smplx, lbs.NUM_BODY_JOINTS = glbs.parents.long(), True, 21
    ref = RefLike()
    ref.lbs_model, ref.deform_model = lbs, None
    for k in ("_positions", "_scales", "_quaternions", "_lbs_weights", "_betas"):
        setattr(ref, k, torch.nn.Parameter(getattr(a, k).detach().clone(), requires_grad=getattr(a, k).requires_grad))
    ref.smpl_canonical_inputs = a.smpl_canonical_inputs
    ref.register_buffer("nerf_bound", torch.tensor(2.0, device=DEV))
    ref.init_offset, ref.init_scale, ref.max_scale = a.init_offset, a.init_scale, a.max_scale
    ref.nerf_encoder, ref.nerf_opacity_and_color_net, ref.nerf_scale_and_quaternion_net = (
        a.nerf_encoder, a.nerf_opacity_and_color_net, a.nerf_scale_and_quaternion_net)
    ref.mesh_binding_gaussians = a.mesh_binding_gaussians
    ref.learn_hand_betas = ref.learn_face_betas = False
    ref.nearest_triangles_buffer = a.nearest_triangles_buffer
    ref.cfg = cfg
    adopted = av.DreamWaltzG.from_reference(ref)
    assert adopted is not a and adopted.nearest_triangles_buffer is a.nearest_triangles_buffer
    with torch.no_grad():
        h = adopted.animate(pose)
    for f in ("positions", "opacities", "colors", "quaternions", "scales"):
        assert torch.equal(getattr(g, f), getattr(h, f)), f
