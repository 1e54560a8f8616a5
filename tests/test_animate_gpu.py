"""-m gpu parity tests for the LBS stage and the grid encoder: HIP kernels (through the C-ABI) vs the CPU oracle.
fp32 tolerances: forward 2e-5 abs on O(1) values; gradients relative L2 <= 1e-4 (table gradients use fp32 atomics)."""
import numpy as np
import pytest
import torch

from oracle import animate as oa

pytestmark = pytest.mark.gpu


def _rel_l2(a, r):
    a = a.detach().double().cpu(); r = r.detach().double().cpu()
    return float((a - r).norm() / r.norm().clamp_min(1e-30))


def _skeleton(seed=0, J=55):
    g = torch.Generator().manual_seed(seed)
    pose = torch.randn(J, 3, generator=g) * 0.4
    pose[3] = 0.0  # exercises the |r + 1e-8| branch of Rodrigues
    joints = torch.randn(J, 3, generator=g) * 0.3
    parents = torch.tensor([-1] + [int(torch.randint(0, i, (1,), generator=g)) for i in range(1, J)])
    transl = torch.randn(3, generator=g) * 0.1
    return pose, joints, parents, transl


def _oracle_A(pose, joints, parents, transl):
    R = oa.batch_rodrigues(pose.double())
    _, A = oa.batch_rigid_transform(R[None], joints.double()[None], parents.numpy())
    if transl is not None:
        A = oa.se3_compose(A, oa.se3_from_T(transl.double()[None]))
    return A[0], R


@pytest.mark.parametrize("with_transl", [True, False])
def test_joint_chain(with_transl):
    from dreamwaltz_g_amd import lbs
    pose, joints, parents, transl = _skeleton()
    tr = transl if with_transl else None
    A_ref, R_ref = _oracle_A(pose, joints, parents, tr)
    A, R = lbs.joint_chain(pose.cuda(), joints.cuda(), parents, None if tr is None else tr.cuda(), return_rot_mats=True)
    assert (A.cpu().double() - A_ref).abs().max() < 2e-5
    assert (R.cpu().double() - R_ref).abs().max() < 2e-6


@pytest.mark.parametrize("N,with_q,normalize", [(1000, True, True), (257, True, False), (64, False, True), (1, True, True),
                                                (50000, True, True)])
def test_lbs_blend_forward_backward(N, with_q, normalize):
    from dreamwaltz_g_amd import lbs
    pose, joints, parents, transl = _skeleton(1)
    A_ref, _ = _oracle_A(pose, joints, parents, transl)
    g = torch.Generator().manual_seed(N)
    w_raw = torch.rand(N, 55, generator=g) * (torch.rand(N, 55, generator=g) < 0.2) + 1e-3
    p = torch.randn(N, 3, generator=g) * 0.4
    q = torch.randn(N, 4, generator=g)
    pd = p.double().requires_grad_(True); qd = q.double().requires_grad_(True)
    w = w_raw.double()
    wn = w / w.sum(-1, keepdim=True) if normalize else w
    po_ref = oa.transform_points(A_ref, pd, weights=wn)
    outs = [po_ref]
    if with_q:
        qo_ref = oa.transform_quaternions_flip(A_ref, qd, wn)
        outs.append(qo_ref)
    pc = p.cuda().requires_grad_(True); qc = q.cuda().requires_grad_(True)
    res = lbs.lbs_blend(A_ref.float().cuda(), w_raw.cuda(), pc, qc if with_q else None, normalize_weights=normalize)
    res = res if with_q else (res,)
    assert (res[0].detach().cpu().double() - po_ref.detach()).abs().max() < 2e-5
    if with_q:
        assert (res[1].detach().cpu().double() - qo_ref.detach()).abs().max() < 5e-5
    gs = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    grads_ref = torch.autograd.grad(outs, [pd, qd] if with_q else [pd], gs)
    torch.autograd.backward(list(res), [x.float().cuda() for x in gs])
    assert _rel_l2(pc.grad, grads_ref[0]) < 1e-4
    if with_q:
        assert _rel_l2(qc.grad, grads_ref[1]) < 1e-4


def test_vertex_transform_matches_transform_V():
    from dreamwaltz_g_amd import lbs
    body = oa.SyntheticBody(V=2000, F_=3000, seed=2)
    inp = oa.random_smpl_inputs(seed=4)
    _, tV, tr = oa.glbs_forward(body, **inp)
    g = torch.Generator().manual_seed(0)
    vi = torch.randperm(2000, generator=g)[:700]
    x = body.v_template[vi]
    ref = oa.transform_points(tV[0], x, indices=vi)
    full_shape = oa.glbs_full_shape(body, expression=inp["expression"])
    full_pose = oa.glbs_full_pose(body, **{k: v for k, v in inp.items() if k.endswith("pose") or k == "global_orient"})
    shapedirs = torch.cat([body.shapedirs, body.expr_dirs], -1)
    v_shaped = body.v_template + oa.blend_shapes(full_shape, shapedirs)[0]
    joints = torch.einsum('ik,ji->jk', v_shaped, body.J_regressor)
    A, R = lbs.joint_chain(full_pose.view(55, 3).cuda(), joints.cuda(), torch.from_numpy(body.parents), inp["transl"][0].cuda(),
                           return_rot_mats=True)
    subset = lbs.gather_vertex_subset(vi.cuda(), body.lbs_weights.cuda(), shapedirs.cuda(), body.posedirs.cuda())
    out = lbs.vertex_transform(x.cuda(), A, subset, full_shape.cuda(), R)
    assert (out.cpu() - ref).abs().max() < 2e-5


def _grid_case(B, seed, gridtype=1, oob=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, generator=g)
    if oob and B > 8:
        x[3] = torch.tensor([1.2, 0.5, 0.5]); x[5] = torch.tensor([0.5, -0.01, 0.5])
        x[6] = torch.tensor([0.0, 1.0, 0.5])  # boundary values are in range
    offsets, pls = oa.grid_offsets()
    table = (torch.rand(int(offsets[-1]), 2, generator=g) * 2 - 1) * 0.1
    return x, table, offsets, pls, gridtype


@pytest.mark.parametrize("B,gridtype", [(4096, 1), (1000, 0), (1, 1), (33, 1), (40000, 1)])   # 40000: atomics path with LDS coarse levels + slab path
def test_grid_encoder_forward_backward(B, gridtype, monkeypatch):
    from dreamwaltz_g_amd.gridencoder import grid_encode
    x, table, offsets, pls, _ = _grid_case(B, B, gridtype)
    xd = x.double().requires_grad_(True); td = table.double().requires_grad_(True)
    ref = oa.grid_encode(xd, td, offsets, pls, gridtype=gridtype)
    xc = x.cuda().requires_grad_(True); tc = table.cuda().requires_grad_(True)
    out = grid_encode(xc, tc, torch.from_numpy(offsets).cuda(), pls, 16, True, gridtype, False, 1)
    err = (out.detach().cpu().double() - ref.detach()).abs()
    # fp32 position arithmetic at the finest level (scale 4095: ulp(pos) = 2.4e-4 of a cell) against the float64 oracle:
    # |err| <= ulp * smoothstep' (1.5) * neighbour difference (<= 2 * 0.1 table amplitude) ~ 7e-5; the reference's table is
    # initialised to +-1e-4 (grid.py:142-144), i.e. 1000x smaller absolute errors in practice.  A floor() flip between
    # fma and mul+add evaluation moves a point to the neighbouring cell where the interpolant is continuous.
    assert err.max() < 7e-5, err.max()
    g = torch.Generator().manual_seed(1)
    go = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    gx_ref, gt_ref = torch.autograd.grad(ref, [xd, td], go)
    out.backward(go.float().cuda())
    assert _rel_l2(tc.grad, gt_ref) < 1e-4
    assert _rel_l2(xc.grad, gx_ref) < 2e-3   # d/dx is scaled by up to 4095 per level: fp32 cancellation
    if B >= 16384:
        # the two table-gradient paths (slab-binned [default], device-scope atomics with LDS-privatised coarse levels) agree, and a second
        # slab backward after the atomics one reproduces the first
        from dreamwaltz_g_amd import gridencoder as ge
        for mode in ("slabs", "device", "slabs"):
            with monkeypatch.context() as m:
                if mode == "device":
                    m.setattr(ge, "SLAB_MIN_POINTS", B + 1)
                tc.grad = None; xc.grad = None
                out2 = grid_encode(xc, tc, torch.from_numpy(offsets).cuda(), pls, 16, True, gridtype, False, 1)
                out2.backward(go.float().cuda())
            assert _rel_l2(tc.grad, gt_ref) < 1e-4, mode
            assert _rel_l2(xc.grad, gx_ref) < 2e-3, mode


@pytest.mark.parametrize("B", [20000, 100000])
def test_grid_encoder_table_gradient_is_bit_reproducible(B):
    """Round 5 (verdict round 4, item 7): the slab-binned table gradient sums every entry's contributions as 64-bit fixed-point integers
    (csrc/gridenc.hip gs_to_fixed) -- in LDS, and with integer atomics across the workgroups of the dense coarse slabs -- so the result does
    not depend on the order the atomics land in: repeated backwards give the SAME BITS (the reference's kernel, gridencoder.cu:245-337, adds
    floats atomically and does not), for overwrite and accumulate modes alike, and the values still match the float64 oracle."""
    from dreamwaltz_g_amd.gridencoder import grid_encode
    x, table, offsets, pls, _ = _grid_case(B, B, 0)
    xd = x.double().requires_grad_(True); td = table.double().requires_grad_(True)
    ref = oa.grid_encode(xd, td, offsets, pls, gridtype=0)
    go = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 1e-3      # SDS-sized gradients
    gt_ref = torch.autograd.grad(ref, [td], go)[0]
    xc = x.cuda().requires_grad_(True); tc = table.cuda().requires_grad_(True)
    grads = []
    for _ in range(4):
        tc.grad = None; xc.grad = None
        out = grid_encode(xc, tc, torch.from_numpy(offsets).cuda(), pls, 16, True, 0, False, 1)
        out.backward(go.float().cuda())
        grads.append(tc.grad.detach().clone())
    assert _rel_l2(grads[0], gt_ref) < 1e-4
    assert float(grads[0].abs().sum()) > 0
    for g in grads[1:]:
        assert torch.equal(g, grads[0])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_grid_encoder_fixed_point_gradient_keeps_a_non_finite_gradient_visible(bad):
    """Round 6 (advisor): the deterministic fixed-point accumulation converts floats to integers, which would turn a NaN / Inf incoming
    gradient into 0 or a saturated value.  The count pass flags it and the table gradient comes out non-finite, as the float-atomic path's
    (and the reference's atomicAdd, gridencoder.cu:245-337) does -- a GradScaler or the replica check can see it."""
    from dreamwaltz_g_amd.gridencoder import grid_encode
    B = 20000
    x, table, offsets, pls, _ = _grid_case(B, B, 0)
    xc = x.cuda().requires_grad_(True); tc = table.cuda().requires_grad_(True)
    out = grid_encode(xc, tc, torch.from_numpy(offsets).cuda(), pls, 16, True, 0, False, 1)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).cuda() * 1e-3
    go[B // 2, 7] = bad
    out.backward(go)
    assert not bool(torch.isfinite(tc.grad).all())
    # and a finite gradient right after it is finite again (no sticky state)
    tc.grad = None; xc.grad = None
    out = grid_encode(xc, tc, torch.from_numpy(offsets).cuda(), pls, 16, True, 0, False, 1)
    out.backward(torch.nan_to_num(go, nan=0.0, posinf=0.0))
    assert bool(torch.isfinite(tc.grad).all()) and float(tc.grad.abs().sum()) > 0


def test_grid_encoder_backend_layout_and_module():
    """[L,B,C] layout of the `_gridencoder` backend + the GridEncoder module mirror (bound=2 mapping, grid.py:149-165)."""
    from dreamwaltz_g_amd import gridencoder as ge
    x, table, offsets, pls, _ = _grid_case(512, 7)
    ref = oa.grid_encode(x.double(), table.double(), offsets, pls)
    outs = torch.empty(16, 512, 2, device="cuda")
    ge.grid_encode_forward(x.cuda(), table.cuda(), torch.from_numpy(offsets).cuda(), outs, 512, 3, 2, 16,
                           float(np.log2(pls)), 16, None, 1, False, 1, 0)
    got = outs.permute(1, 0, 2).reshape(512, 32).cpu().double()
    assert (got - ref).abs().max() < 7e-5
    enc = ge.GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                         desired_resolution=4096, gridtype='tiled', align_corners=False, interpolation='smoothstep').cuda()
    assert enc.embeddings.shape == (6328848, 2)
    pos = (torch.rand(100, 3) * 4 - 2)
    y = enc(pos.cuda(), bound=2)
    ref2 = oa.grid_encode(((pos + 2) / 4).double(), enc.embeddings.detach().cpu().double(), offsets, pls)
    assert (y.detach().cpu().double() - ref2).abs().max() < 1e-6


def _avatar_pair(N=3000, with_mesh=True, seed=0):
    """Builds the oracle inputs and the product avatar from the SAME tensors."""
    from dreamwaltz_g_amd import avatar as av
    body = oa.SyntheticBody(V=1500, F_=2500, seed=seed)
    nets = oa.init_avatar_networks(seed=seed, table_std=0.05)   # large table -> visible encoder signal
    g = torch.Generator().manual_seed(seed + 1)
    params = dict(_positions=(torch.rand(N, 3, generator=g) * 2 - 1) * torch.tensor([0.4, 0.9, 0.2]),
                  _scales=torch.log(torch.rand(N, 3, generator=g) * 0.018 + 0.002),
                  _quaternions=torch.randn(N, 4, generator=g),
                  _lbs_weights=torch.rand(N, 55, generator=g) * (torch.rand(N, 55, generator=g) < 0.1) + 1e-4)
    cnl = dict(body_pose=torch.zeros(1, 63), global_orient=torch.zeros(1, 3), left_hand_pose=torch.zeros(1, 45),
               right_hand_pose=torch.zeros(1, 45), expression=torch.zeros(1, 100))
    obs = oa.random_smpl_inputs(seed=seed + 2)
    mesh = None
    if with_mesh:
        vi = torch.randperm(body.V, generator=g)[:300]
        tri = torch.randint(0, 300, (200, 3), generator=g)
        tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
        base = torch.tensor([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12],
                             [5 / 12, 1 / 6, 5 / 12], [5 / 12, 5 / 12, 1 / 6]])
        bary = base.expand(tri.shape[0], -1, -1).clone() * (1 + 0.1 * torch.rand(tri.shape[0], 6, 3, generator=g))
        mesh = dict(vertex_indices=vi, triangles=tri, vertex_coords=body.v_template[vi], bary=bary,
                    scales=torch.rand(tri.shape[0] * 6, 3, generator=g) * 2.5)
    bd = {k: getattr(body, k) for k in ("v_template", "shapedirs", "expr_dirs", "posedirs", "J_regressor", "lbs_weights", "betas",
                                        "expression", "pose_mean", "jaw_pose", "leye_pose", "reye_pose")}
    bd["parents"] = torch.from_numpy(body.parents)
    glbs = av.GeneralLinearBlendSkinning(bd)
    mb = None
    if with_mesh:
        m = av.MeshBindingGaussianModel(mesh["vertex_coords"], mesh["triangles"], mesh["vertex_indices"])
        m._bary_coords.data.copy_(mesh["bary"]); m._scales.data.copy_(mesh["scales"])
        mb = {"hands": m}
    a = av.DreamWaltzG(glbs, params["_positions"], torch.exp(params["_scales"]), params["_quaternions"], params["_lbs_weights"],
                       {k: v.cuda() for k, v in cnl.items()}, mb)
    a.nerf_encoder.embeddings.data.copy_(nets["table"])
    for l in range(3):
        a.nerf_opacity_and_color_net.net[l].weight.data.copy_(nets["static_w"][l])
        a.nerf_opacity_and_color_net.net[l].bias.data.copy_(nets["static_b"][l])
    a.nerf_scale_and_quaternion_net.load_state_dict(nets["deform"])
    return a.cuda(), params, nets, body, obs, cnl, mesh


@pytest.mark.parametrize("with_mesh", [False, True])
def test_animate_matches_oracle_forward_and_backward(with_mesh):
    a, params, nets, body, obs, cnl, mesh = _avatar_pair(with_mesh=with_mesh)
    # oracle in float64 with autograd
    to64 = lambda d: {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}  # noqa: E731
    body64 = oa.SyntheticBody(V=1500, F_=2500, seed=0).to(torch.float64)
    p64 = {k: v.double().requires_grad_(k != "_lbs_weights") for k, v in params.items()}
    n64 = dict(offsets=nets["offsets"], per_level_scale=nets["per_level_scale"], table=nets["table"].double().requires_grad_(True),
               static_w=[w.double().requires_grad_(True) for w in nets["static_w"]],
               static_b=[b.double().requires_grad_(True) for b in nets["static_b"]],
               deform={k: v.double().requires_grad_(True) for k, v in nets["deform"].items()})
    m64 = None
    if mesh is not None:
        m64 = dict(mesh); m64["vertex_coords"] = mesh["vertex_coords"].double()
        m64["bary"] = mesh["bary"].double().requires_grad_(True); m64["scales"] = mesh["scales"].double().requires_grad_(True)
    ref = oa.animate(p64, n64, body64, to64(obs), to64(cnl), mesh=m64)
    out = a.animate({k: v.cuda() for k, v in obs.items()})
    tol = dict(positions=5e-5, opacities=2e-5, colors=2e-5, quaternions=2e-4, scales=2e-5)
    for k, t in tol.items():
        err = (out[k].detach().cpu().double() - ref[k].detach()).abs().max()
        assert err < t, (k, float(err))
    g = torch.Generator().manual_seed(9)
    gs = {k: torch.randn(ref[k].shape, generator=g, dtype=torch.float64) for k in tol}
    loss_ref = sum((ref[k] * gs[k]).sum() for k in tol)
    loss = sum((out[k] * gs[k].float().cuda()).sum() for k in tol)
    loss_ref.backward(); loss.backward()
    pairs = [("_positions", a._positions.grad, p64["_positions"].grad), ("_scales", a._scales.grad, p64["_scales"].grad),
             ("_quaternions", a._quaternions.grad, p64["_quaternions"].grad),
             ("table", a.nerf_encoder.embeddings.grad, n64["table"].grad)]
    for l in range(3):
        pairs.append(("static_w%d" % l, a.nerf_opacity_and_color_net.net[l].weight.grad, n64["static_w"][l].grad))
        pairs.append(("static_b%d" % l, a.nerf_opacity_and_color_net.net[l].bias.grad, n64["static_b"][l].grad))
    sd = dict(a.nerf_scale_and_quaternion_net.named_parameters())
    for k in ("layers.0.weight", "layers.0.bias", "layers.3.weight", "gaussian_warp.weight", "gaussian_scaling.bias"):
        pairs.append(("deform." + k, sd[k].grad, n64["deform"][k].grad))
    if mesh is not None:
        gm = a.mesh_binding_gaussians["hands"]
        pairs += [("bary", gm._bary_coords.grad, m64["bary"].grad), ("mesh_scales", gm._scales.grad, m64["scales"].grad)]
    for name, got, want in pairs:
        assert got is not None, name
        assert _rel_l2(got, want) < 2e-3, (name, _rel_l2(got, want))


def test_meshbind_kernels_match_oracle():
    """csrc/meshbind.hip through the C-ABI vs oracle/animate.py (compute_normal, mesh_positions, mesh_scales_and_quaternions)."""
    from dreamwaltz_g_amd import meshbind as mb
    g = torch.Generator().manual_seed(5)
    V, n_per = 500, 6
    verts_o = torch.randn(V, 3, generator=g) * 0.2
    verts_c = torch.randn(V, 3, generator=g) * 0.2
    tri = torch.randint(0, V, (700, 3), generator=g)
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    Fp = tri.shape[0]
    base = torch.tensor([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12],
                         [5 / 12, 1 / 6, 5 / 12], [5 / 12, 5 / 12, 1 / 6]])
    bary = base.expand(Fp, -1, -1) * (1 + 0.3 * torch.rand(Fp, 6, 3, generator=g))
    scales = torch.rand(Fp * n_per, 3, generator=g) * 2.5
    b64 = bary.double().requires_grad_(True); s64 = scales.double().requires_grad_(True)
    vn_ref, _ = oa.compute_normal(verts_o.double(), tri)
    cpos_ref = oa.mesh_positions(b64, verts_c.double(), tri)
    pos_ref = oa.mesh_positions(b64, verts_o.double(), tri)
    scl_ref, q_ref = oa.mesh_scales_and_quaternions(b64, s64, verts_o.double(), tri, pos_ref, n_per)
    off, faces = mb.build_vertex_face_csr(tri, V)
    tri32 = tri.to(torch.int32).cuda()
    vn = mb.vertex_normals(verts_o.cuda(), tri32, off.cuda(), faces.cuda())
    assert (vn.cpu().double() - vn_ref).abs().max() < 2e-6
    bg = bary.cuda().requires_grad_(True); sg = scales.cuda().requires_grad_(True)
    cpos, pos, scl, q = mb.meshbind(bg, sg, verts_c.cuda(), verts_o.cuda(), vn, tri32, n_per)
    for got, ref, tol in ((cpos, cpos_ref, 1e-6), (pos, pos_ref, 1e-6), (scl, scl_ref, 1e-6), (q, q_ref, 3e-5)):
        assert (got.detach().cpu().double() - ref.detach()).abs().max() < tol
    ws = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (cpos_ref, pos_ref, scl_ref, q_ref)]
    sum((t * w).sum() for t, w in zip((cpos_ref, pos_ref, scl_ref, q_ref), ws)).backward()
    sum((t * w.float().cuda()).sum() for t, w in zip((cpos, pos, scl, q), ws)).backward()
    assert _rel_l2(bg.grad, b64.grad) < 2e-4, _rel_l2(bg.grad, b64.grad)
    assert _rel_l2(sg.grad, s64.grad) < 1e-5
    # observed pass only (no canonical vertices): canonical output is empty and carries no gradient
    c2, p2, s2, q2 = mb.meshbind(bg, sg, None, verts_o.cuda(), vn, tri32, n_per)
    assert c2.numel() == 0 and torch.equal(p2, pos) and torch.equal(q2, q)


@pytest.mark.parametrize("B", [3000, 20000])          # 20000: the slab-binned table gradient behind the same contract
def test_gridencoder_dropin_backend_fp32_and_half_buffers(B):
    """dropin/_gridencoder.py as the reference's grid.py drives it (backend contract of src/bindings.cpp:5-9, [L,B,C] layout):
    fp32 buffers, and the HALF buffers grid.py allocates under autocast (embeddings / outputs / dy_dx / grad / grad_embeddings /
    grad_inputs in fp16, inputs fp32: grid.py:44-58,79-86) -- every buffer is written in its own dtype, nothing is reinterpreted."""
    import os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "dropin"))
    import _gridencoder as backend
    D, C, L = 3, 2, 16
    x, table, offsets, pls, _ = _grid_case(B, 11)
    S, H = float(np.log2(pls)), 16
    off = torch.from_numpy(offsets).cuda()
    ref = oa.grid_encode(x.double(), table.double(), offsets, pls)
    go = torch.randn(L, B, C, generator=torch.Generator().manual_seed(2))
    xd = x.double().requires_grad_(True); td = table.double().requires_grad_(True)
    refd = oa.grid_encode(xd, td, offsets, pls)
    gx_ref, gt_ref = torch.autograd.grad(refd, [xd, td], go.permute(1, 0, 2).reshape(B, L * C).double())
    for dt, tol_o, tol_g in ((torch.float32, 7e-5, 1e-4), (torch.float16, 2e-3, 2e-2)):
        emb = table.cuda().to(dt)
        out = torch.full((L, B, C), float("nan"), device="cuda", dtype=dt)
        dy = torch.empty(B, L * D * C, device="cuda", dtype=dt)
        guard = torch.full((1024,), 7.0, device="cuda", dtype=dt)       # a neighbour in the allocator: must stay untouched
        backend.grid_encode_forward(x.cuda(), emb, off, out, B, D, C, L, S, H, dy, 1, False, 1)
        got = out.float().permute(1, 0, 2).reshape(B, L * C).cpu().double()
        assert (got - ref).abs().max() < tol_o, (dt, float((got - ref).abs().max()))
        ge = torch.zeros_like(emb)
        ge[5, 0] = 3.0                                                    # the backend ACCUMULATES into the caller's buffer
        gi = torch.zeros(B, D, device="cuda", dtype=dt)
        backend.grid_encode_backward(go.cuda().to(dt), x.cuda(), emb, off, ge, B, D, C, L, S, H, dy, gi, 1, False, 1)
        assert ge.dtype == dt and gi.dtype == dt and torch.isfinite(ge.float()).all() and torch.isfinite(gi.float()).all()
        ge = ge.float(); ge[5, 0] -= 3.0
        assert _rel_l2(ge.float(), gt_ref) < tol_g, (dt, _rel_l2(ge.float(), gt_ref))
        assert _rel_l2(gi.float(), gx_ref) < max(tol_g, 5e-3), (dt, _rel_l2(gi.float(), gx_ref))
        assert bool((guard == 7.0).all())
    with pytest.raises(RuntimeError):
        backend.grid_encode_forward(x, table.cuda(), off, torch.empty(L, B, C, device="cuda"), B, D, C, L, S, H, None, 1, False, 1)   # CPU inputs
    with pytest.raises(RuntimeError):
        backend.grid_encode_forward(x.cuda(), table.cuda(), off, torch.empty(L, B + 1, C, device="cuda"), B, D, C, L, S, H, None, 1, False, 1)


def test_rasterizer_dropin_package_imports_and_renders():
    """dropin/diff_gaussian_rasterization: the names gaussian_renderer.py:5 imports, bound to the HIP rasterizer."""
    import os, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "dropin"))
    import diff_gaussian_rasterization as dgr
    from tests import raster_cases as rc
    sc = rc.make_scene(500, 64, 64, seed=4)
    t = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in sc.items()}
    rs = dgr.GaussianRasterizationSettings(image_height=64, image_width=64, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], bg=t["bg"],
                                           scale_modifier=1.0, viewmatrix=t["viewmatrix"], projmatrix=t["projmatrix"], sh_degree=3,
                                           campos=t["campos"], prefiltered=False, debug=False)
    img, radii, depth, alpha = dgr.GaussianRasterizer(raster_settings=rs)(
        means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), shs=None, colors_precomp=t["colors"], opacities=t["opacities"],
        scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
    ref = rc.oracle_forward(sc)
    assert img.shape == (3, 64, 64) and radii.dtype == torch.int32 and depth.shape == (1, 64, 64) and alpha.shape == (1, 64, 64)
    assert float((img.cpu() - torch.from_numpy(ref["color"])).abs().max()) < 1e-4
    with pytest.raises(Exception):
        dgr.GaussianRasterizer(raster_settings=rs)(means3D=t["means3D"], means2D=None, opacities=t["opacities"])   # neither SHs nor colours


def test_shape_gradient_entry_points_agree_and_repeat():
    """dwg_lbs_vertex_transform_backward_shape (library-owned workspace, the round-2 signature) == ..._ws (caller's workspace, what lbs.py
    calls), and both give the same bits on a second call: the sums are formed in a fixed order (round 6: no float atomics)."""
    import ctypes
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    Vp, J, S = 777, 55, 120
    A = torch.randn(J, 4, 4, generator=g).cuda()
    w = torch.rand(Vp, J, generator=g).cuda(); w = w / w.sum(-1, keepdim=True)
    sd = (torch.randn(Vp, 3, S, generator=g) * 0.01).cuda()
    go = torch.randn(Vp, 3, generator=g).cuda()
    pose = (torch.randn(J, 3, generator=g) * 0.3).cuda()
    parents = torch.tensor([-1] + [max(0, (j - 1) // 2) for j in range(1, J)], dtype=torch.int32).cuda()
    jd = (torch.randn(J, 3, S, generator=g) * 0.01).cuda()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = _lib.ptr
    outs = []
    for rep in range(2):
        gs0, sc0 = torch.empty(S, device="cuda"), torch.empty(J, 3, device="cuda")
        assert L.dwg_lbs_vertex_transform_backward_shape(Vp, J, S, p(A), p(w), p(sd), p(go), p(pose), p(parents), p(jd), p(sc0), p(gs0), st) == 0
        gs1, sc1 = torch.empty(S, device="cuda"), torch.empty(J, 3, device="cuda")
        ws = torch.empty(int(L.dwg_lbs_vertex_transform_backward_shape_workspace_floats(Vp)), device="cuda")
        assert L.dwg_lbs_vertex_transform_backward_shape_ws(Vp, J, S, p(A), p(w), p(sd), p(go), p(pose), p(parents), p(jd), p(sc1), p(gs1), p(ws), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(gs0, gs1) and torch.equal(sc0, sc1)
        outs.append(gs0.clone())
    assert torch.equal(outs[0], outs[1]) and float(outs[0].abs().max()) > 0
    # the first (vertex) term against plain torch: g_shape_v[l] = sum_v S_v[:, l] . (R_v^T g_v),  R_v = sum_j w_vj A_j[:3, :3]
    R = torch.einsum('vj,jrc->vrc', w.double(), A[:, :3, :3].double())
    gx = torch.einsum('vrc,vr->vc', R, go.double())
    first = torch.einsum('vcl,vc->l', sd.double(), gx)
    gAt = torch.einsum('vj,vc->jc', w.double(), go.double())
    assert torch.allclose(sc1.double(), gAt, rtol=1e-4, atol=1e-5)
    # the whole gradient against float64 autograd through the oracle: the first term above plus the chain term -- the shape moves the rest
    # joints, J = J_template + jdirs . beta, and with them the translation column of every A_j (this test's A is arbitrary, so its rotation
    # blocks stay as given and the chain supplies the translations; the gradient is linear in beta and does not depend on J_template or beta,
    # which are drawn here).  Bar as in test_vertex_gradients_gpu.py: 16 x the float32 oracle's own rel-L2 error, capped at 1e-4.
    J_template, beta0 = torch.randn(J, 3, generator=g) * 0.3, torch.randn(S, generator=g) * 0.5

    def g_shape_oracle(dt):
        beta = beta0.to(dt).requires_grad_(True)
        joints = J_template.to(dt) + torch.einsum('jcl,l->jc', jd.cpu().to(dt), beta)
        Rp = oa.batch_rodrigues(pose.cpu().to(dt))
        A_chain = oa.batch_rigid_transform(Rp[None], joints[None], parents.cpu().numpy())[1][0]
        SE3 = torch.cat([A.cpu().to(dt)[:, :, :3], A_chain[:, :, 3:]], dim=2)
        v = torch.einsum('vcl,l->vc', sd.cpu().to(dt), beta)
        out = oa.transform_points(SE3, v, weights=w.cpu().to(dt))
        return torch.autograd.grad(out, beta, go.cpu().to(dt))[0]

    g64, g32 = g_shape_oracle(torch.float64), g_shape_oracle(torch.float32)
    assert _rel_l2(g64 - first.cpu(), g64) > 1e-2                # (the chain term is a visible part of it)
    err, err32 = _rel_l2(gs1, g64), _rel_l2(g32, g64)
    print("g_shape rel-L2: kernel %.3e, float32 oracle %.3e" % (err, err32))
    assert err <= min(16.0 * err32, 1e-4), (err, err32)
