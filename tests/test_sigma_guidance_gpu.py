"""GPU parity of the sigma guidance geometry (boundary B8, dreamwaltz_g_amd.sigma_guidance) against the float64 restatement of
tests/sigma_guidance_cases.py on the same draws, and of calc_sigma_loss on a fake trainer against a float64 composition of the
reference's loss formulas on the same points and mask.  Synthetic meshes only; reads nothing of the reference."""
import math
import types

import numpy as np
import pytest
import torch

from tests import nerf_field_cases as nc
from tests import sigma_guidance_cases as sc

pytestmark = pytest.mark.gpu


def _sg():
    from dreamwaltz_g_amd import sigma_guidance as sg
    return sg


_MESH = {}


def _mesh():
    """Icosphere level 5 (+ 4 degenerate faces), its cap part (z > 0.2) with a ring of wrist faces."""
    if not _MESH:
        V, F = sc.make_icosphere(5)
        pf, wf = sc.make_part(V, F)
        Vd, Fd = sc.add_degenerate(V, F)
        _MESH.update(V=V, F=F, pf=pf, wf=wf, Vd=Vd, Fd=Fd)
    return _MESH


def _part(V, faces, wrist=None):
    return _sg().PartMesh(faces, len(V), "cuda", wrist=wrist)


def _draws(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((n, 4), dtype=torch.float64, device="cuda", generator=g)


# --------------------------------------------------------------------------------------------------------------------------------------
# geometry
# --------------------------------------------------------------------------------------------------------------------------------------
def test_vertex_normals_of_the_part_match_float64():
    m = _mesh()
    V, F, pf = m['V'], m['F'], m['pf']
    Vt = torch.from_numpy(V).cuda()
    _, _, vn = _sg()._prepare(Vt, _part(V, F[pf]))
    ref = sc.vertex_normals(V, F[pf])
    err = float((vn.double().cpu() - ref).abs().max())
    assert err <= 1e-5, err
    whole = sc.vertex_normals(V, F)
    used = np.unique(F[pf].reshape(-1))
    moved = used[(whole[used] - ref[used]).norm(dim=1).numpy() > 1e-3]
    assert len(moved) > 50                                          # part-boundary vertices: their whole-mesh normal differs
    assert float((vn.double().cpu()[moved] - ref[moved]).abs().max()) <= 1e-5
    unused = np.setdiff1d(np.arange(len(V)), used)
    assert float(vn[torch.from_numpy(unused).cuda()].abs().max()) == 0.0


def test_samples_match_float64_on_the_same_draws():
    m = _mesh()
    V, F, pf = m['V'], m['F'], m['pf']
    sg = _sg()
    Vt = torch.from_numpy(V).cuda()
    part = _part(V, F[pf])
    n = 200000
    draws = _draws(n, 7)
    _, cdf, vn = sg._prepare(Vt, part)
    pts, fid, pn, noisy = sg._sample(Vt, part, cdf, vn, draws, 0.05)
    rp, rf, rn, rnoisy = sc.sample(Vt.double(), torch.from_numpy(F[pf]).cuda(), draws, 0.05)
    cdf64 = sc.area_cdf(Vt.double(), torch.from_numpy(F[pf]).cuda())
    assert float((cdf - cdf64).abs().max()) <= 1e-12 * float(cdf64[-1])
    same = fid.long() == rf
    assert float(same.double().mean()) >= 0.999
    bad = torch.nonzero(~same).flatten()
    if len(bad):                                                     # every mismatch sits on a CDF boundary, and picks a neighbour
        lo = torch.minimum(fid.long()[bad], rf[bad])
        assert int((fid.long()[bad] - rf[bad]).abs().max()) == 1
        x = draws[bad, 0] * cdf64[-1]
        assert float((cdf64[lo] - x).abs().max()) <= 1e-6 * float(cdf64[-1])
    s = same
    assert float((pts.double()[s] - rp[s]).abs().max()) <= 1e-6
    assert float((noisy.double()[s] - rnoisy[s]).abs().max()) <= 1e-6
    assert float((pn.double()[s] - rn[s]).abs().max()) <= 1e-5
    assert fid.dtype == torch.int32 and int(fid.min()) >= 0 and int(fid.max()) < len(pf)


def test_sample_distribution_follows_the_areas():
    """2 M draws: face frequencies against the area weights (chi-square, Wilson-Hilferty normal approximation of the p-value), and
    mean barycentrics of the points in their faces within 1e-3 of 1/3."""
    m = _mesh()
    V, F, pf = m['V'], m['F'], m['pf']
    sg = _sg()
    Vt, Ft = torch.from_numpy(V).cuda(), torch.from_numpy(F[pf]).cuda()
    torch.manual_seed(1234)
    n = 2000000
    pts, fid, pn = sg.sample_surface(Vt, Ft, n)
    area = sc.face_areas(Vt.double(), Ft)
    expect = area / area.sum() * n
    counts = torch.bincount(fid, minlength=len(pf)).double()
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    k = len(pf) - 1
    z = ((chi2 / k) ** (1.0 / 3) - (1 - 2.0 / (9 * k))) / math.sqrt(2.0 / (9 * k))
    p = 0.5 * math.erfc(z / math.sqrt(2))
    assert p > 1e-3, (chi2, k, p)
    v0, e0, e1 = sc.face_frames(Vt.double(), Ft)
    ap = pts.double() - v0[fid]
    a, b = e0[fid], e1[fid]
    aa, bb, ab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    r0, r1 = (a * ap).sum(1), (b * ap).sum(1)
    det = aa * bb - ab * ab
    v, w = (bb * r0 - ab * r1) / det, (aa * r1 - ab * r0) / det
    lam = torch.stack([1 - v - w, v, w], 1)
    assert float(lam.min()) >= -1e-4 and float(lam.max()) <= 1 + 1e-4
    assert float((lam.mean(0) - 1.0 / 3).abs().max()) <= 1e-3, lam.mean(0)
    assert float((pn.norm(dim=1) - 1).abs().max()) <= 1e-5


def _distance_points(V, F, n=10000, seed=3):
    """Offsets 0 .. 0.05 along the normals of surface samples (both sides), uniform points in a box, points exactly on vertices and on
    edge midpoints, points near the degenerate faces, and a far point."""
    r = np.random.RandomState(seed)
    Vt, Ft = torch.from_numpy(V).double(), torch.from_numpy(F[:20480])
    k = n // 4
    p, _, pn, _ = sc.sample(Vt, Ft, r.rand(k, 4))
    off = torch.from_numpy(r.rand(k) * 0.1 - 0.05)
    along = p + off[:, None] * pn
    box = torch.from_numpy(r.rand(k, 3) * 2.6 - 1.3)
    on_v = Vt[torch.from_numpy(r.randint(0, 10242, k // 2))]
    e = Ft[torch.from_numpy(r.randint(0, 20480, k // 2))]
    on_e = ((Vt[e[:, 0]].float() + Vt[e[:, 1]].float()) * 0.5).double()
    rest = n - 2 * k - 2 * (k // 2) - 1
    deg = Vt[-3:][torch.from_numpy(r.randint(0, 3, rest))] + torch.from_numpy(r.randn(rest, 3) * 0.02)
    far = torch.tensor([[7.0, -3.0, 5.0]], dtype=torch.float64)
    return torch.cat([along, box, on_v, on_e, deg, far]).float()


def test_point_mesh_distance_matches_float64_brute_force():
    m = _mesh()
    V, F = m['Vd'], m['Fd']
    sg = _sg()
    P = _distance_points(V, F).cuda()
    Vt, Ft = torch.from_numpy(V).cuda(), torch.from_numpy(F).cuda()
    d2, I, C = sg.point_mesh_squared_distance(P, Vt, Ft)
    assert d2.dtype == torch.float32 and I.dtype == torch.int64 and C.shape == P.shape
    D = sc.all_face_distances(P.double(), Vt.double(), Ft, chunk=128)             # [N, F] float64
    dmin, imin = D.min(dim=1)
    scale = dmin.clamp_min(1.0)
    d = d2.double().sqrt()
    assert float(((d - dmin).abs() / scale).max()) <= 2e-6
    # the closest point is the float64 closest point of the returned face
    d2f, q = sc.point_face_d2(P.double(), Vt.double(), Ft, I)
    assert float(((C.double() - q).abs().max(dim=1).values / scale).max()) <= 2e-6
    # the returned face is within 1e-6 of the minimum, and no face of lower index attains the float64 minimum exactly (genuine ties:
    # shared edges and vertices) -- up to 0.1 % of the points, where the fp32 order of two near-equal candidates differs
    dI = D.gather(1, I[:, None]).squeeze(1)
    assert float(((dI - dmin) / scale).max()) <= 1e-6
    tie = D <= (dmin + 1e-12 * scale)[:, None]
    idx = torch.arange(D.shape[1], device=D.device)[None].expand_as(D)
    lowest_tie = torch.where(tie, idx, torch.full_like(idx, D.shape[1])).min(dim=1).values
    late = int((I > lowest_tie).sum())
    assert late <= 0.001 * len(P), late


@pytest.mark.parametrize("wo_wrist", [True, False])
def test_keep_mask_matches_float64(wo_wrist):
    m = _mesh()
    V, F, pf, wf = m['V'], m['F'], m['pf'], m['wf']
    sg = _sg()
    Vt = torch.from_numpy(V).cuda()
    wrist = np.isin(pf, wf)
    part = _part(V, F[pf], wrist)
    n, thick = 20000, 0.005
    draws = _draws(n, 11)
    g = sg.guidance_points(Vt, part, draws, 0.05, thick, wo_wrist=wo_wrist)
    Ft = torch.from_numpy(F[pf]).cuda()
    D = sc.all_face_distances(g['noisy'].double(), Vt.double(), Ft, chunk=128)
    dmin = D.min(dim=1).values
    # the tie rule: the lowest index among the faces at the float64 minimum (shared edges and vertices tie exactly)
    idx = torch.arange(D.shape[1], device=D.device)[None].expand_as(D)
    tie = D <= (dmin + 1e-12)[:, None]
    lowest = torch.where(tie, idx, torch.full_like(idx, D.shape[1])).min(dim=1).values
    ref = sc.keep_mask(dmin ** 2, lowest, thick, wrist if wo_wrist else None)
    keep = g['keep'] > 0
    wt = torch.from_numpy(wrist).cuda()
    # exempt: within 1e-5 of the threshold, or a face within 1e-6 of the minimum (but not tied with it) whose wrist flag differs from
    # the tie rule's face -- fp32 may pick either
    near = (D <= (dmin + 1e-6)[:, None]) & ~tie
    mixed = (near & (wt[None] != wt[lowest][:, None])).any(1) if wo_wrist else torch.zeros_like(keep)
    exempt = ((dmin - thick).abs() <= 1e-5) | mixed
    differ = keep != ref
    assert bool((~differ)[~exempt].all()), int((differ & ~exempt).sum())
    assert int(differ.sum()) <= 0.001 * n, int(differ.sum())
    # the exempt set itself: the 1e-5 band alone holds ~0.08 % of the points at this noise range (|offset| is uniform on [0, 0.025],
    # so 2e-5 / 0.025 of them), and the wrist ring's boundary adds near ties
    assert int(exempt.sum()) <= 0.0025 * n, int(exempt.sum())
    assert int(g['kept']) == int(keep.sum())
    assert 0.5 * n < int(keep.sum()) < n
    if wo_wrist:
        assert int((wt[g['closest_face'].long()] & keep).sum()) == 0


# --------------------------------------------------------------------------------------------------------------------------------------
# the whole call
# --------------------------------------------------------------------------------------------------------------------------------------
class _SMPLStub:
    def __init__(self, faces, part_fids, wrist_fids):
        self.model = types.SimpleNamespace(faces=faces)
        self.part_fids, self.wrist_fids = part_fids, wrist_fids

    def get_semantic_indices(self, select_parts):
        return None, (list(self.wrist_fids) if list(select_parts) == ['wrists'] else list(self.part_fids))


def _normal(net):
    def normal(x, eps=1e-3):                        # central differences of the density, as the reference's default normal
        cols = []
        for k in range(3):
            dx = torch.zeros(1, 3, device=x.device)
            dx[0, k] = eps
            sp, _ = net.common_forward((x + dx).clamp(-net.bound, net.bound))
            sn, _ = net.common_forward((x - dx).clamp(-net.bound, net.bound))
            cols.append(sp - sn)
        n = -0.5 * torch.stack(cols, dim=-1) / eps
        return torch.nan_to_num(n / n.norm(dim=-1, keepdim=True).clamp_min(1e-20))
    return normal


def _trainer(loss_type, num_points=3000, albedo=0.0, normal=0.0, whole=False, seed=0):
    from dreamwaltz_g_amd.nerf import bind_nerf_network
    m = _mesh()
    V, F = m['V'], m['F']
    pf, wf = (np.arange(len(F)), m['wf']) if whole else (m['pf'], m['wf'])
    net = nc.make_network(seed=seed).cuda()
    assert bind_nerf_network(net) is None
    net.normal = _normal(net)
    cfg = types.SimpleNamespace(sigma_loss_type=loss_type, sigma_noise_range=0.05, sigma_num_points=num_points, sigma_surface_thickness=0.005,
                                sigma_guidance_peak=15.0, sigma_guidance_delta=0.2, lambda_sigma_sigma=1.0, lambda_sigma_albedo=albedo,
                                lambda_sigma_normal=normal)
    tr = types.SimpleNamespace(cfg=cfg, smpl_model=_SMPLStub(F, pf, wf), model=net, losses={'mse': torch.nn.MSELoss(reduction='mean')},
                               time_to_snapshot=False)
    data = {'smpl_outputs': types.SimpleNamespace(vertices=torch.from_numpy(V)[None].cuda())}
    return tr, data


def _params(net):
    ps = {'embeddings': net.encoder.embeddings}
    for l, lin in enumerate(net.sigma_net.net):
        ps['w%d' % l], ps['b%d' % l] = lin.weight, lin.bias
    return ps


def _run(tr, data, seed, parts=('hands',), **kw):
    sg = _sg()
    for p in tr.model.parameters():
        p.grad = None
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = {}
    losses = sg.calc_sigma_loss(tr, data, {}, torch.zeros(1, device="cuda"), list(parts), generator=g, out=out, **kw)
    sum(losses.values()).backward()
    grads = {k: p.grad.detach().clone() for k, p in _params(tr.model).items()}
    return losses, out, grads


def _reference_losses(cfg, s, a, normals, pn, n, keep):
    """The reference's formulas in float64 on the COMPACTED points (positives, then the kept negatives)."""
    import torch.nn.functional as F
    sel = torch.cat([torch.arange(n, device=s.device), n + torch.nonzero(keep).flatten()])
    s, a = s[sel], (a[sel] if a is not None else None)
    k = int(keep.sum())
    losses = {}
    lt = cfg.sigma_loss_type
    if lt.startswith('opacity'):
        op = 1.0 - torch.exp(-cfg.sigma_guidance_delta * s)
        gt = torch.cat([torch.ones(n), torch.zeros(k)]).to(op)
        if lt == 'opacity_ce':
            q = gt
            loss = (-(op * torch.log(q.clamp(0.01, 0.99)) + (1 - op) * torch.log((1 - q).clamp(0.01, 0.99)))).sum()
        else:
            loss = ((op - gt) ** 2).mean()
    else:
        peak = cfg.sigma_guidance_peak
        if lt == 'mse':
            gt = peak * (torch.cat([torch.ones(n), torch.zeros(k)]).to(s) - 0.5) * 2
            loss = ((s - gt) ** 2).mean()
        else:
            loss = (F.relu(s[n:] + peak) ** 2).mean() + (F.relu(peak - s[:n]) ** 2).mean()
    losses['sigma_loss'] = loss * cfg.lambda_sigma_sigma
    if cfg.lambda_sigma_albedo > 0:
        losses['albedo_loss'] = a[:n].var(dim=0).sum() * cfg.lambda_sigma_albedo
    if cfg.lambda_sigma_normal > 0:
        losses['normal_loss'] = (1.0 - (normals * pn).sum(-1).abs()).mean() * cfg.lambda_sigma_normal
    return losses


WHOLE_CASES = [('margin', 0.0, 0.0), ('mse', 0.0, 0.0), ('opacity_mse', 0.0, 0.0), ('opacity_ce', 0.0, 0.0), ('margin', 0.5, 0.3)]


@pytest.mark.parametrize("loss_type,albedo,normal", WHOLE_CASES)
def test_calc_sigma_loss_matches_float64_composition(loss_type, albedo, normal):
    """The losses and the gradient of every field parameter against the reference's formulas in float64 on the compacted points, fed
    the field's own f32 outputs at the same points: what is checked is the masked, sync-free composition (the field itself is B7's,
    tested against float64 in test_nerf_field_gpu.py).  The composition's gradient goes back through the same field backward."""
    tr, data = _trainer(loss_type, albedo=albedo, normal=normal)
    losses, out, grads = _run(tr, data, seed=5)
    n = out['points'].shape[0]
    net, cfg = tr.model, tr.cfg
    keep = out['keep'] > 0
    assert 0 < int(keep.sum()) < n
    xyzs = out['xyzs']
    for p in net.parameters():
        p.grad = None
    if loss_type.startswith('opacity'):
        s32, a32 = net.common_forward(xyzs)
    else:
        s32, a32 = net.local_geometry_forward(xyzs)
    nrm32 = net.normal(xyzs[:n]) if normal > 0 else None
    s64 = s32.detach().double().requires_grad_(True)
    a64 = a32.detach().double().requires_grad_(True)
    n64 = nrm32.detach().double().requires_grad_(True) if nrm32 is not None else None
    ref = _reference_losses(cfg, s64, a64, n64, out['point_normals'].double(), n, keep)
    assert sorted(ref) == sorted(losses)
    for k in ref:
        e = abs(float(losses[k]) - float(ref[k])) / max(abs(float(ref[k])), 1e-30)
        assert e <= 1e-5, (k, float(losses[k]), float(ref[k]), e)
    leaves = [t for t in (s64, a64, n64) if t is not None]
    gs = torch.autograd.grad(sum(ref.values()), leaves, allow_unused=True)
    outs = [t for t in (s32, a32, nrm32) if t is not None]
    torch.autograd.backward([o for o, g in zip(outs, gs) if g is not None], [g.float() for g in gs if g is not None])
    for name, p in _params(net).items():
        e = nc.rel_err(grads[name], p.grad)
        assert e <= 1e-5, (name, e)
    dropped = ~keep
    assert int(dropped.sum()) > 0


def test_calc_sigma_loss_f32_matches_the_float64_field():
    """margin end to end in float64 (tests/nerf_field_cases.restate for the field): B7's f32 bars (5e-5 forward, 1e-4 gradients)."""
    tr, data = _trainer('margin', num_points=2000)
    losses, out, grads = _run(tr, data, seed=9)
    n = out['points'].shape[0]
    keep = out['keep'] > 0
    s, _, leaves = nc.restate(tr.model, out['xyzs'].cpu().numpy(), raw=True)
    ref = _reference_losses(tr.cfg, s, None, None, None, n, keep.cpu())
    loss64 = ref['sigma_loss']
    assert abs(float(losses['sigma_loss']) - float(loss64)) <= 5e-5 * abs(float(loss64))
    loss64.backward()
    for name in grads:
        e = nc.rel_l2(grads[name], leaves[name].grad)
        assert e <= 1e-4, (name, e)


def test_calc_sigma_loss_f16_within_twice_the_composition_error():
    """Under fp16 autocast (B7's f16 mode): the loss against float64 with the f16 rounding points, within twice the error of the
    unbound torch composition of the same network."""
    tr, data = _trainer('margin', num_points=2000)
    with torch.autocast("cuda", dtype=torch.float16):
        losses, out, grads = _run(tr, data, seed=13)
    n = out['points'].shape[0]
    keep = out['keep'] > 0
    s, _, leaves = nc.restate(tr.model, out['xyzs'].cpu().numpy(), raw=True, f16=True)
    loss64 = _reference_losses(tr.cfg, s, None, None, None, n, keep.cpu())['sigma_loss']
    loss64.backward()
    from dreamwaltz_g_amd.nerf import unbind_nerf_network
    unbind_nerf_network(tr.model)
    for p in tr.model.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.float16):
        sc_, _ = tr.model.local_geometry_forward(out['xyzs'])
    comp = _reference_losses(tr.cfg, sc_.float(), None, None, None, n, keep)['sigma_loss']
    comp.backward()
    e_k = abs(float(losses['sigma_loss']) - float(loss64))
    e_c = abs(float(comp) - float(loss64))
    assert e_k <= 2 * e_c + 1e-6 * abs(float(loss64)), (e_k, e_c)
    comp_grads = {k: p.grad for k, p in _params(tr.model).items()}
    # the last bias's sigma entry is a sum of dsigma over all points, where the margin's positive and negative terms nearly cancel
    # (30 / N each, opposite signs): its relative error is that of a few fp16 roundings amplified by the cancellation, so it is judged
    # in the whole gradient vector rather than on its own
    last_b = 'b%d' % (len(tr.model.sigma_net.net) - 1)
    for name in grads:
        if name == last_b:
            continue
        ek, ec = nc.rel_l2(grads[name], leaves[name].grad), nc.rel_l2(comp_grads[name], leaves[name].grad)
        assert ek <= 2 * ec + 1e-6, (name, ek, ec)
    cat = lambda d: torch.cat([d[k].detach().double().cpu().reshape(-1) for k in sorted(grads)])     # noqa: E731
    ek, ec = nc.rel_l2(cat(grads), cat({k: leaves[k].grad for k in grads})), nc.rel_l2(cat(comp_grads), cat({k: leaves[k].grad for k in grads}))
    assert ek <= 2 * ec + 1e-6, ("all", ek, ec)


def test_calc_sigma_loss_whole_mesh_part_with_negative_num_points():
    tr, data = _trainer('margin', num_points=-1, whole=True)
    losses, out, grads = _run(tr, data, seed=17)
    assert out['points'].shape == (20480, 3) and out['xyzs'].shape == (40960, 3)
    assert torch.isfinite(losses['sigma_loss']) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert 0 < int(out['kept']) <= 20480


def test_calc_sigma_loss_makes_no_host_sync():
    tr, data = _trainer('margin')
    _run(tr, data, seed=21)                                          # builds and caches the part topology (host -> device once)
    sg = _sg()
    g = torch.Generator(device="cuda").manual_seed(21)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = sg.calc_sigma_loss(tr, data, {}, torch.zeros(1, device="cuda"), ['hands'], generator=g)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(losses['sigma_loss'])


def test_calc_sigma_loss_is_deterministic():
    tr, data = _trainer('opacity_ce', albedo=0.5)
    l1, o1, g1 = _run(tr, data, seed=33)
    l2, o2, g2 = _run(tr, data, seed=33)
    for k in ('points', 'noisy', 'keep', 'closest_face', 'sqr_dist', 'kept'):
        assert torch.equal(o1[k], o2[k]), k
    for k in l1:
        assert torch.equal(l1[k], l2[k]), k
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
