"""Float64 restatement of the NeRF stage's sigma guidance geometry (boundary B8) for the tests of dreamwaltz_g_amd.sigma_guidance.

The reference computes this part with trimesh and libigl (core/trainer.py:718-825), which are not installed here; what follows restates
their published algorithms, so nothing is pinned against the packages themselves:
  face_areas / area_cdf       trimesh's area_faces (|e0 x e1| / 2) and the cumulative sum sample_surface searches
  vertex_normals              trimesh's weighted_vertex_normals over the given faces only: sum of corner angle * unit face normal, unitized
                              (a face whose cross product is below 1e-12 has a zero normal; a zero sum stays zero)
  sample                      trimesh's sample_surface on given draws [N, 4] (face pick, r1, r2, noise) + the interpolated point normal
                              unitize(sum lambda_k n_k) + the noisy point p + (u3 - 0.5) * range * n
  closest_point               libigl's point_mesh_squared_distance: Ericson's region test (Real-Time Collision Detection 5.1.5);
                              a collinear face (|e0 x e1|^2 <= 1e-14 |e0|^2 |e1|^2) counts as its three segments
  closest_point_enumerated    an independent check: the interior projection (when inside) and every edge and vertex, the nearest wins
  distance                    brute force over all faces, chunked; the lowest face index among exact minima
Everything is torch float64 on the device of its inputs.  Synthetic meshes: make_icosphere(level) (level 5: 10 242 vertices, 20 480
faces, about SMPL-X size), make_part (a cap with a ring of "wrist" faces), add_degenerate (collinear and repeated-vertex faces).
"""
import numpy as np
import torch


# --------------------------------------------------------------------------------------------------------------------------------------
# meshes
# --------------------------------------------------------------------------------------------------------------------------------------
def make_icosphere(level):
    """(V [Nv, 3] fp32 numpy on the unit sphere, F [Nf, 3] int64): the icosahedron subdivided `level` times."""
    t = (1.0 + 5 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = f
    for _ in range(level):
        mid = {}

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        nf = []
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        faces = nf
    return np.array(verts, np.float32), np.array(faces, np.int64)


def make_part(V, F, zmin=0.2, wrist_band=0.08):
    """(part_fids, wrist_fids): the faces whose centroid has z > zmin, and those of them within wrist_band of the cap's rim."""
    cz = V[F].mean(axis=1)[:, 2]
    part = np.nonzero(cz > zmin)[0]
    wrist = part[cz[part] < zmin + wrist_band]
    return part, wrist


def add_degenerate(V, F):
    """V, F with degenerate faces appended: an exactly collinear face (its vertices differ in z only), two faces with a repeated vertex
    (segments) and one whose three corners coincide (a point)."""
    V = np.asarray(V, np.float32)
    a, b, c = F[0]
    nv = len(V)
    extra_v = np.stack([V[a] + np.float32([0, 0, 0.1]), V[a] + np.float32([0, 0, 0.2]), V[c] + np.float32([0.3, 0, 0])]).astype(np.float32)
    extra_f = np.array([[a, nv, nv + 1], [a, a, b], [c, nv + 2, nv + 2], [b, b, b]], np.int64)
    return np.concatenate([V, extra_v]), np.concatenate([F, extra_f])


# --------------------------------------------------------------------------------------------------------------------------------------
# part mesh
# --------------------------------------------------------------------------------------------------------------------------------------
def _t(x, device=None):
    return torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x, device=device).double()


def _unitize(x, thr=1e-12):
    n = x.norm(dim=-1, keepdim=True)
    return torch.where(n > thr, x / torch.where(n > thr, n, torch.ones_like(n)), torch.zeros_like(x))


def face_areas(V, F):
    V = _t(V)
    F = torch.as_tensor(F, device=V.device).long()
    tri = V[F]
    return 0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=-1)


def area_cdf(V, F):
    return torch.cumsum(face_areas(V, F), 0)


def vertex_normals(V, F):
    """[Nv, 3] float64: trimesh's weighted_vertex_normals over the faces F only."""
    V = _t(V)
    F = torch.as_tensor(F, device=V.device).long()
    tri = V[F]
    fn = _unitize(torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
    out = torch.zeros_like(V)
    for c in range(3):
        u = _unitize(tri[:, (c + 1) % 3] - tri[:, c])
        w = _unitize(tri[:, (c + 2) % 3] - tri[:, c])
        ang = torch.arccos((u * w).sum(-1).clamp(-1, 1))
        out.index_add_(0, F[:, c], fn * ang[:, None])
    return _unitize(out)


def sample(V, F, draws, noise_range=0.0):
    """trimesh's sample_surface on the draws [N, 4] float64: (points, face_index, point_normals, noisy), float64."""
    V = _t(V)
    F = torch.as_tensor(F, device=V.device).long()
    d = _t(draws, V.device)
    cdf = area_cdf(V, F)
    fid = torch.searchsorted(cdf, d[:, 0] * cdf[-1], side='left').clamp_max(len(F) - 1)
    r1, r2 = d[:, 1].clone(), d[:, 2].clone()
    fold = (r1 + r2) > 1.0
    r1 = torch.where(fold, (r1 - 1).abs(), r1)
    r2 = torch.where(fold, (r2 - 1).abs(), r2)
    tri = V[F[fid]]
    pts = (r1[:, None] * (tri[:, 1] - tri[:, 0]) + r2[:, None] * (tri[:, 2] - tri[:, 0])) + tri[:, 0]
    vn = vertex_normals(V, F)[F[fid]]
    lam = torch.stack([1 - r1 - r2, r1, r2], dim=1)
    pn = _unitize((vn * lam[:, :, None]).sum(1))
    noisy = pts + ((d[:, 3] - 0.5) * noise_range)[:, None] * pn
    return pts, fid, pn, noisy


# --------------------------------------------------------------------------------------------------------------------------------------
# closest points
# --------------------------------------------------------------------------------------------------------------------------------------
def _degenerate(e0, e1):
    nn = torch.linalg.cross(e0, e1).pow(2).sum(-1)
    return nn <= 1e-14 * e0.pow(2).sum(-1) * e1.pow(2).sum(-1)


def _seg(ap, d):
    """closest parameter in [0, 1] on the segment t d to ap (broadcast), and the squared distance."""
    dd = (d * d).sum(-1)
    t = torch.where(dd > 0, (ap * d).sum(-1) / torch.where(dd > 0, dd, torch.ones_like(dd)), torch.zeros_like(dd)).clamp(0, 1)
    r = ap - t[..., None] * d
    return t, (r * r).sum(-1)


def _edges_vw(ap, e0, e1):
    """(v, w) of the nearest point of the three edges (AB, AC, BC)."""
    tab, dab = _seg(ap, e0)
    tac, dac = _seg(ap, e1)
    tbc, dbc = _seg(ap - e0, e1 - e0)
    v, w, best = tab, torch.zeros_like(tab), dab
    c = dac < best
    v, w, best = torch.where(c, torch.zeros_like(v), v), torch.where(c, tac, w), torch.where(c, dac, best)
    c = dbc < best
    v, w = torch.where(c, 1 - tbc, v), torch.where(c, tbc, w)
    return v, w


def closest_vw(ap, e0, e1):
    """Ericson's region test in float64: (v, w) with the closest point v0 + v e0 + w e1 (all arguments broadcast, [..., 3])."""
    ap, e0, e1 = torch.broadcast_tensors(ap, e0, e1)
    d1, d2 = (e0 * ap).sum(-1), (e1 * ap).sum(-1)
    aa, bb, ab = (e0 * e0).sum(-1), (e1 * e1).sum(-1), (e0 * e1).sum(-1)
    d3, d4, d5, d6 = d1 - aa, d2 - ab, d1 - ab, d2 - bb
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    z, o = torch.zeros_like(d1), torch.ones_like(d1)
    safe = lambda n, d: n / torch.where(d != 0, d, o)           # noqa: E731
    den = va + vb + vc
    v, w = safe(vb, den), safe(vc, den)                                                  # interior
    ev, ew = _edges_vw(ap, e0, e1)
    inside = (va >= 0) & (vb >= 0) & (vc >= 0) & (den > 0)
    v, w = torch.where(inside, v, ev), torch.where(inside, w, ew)
    # the regions in reverse priority, so that the first test of Ericson's sequence wins
    t = safe(d4 - d3, (d4 - d3) + (d5 - d6))
    c = (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)
    v, w = torch.where(c, 1 - t, v), torch.where(c, t, w)
    c = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    v, w = torch.where(c, z, v), torch.where(c, safe(d2, d2 - d6), w)
    c = (d6 >= 0) & (d5 <= d6)
    v, w = torch.where(c, z, v), torch.where(c, o, w)
    c = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    v, w = torch.where(c, safe(d1, d1 - d3), v), torch.where(c, z, w)
    c = (d3 >= 0) & (d4 <= d3)
    v, w = torch.where(c, o, v), torch.where(c, z, w)
    c = (d1 <= 0) & (d2 <= 0)
    v, w = torch.where(c, z, v), torch.where(c, z, w)
    deg = _degenerate(e0, e1)
    return torch.where(deg, ev, v), torch.where(deg, ew, w)


def closest_vw_enumerated(ap, e0, e1):
    """Independent enumeration: the interior projection (when it falls inside a non-degenerate face), every edge and every vertex."""
    ap, e0, e1 = torch.broadcast_tensors(ap, e0, e1)
    aa, bb, ab = (e0 * e0).sum(-1), (e1 * e1).sum(-1), (e0 * e1).sum(-1)
    r0, r1 = (e0 * ap).sum(-1), (e1 * ap).sum(-1)
    det = aa * bb - ab * ab
    ok = ~_degenerate(e0, e1)
    detn = torch.where(ok, det, torch.ones_like(det))
    v, w = (bb * r0 - ab * r1) / detn, (aa * r1 - ab * r0) / detn
    cands = []
    cands.append((v, w, ok & (v >= 0) & (w >= 0) & (v + w <= 1)))
    for o_, d_, base in ((0, e0, (0, 0)), (1, e1, (0, 0)), (2, e1 - e0, (1, 0))):
        t, _ = _seg(ap - (e0 if o_ == 2 else 0), d_)
        if o_ == 0:
            cands.append((t, torch.zeros_like(t), torch.ones_like(ok)))
        elif o_ == 1:
            cands.append((torch.zeros_like(t), t, torch.ones_like(ok)))
        else:
            cands.append((1 - t, t, torch.ones_like(ok)))
    for vv, ww in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
        cands.append((torch.full_like(v, vv), torch.full_like(v, ww), torch.ones_like(ok)))
    best, bv, bw = None, None, None
    for cv, cw, valid in cands:
        r = ap - cv[..., None] * e0 - cw[..., None] * e1
        d = torch.where(valid, (r * r).sum(-1), torch.full_like(v, float('inf')))
        if best is None:
            best, bv, bw = d, cv, cw
        else:
            c = d < best
            best, bv, bw = torch.where(c, d, best), torch.where(c, cv, bv), torch.where(c, cw, bw)
    return bv, bw


def face_frames(V, F):
    V = _t(V)
    F = torch.as_tensor(F, device=V.device).long()
    tri = V[F]
    return tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]


def point_face_d2(P, V, F, fids=None, enumerated=False):
    """Squared distances and closest points of P [N, 3] to the faces fids [N] (one face per point), float64."""
    P = _t(P)
    v0, e0, e1 = face_frames(V, F)
    fids = torch.as_tensor(fids, device=P.device).long()
    ap = P - v0[fids]
    v, w = (closest_vw_enumerated if enumerated else closest_vw)(ap, e0[fids], e1[fids])
    q = v0[fids] + v[:, None] * e0[fids] + w[:, None] * e1[fids]
    return ((P - q) ** 2).sum(-1), q


def all_face_distances(P, V, F, chunk=32):
    """[N, Nf] float64 distances (not squared) of every point to every face, in chunks of points."""
    P = _t(P)
    v0, e0, e1 = face_frames(V, F)
    out = []
    for s in range(0, len(P), chunk):
        ap = P[s:s + chunk, None, :] - v0[None]
        v, w = closest_vw(ap, e0[None], e1[None])
        r = ap - v[..., None] * e0[None] - w[..., None] * e1[None]
        out.append((r * r).sum(-1).sqrt())
    return torch.cat(out) if out else torch.zeros((0, len(v0)), dtype=torch.float64, device=P.device)


def distance(P, V, F, chunk=32):
    """libigl's point_mesh_squared_distance in float64: (sqrD, I, C); ties: the lowest face index."""
    D = all_face_distances(P, V, F, chunk)
    I = torch.argmin(D, dim=1)
    d2, C = point_face_d2(P, V, F, I)
    return d2, I, C


def keep_mask(d2, closest, thickness, wrist_flags=None):
    keep = d2.sqrt() > thickness
    if wrist_flags is not None:
        keep = keep & ~torch.as_tensor(wrist_flags, device=d2.device).bool()[closest]
    return keep


def stratified_draws(n, seed=0):
    """[n, 4] float64 draws in [0, 1) from numpy (the tests feed the same draws to the kernels and to the restatement)."""
    return np.random.RandomState(seed).rand(n, 4)
