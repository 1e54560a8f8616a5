"""Shared inputs and float64 numpy oracles of the avatar-construction tests (boundary B11, include/dwg_avatar_init.h).

The oracles are written from the statements' meaning: Ericson's closest point on a triangle (Real-Time Collision Detection 5.1.5) by
Voronoi region, brute-force K nearest neighbours ordered by (squared distance, index), barycentric interpolation of a vertex table, and
the neighbour smoothing w' = (1 - u) w + u sum_k a_k w[idx_k] with a = row-normalised 1 / (mesh distance of the neighbour x distance to
it) and u the clamped ramp of the point's own mesh distance.
"""
import functools

import numpy as np


# ------------------------------------------------------------------------------------------------------------------------------------
# meshes and point sets
# ------------------------------------------------------------------------------------------------------------------------------------
def make_sphere(rings=12, segments=24, radius=0.5):
    """Latitude-longitude sphere without pole caps: rings x segments vertices, 2 (rings - 1) segments faces (12 x 24 -> 288, 528), wound
    so that the face normals (v1 - v0) x (v2 - v0) point outwards.  fp32 vertices, int64 faces."""
    th = np.pi * (np.arange(rings) + 1.0) / (rings + 1.0)
    ph = 2.0 * np.pi * np.arange(segments) / segments
    V = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones(segments))], -1)
    V = (radius * V).reshape(-1, 3).astype(np.float32)
    F = []
    for i in range(rings - 1):
        for j in range(segments):
            a, b = i * segments + j, i * segments + (j + 1) % segments
            c, d = a + segments, b + segments
            F += [(a, c, b), (b, c, d)]
    F = np.asarray(F, dtype=np.int64)
    n = face_normals(V, F)
    assert (np.einsum('fk,fk->f', n, V[F].mean(1).astype(np.float64)) > 0).all()
    return V, F


def face_normals(V, F):
    t = V.astype(np.float64)[F]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def interior_points(V, F, count=600, seed=0, offset=0.01):
    """Points over face interiors: foot = sum b_i v_i with min b >= 0.1 and pairwise differences >= 0.02, moved +-offset along the face
    normal.  Returns (points fp32, face, bary float64 of the fp32 points' feet before rounding)."""
    rng = np.random.default_rng(seed)
    face = rng.integers(0, len(F), count)
    bary = np.empty((count, 3))
    for i in range(count):
        while True:
            b = rng.dirichlet(np.ones(3))
            if b.min() >= 0.1 and min(abs(b[0] - b[1]), abs(b[1] - b[2]), abs(b[0] - b[2])) >= 0.02:
                break
        bary[i] = b
    foot = np.einsum('nk,nkc->nc', bary, V.astype(np.float64)[F[face]])
    sign = np.where(rng.random(count) < 0.5, -1.0, 1.0)
    pts = foot + (sign * offset)[:, None] * face_normals(V, F)[face]
    return pts.astype(np.float32), face, bary


def edge_and_corner_points(V, F, count=200, seed=1):
    """Points whose closest mesh point (the foot) is on an edge (half of them) or a vertex of a face away from the open rims, moved
    outwards by 0.01 .. 0.03 along the unit sum of the normals of the faces around that edge / vertex: a direction inside the feature's
    normal cone on this convex mesh, so the foot stays the closest point.  Returns (points fp32, feet float64)."""
    rng = np.random.default_rng(seed)
    N, Vd = face_normals(V, F), V.astype(np.float64)
    rim = set(np.nonzero(np.bincount(F.reshape(-1), minlength=len(V)) < 6)[0].tolist())       # an inner vertex has six faces
    inner = np.array([f for f in range(len(F)) if not rim & set(F[f].tolist())])
    pts, feet = [], []
    for i in range(count):
        f = F[rng.choice(inner)]
        if i % 2 == 0:
            e, t = rng.integers(0, 3), rng.uniform(0.1, 0.9)
            a, b = f[e], f[(e + 1) % 3]
            foot = t * Vd[a] + (1 - t) * Vd[b]
            around = ((F == a).any(1) & (F == b).any(1))
        else:
            a = f[rng.integers(0, 3)]
            foot = Vd[a]
            around = (F == a).any(1)
        n = N[around].sum(0)
        pts.append(foot + rng.uniform(0.01, 0.03) * n / np.linalg.norm(n)); feet.append(foot)
    return np.asarray(pts, np.float32), np.asarray(feet)


def shell_points(count, seed, radius=0.5, lo=0.002, hi=0.05, zmax=0.9):
    """Points on both sides of the sphere of `radius`, |r - radius| uniform in [lo, hi], away from the open poles (|z| / r <= zmax)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-zmax, zmax, count)
    ph = rng.uniform(0, 2 * np.pi, count)
    s = np.sqrt(1 - z * z)
    d = np.stack([s * np.cos(ph), s * np.sin(ph), z], -1)
    r = radius + rng.uniform(lo, hi, count) * np.where(rng.random(count) < 0.5, -1.0, 1.0)
    return (d * r[:, None]).astype(np.float32)


def lattice(n=9, spacing=1.0 / 64):
    """n^3 lattice points; with spacing 1 / 64 every coordinate difference and squared distance is exact in fp32."""
    g = np.arange(n, dtype=np.float32) * np.float32(spacing)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def uniform_cloud(count=4096, seed=0):
    """torch.rand(count, 3) with the CPU generator seeded `seed`, mapped to [-1, 1]^3 (fp32 numpy, read-only)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(count, 3, generator=g) * 2 - 1).numpy()
    a.setflags(write=False)
    return a


def sparse_table(rows, cols=55, seed=0, density=0.1):
    """Sparse non-negative fp32 table whose rows sum to 1 (every row has at least one entry)."""
    rng = np.random.default_rng(seed)
    t = rng.random((rows, cols)) * (rng.random((rows, cols)) < density)
    t[np.arange(rows), rng.integers(0, cols, rows)] += 0.5
    return (t / t.sum(1, keepdims=True)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# oracles (float64)
# ------------------------------------------------------------------------------------------------------------------------------------
def closest_on_triangles(P, A, B, C):
    """Ericson: closest point of triangle (A, B, C) to P, broadcast over leading axes.  Returns (closest point, bary [..., 3])."""
    ab, ac, ap = B - A, C - A, P - A
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = P - B
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = P - C
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide='ignore', invalid='ignore'):
        den = 1.0 / (va + vb + vc)
        v, w = vb * den, vc * den                                   # interior
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    vs = [zero, one, t_ab, zero, zero, 1 - t_bc]
    ws = [zero, zero, zero, one, t_ac, t_bc]
    v, w = np.select(conds, vs, v), np.select(conds, ws, w)
    bary = np.stack([1 - v - w, v, w], -1)
    return A + v[..., None] * ab + w[..., None] * ac, bary


def nearest_triangles(P, V, F, tie=0.0, chunk=256):
    """Brute force over all faces in float64 -> dict(d2 [N], face [N], closest [N, 3], bary [N, 3], runner_up_d2 [N]): the closest face
    (the lowest index among faces whose DISTANCE is within tie * (1 + d) of the minimum), its closest point and barycentrics, and the
    smallest squared distance among the other faces."""
    P, T = np.asarray(P, np.float64), np.asarray(V, np.float64)[np.asarray(F)]
    out = dict(d2=[], face=[], closest=[], bary=[], runner_up_d2=[])
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        q, b = closest_on_triangles(p, T[None, :, 0], T[None, :, 1], T[None, :, 2])
        d2 = ((q - p) ** 2).sum(-1)
        dmin = np.sqrt(d2.min(1))
        face = np.argmax(np.sqrt(d2) <= (dmin + tie * (1 + dmin))[:, None], axis=1)
        r = np.arange(len(face))
        rest = d2.copy()
        rest[r, face] = np.inf
        out['d2'].append(d2[r, face]); out['face'].append(face); out['closest'].append(q[r, face]); out['bary'].append(b[r, face])
        out['runner_up_d2'].append(rest.min(1))
    return {k: (np.concatenate(v) if v else np.zeros((0,) + ((3,) if k in ('closest', 'bary') else ()))) for k, v in out.items()}


def faces_within(P, V, F, tol, chunk=256):
    """[N, F] bool: the faces whose distance to the point is within tol * (1 + d) of the minimum d (float64)."""
    P, T = np.asarray(P, np.float64), np.asarray(V, np.float64)[np.asarray(F)]
    out = []
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        q, _ = closest_on_triangles(p, T[None, :, 0], T[None, :, 1], T[None, :, 2])
        d = np.sqrt(((q - p) ** 2).sum(-1))
        dmin = d.min(1, keepdims=True)
        out.append(d <= dmin + tol * (1 + dmin))
    return np.concatenate(out) if out else np.zeros((0, len(T)), bool)


def knn(Q, R, K, chunk=512):
    """(idx [Nq, K] int64, d2 [Nq, K] float64) of the K nearest rows of R to each row of Q by (squared distance, index); d2 is the sum
    of the squared coordinate differences of the fp32 inputs in float64."""
    Q, R = np.asarray(Q, np.float64), np.asarray(R, np.float64)
    idx, d2 = [], []
    for s in range(0, len(Q), chunk):
        d = ((Q[s:s + chunk, None, :] - R[None]) ** 2).sum(-1)
        o = np.argsort(d, axis=1, kind='stable')[:, :K]              # stable: equal distances stay in index order
        idx.append(o); d2.append(np.take_along_axis(d, o, 1))
    return np.concatenate(idx), np.concatenate(d2)


def interp(table, vertex_indices, bary):
    return np.einsum('nij,ni->nj', np.asarray(table, np.float64)[vertex_indices], np.asarray(bary, np.float64))


def smoothing_weights(idx, d2, mesh_d2, use_sqrt=True, low=0.01, high=None):
    high = low if high is None else high
    kd, md = np.asarray(d2, np.float64), np.asarray(mesh_d2, np.float64)
    if use_sqrt:
        kd, md = np.sqrt(kd), np.sqrt(md)
    a = 1.0 / (md[idx] * kd)
    a = a / a.sum(-1, keepdims=True)
    u = md.copy()
    u[md <= low] = 0.0
    u[md >= high] = 1.0
    mid = (md > low) & (md < high)
    u[mid] = (md[mid] - low) / (high - low) if high > low else u[mid]
    return a, u


def smooth(w, idx, a, u, n):
    w = np.asarray(w, np.float64).copy()
    for _ in range(n):
        w = (1.0 - u)[:, None] * w + u[:, None] * np.einsum('nk,nkj->nj', a, w[idx])
    return w
