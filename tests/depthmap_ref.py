"""float64 side of the depth-map tests (tests/test_depth_condition_{gpu,host}.py; include/dwg_depthmap.h) -- TEST INFRASTRUCTURE ONLY.

  pixel_rays()      one pinhole ray per pixel, exactly as the header states them: direction ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)
                    rotated by R^T, in float64, rounded to float32; origin -R^T T.  Written product by product (numpy's element-wise
                    float64 statements have no fused multiply-add), so the float32 rays are the bits the kernel casts
  reference()       oracle.condition.ray_cast on those rays (the repository's stand-in for open3d's cast_rays: imported, not edited) ->
                    t_hit; for the rays that hit, the hit triangle (lowest index at the minimum), its normal, and the runner-up distance
  sensitivity()     the largest relative change of the oracle's own depth when every float32 ray component moves by one ulp, all eight
                    sign patterns -- what the two sides may legitimately differ by
  depth_image()     export_depth's statements (smpl_condition.py:242-248) on a float32 array, as numpy does them
  loss()            Trainer.pretrain_forward's two MSE terms (trainer.py:1250,1264-1277) in torch float64, with their gradients
"""
import functools
import itertools
import os

import numpy as np
import torch

from oracle import condition as oc

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_golden_r2_condition.npz"))


def ellipsoid(nu, nv, radii=(0.25, 0.8, 0.15)):
    """The closed test mesh of tests/test_condition_gpu.py (_ellipsoid)."""
    us = np.linspace(0, 2 * np.pi, nu, endpoint=False); vs = np.linspace(0, np.pi, nv + 1)
    vv, uu = np.meshgrid(vs, us, indexing="ij")
    verts = np.stack([radii[0] * np.sin(vv) * np.cos(uu), radii[1] * np.cos(vv), radii[2] * np.sin(vv) * np.sin(uu)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    a = (i * nu + j).reshape(-1); b = (i * nu + (j + 1) % nu).reshape(-1)
    tris = np.concatenate([np.stack([a, a + nu, b], 1), np.stack([b, a + nu, b + nu], 1)])
    return verts.astype(np.float32), tris.astype(np.int32)


def golden_mesh():
    return np.asarray(G["cond.vertices"], dtype=np.float32), G["cond.triangles"].astype(np.int32)


def camera(name, width, height, zero_translation=False):
    """The golden camera `name` with its intrinsics adjusted to width x height: (extrinsic [4,4], intrinsics [3,3]) float32."""
    E = np.asarray(G["cond.%s.extrinsic" % name], dtype=np.float32).copy()
    if zero_translation:
        E[:3, 3] = 0
    K = oc.adjust_intrinsics_size(np.asarray(G["cond.%s.intrinsics_raw" % name], dtype=np.float32), width, height).astype(np.float32)
    return E, K


def pixel_rays(extrinsic, intrinsics, x, y):
    """Rays through the pixel indices (x, y) (arrays; pixel centres are at index + 0.5) -> origin [3] float64, directions [N, 3] float32."""
    E = np.asarray(extrinsic, dtype=np.float32).astype(np.float64)
    K = np.asarray(intrinsics, dtype=np.float32).astype(np.float64)
    R, T = E[:3, :3], E[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    dx = ((np.asarray(x, dtype=np.float64) + 0.5 - cx) / fx).reshape(-1)
    dy = ((np.asarray(y, dtype=np.float64) + 0.5 - cy) / fy).reshape(-1)
    d = np.stack([(R[0, i] * dx + R[1, i] * dy) + R[2, i] for i in range(3)], 1)
    o = np.array([-((R[0, i] * T[0] + R[1, i] * T[1]) + R[2, i] * T[2]) for i in range(3)])
    return o, d.astype(np.float32)


def rays(extrinsic, intrinsics, width, height):
    """One ray per pixel of a width x height image, row-major."""
    y, x = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    return pixel_rays(extrinsic, intrinsics, x, y)


def _per_triangle(o, d, v0, e1, e2):
    """oracle.condition.ray_cast's statements for ONE ray, kept per triangle: t [F] (inf where the triangle is not hit)."""
    tv = o[None, :] - v0
    p = np.cross(d[None, :], e2)
    det = (e1 * p).sum(1)
    ok = np.abs(det) > 1e-12
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    u = (tv * p).sum(1) * inv
    q = np.cross(tv, e1)
    w = (q * d[None, :]).sum(1) * inv
    t = (q * e2).sum(1) * inv
    hit = ok & (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
    return np.where(hit, t, np.inf)


def reference(extrinsic, intrinsics, width, height, vertices, triangles):
    """-> dict: t [H,W] float64 (inf = miss), tri [H,W] (-1 = miss), second [H,W] (runner-up distance, inf if none),
    normal [H,W,3] float64 (zero = miss), origin, dirs."""
    o, d = rays(extrinsic, intrinsics, width, height)
    t = oc.ray_cast(o, d, vertices, triangles)
    v = np.asarray(vertices, dtype=np.float64)
    tri = np.asarray(triangles)
    v0, e1, e2 = v[tri[:, 0]], v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]]
    idx = np.full(t.shape, -1, dtype=np.int64)
    second = np.full(t.shape, np.inf)
    normal = np.zeros((t.shape[0], 3))
    d64 = d.astype(np.float64)
    for i in np.nonzero(np.isfinite(t))[0]:
        tt = _per_triangle(o, d64[i], v0, e1, e2)
        k = int(np.argmin(tt))                                  # first index at the minimum: the lower triangle index wins a tie
        assert tt[k] == t[i], "the helper's statements are not the oracle's"
        idx[i] = k
        tt[k] = np.inf
        second[i] = tt.min()
        n = np.cross(e1[k], e2[k])
        normal[i] = n / np.linalg.norm(n)
    sh = (height, width)
    return dict(t=t.reshape(sh), tri=idx.reshape(sh), second=second.reshape(sh), normal=normal.reshape(sh + (3,)), origin=o, dirs=d)


def sensitivity(ref, vertices, triangles):
    """(s, flips): the largest relative change of the oracle's depth over the hit rays when every float32 ray component moves by one
    ulp (all eight sign patterns), and how many of those rays stopped hitting."""
    t = ref["t"].reshape(-1)
    hit = np.isfinite(t)
    d = ref["dirs"][hit]
    s, flips = 0.0, 0
    for signs in itertools.product((-1.0, 1.0), repeat=3):
        target = np.where(np.array(signs, dtype=np.float32) > 0, np.float32(np.inf), np.float32(-np.inf))
        dp = np.nextafter(d, np.broadcast_to(target, d.shape))
        tp = oc.ray_cast(ref["origin"], dp, vertices, triangles)
        ok = np.isfinite(tp)
        flips += int((~ok).sum())
        s = max(s, float((np.abs(tp[ok] - t[hit][ok]) / t[hit][ok]).max()))
    return s, flips


def depth_image(t_hit):
    """export_depth(inverse=True, normalize=True) on a float32 [H,W] array -> uint8 [H,W,3]; an all-zero image where the maximum is 0
    after the subtraction (the reference divides 0 by 0 there)."""
    depth = np.asarray(t_hit, dtype=np.float32).copy()
    with np.errstate(divide="ignore"):
        depth = 1.0 / depth
    assert depth.dtype == np.float32
    depth -= np.min(depth)
    if not np.max(depth) > 0:
        return np.zeros(depth.shape + (3,), dtype=np.uint8)
    depth /= np.max(depth)
    image = np.asarray(depth * 255.0, np.uint8)
    return np.stack([image, image, image], axis=2)


def loss(render_depth, render_ws, smpl_depth, grad=1.0, dtype=torch.float64):
    """-> (loss, grad_depth, grad_ws) of the reference's statements evaluated in `dtype` on the CPU."""
    rd = render_depth.detach().cpu().to(dtype).requires_grad_(True)
    rw = render_ws.detach().cpu().to(dtype).requires_grad_(True)
    sd = torch.nan_to_num(smpl_depth.detach().cpu().to(dtype), nan=0.0, posinf=0.0, neginf=0.0).reshape(rd.shape)
    mask = (sd > 1e-6).to(dtype)
    out = torch.nn.functional.mse_loss(rw, mask) + torch.nn.functional.mse_loss(rd, sd)
    out.backward(torch.tensor(grad, dtype=dtype))
    return out.detach(), rd.grad, rw.grad


@functools.lru_cache(maxsize=None)
def case(name):
    """The five cases of the depth tests, each computed once: dict(E, K, W, H, v, t, ref, s)."""
    if name in ("front", "side", "wide"):
        W, H = (44, 25) if name == "wide" else (64, 64)
        v, t = golden_mesh()
        E, K = camera(name, W, H)
    elif name == "inside":                                       # the camera sits inside the closed mesh: every ray hits
        W, H = 32, 32
        v, t = ellipsoid(24, 12)
        E, K = camera("side", W, H, zero_translation=True)
    elif name == "body":                                         # a mesh of the body's size (SMPL-X: 10 475 vertices, 20 908 triangles)
        W, H = 48, 48
        v, t = ellipsoid(146, 72)
        E, K = camera("front", W, H)
    else:
        raise KeyError(name)
    ref = reference(E, K, W, H, v, t)
    s = case("front")["s"] if name == "body" else sensitivity(ref, v, t)[0]
    return dict(E=E, K=K, W=W, H=H, v=v, t=t, ref=ref, s=s)


CASES = ["front", "side", "wide", "inside", "body"]
