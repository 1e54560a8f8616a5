"""Helpers of the scene-cull tests (boundary B25): a numpy restatement, in float64 and in float32, of the decision by which the rasterizer's
k_preprocess gives a Gaussian a radius > 0 (csrc/raster.hip: the near plane, cov3d_of, ewa_project, the larger eigenvalue, the tile
rectangle), the generators of the cases the cull's bound is checked over, and the g++ build of csrc/cull_math.h."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT = 16
CAMERA_FLOATS = 37
IMAGES = ((64, 64), (35, 67))                      # (H, W): a square image and one whose edges are no multiple of a tile


# ---- the rasterizer's keep decision, restated ---------------------------------------------------------------------------------------------
def preprocess_keeps(positions, scales, quats, block, H, W, dtype=np.float64):
    """bool [N]: k_preprocess gives radius > 0 (scale_modifier 1), every statement evaluated in `dtype`.  positions [N, 3], scales [N, 3]
    (activated), quats [N, 4] (as the rasterizer reads them: real first, not normalised again), block: one camera block of 37 floats."""
    f = dtype
    p, s, q = (np.asarray(a, dtype=np.float32).astype(f) for a in (positions, scales, quats))
    block = np.asarray(block, dtype=np.float32).astype(f)
    view, proj = block[:16].reshape(4, 4), block[16:32].reshape(4, 4)             # element [c, k] multiplies coordinate c into output k
    tanx, tany = block[35], block[36]
    fx, fy = f(W) / (f(2) * tanx), f(H) / (f(2) * tany)
    with np.errstate(all="ignore"):
        pv = p @ view[:3, :3] + view[3, :3]
        ph = p @ proj[:3, :] + proj[3, :]
        pw = f(1) / (ph[:, 3] + f(1e-7))
        ndcx, ndcy = ph[:, 0] * pw, ph[:, 1] * pw
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.stack([f(1) - f(2) * (y * y + z * z), f(2) * (x * y - r * z), f(2) * (x * z + r * y),
                      f(2) * (x * y + r * z), f(1) - f(2) * (x * x + z * z), f(2) * (y * z - r * x),
                      f(2) * (x * z - r * y), f(2) * (y * z + r * x), f(1) - f(2) * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
        M = R * s[:, None, :]
        S = M @ M.transpose(0, 2, 1)
        limx, limy = f(1.3) * tanx, f(1.3) * tany
        tz = pv[:, 2]
        tx = np.clip(pv[:, 0] / tz, -limx, limx) * tz
        ty = np.clip(pv[:, 1] / tz, -limy, limy) * tz
        J0, J2 = fx / tz, -(fx * tx) / (tz * tz)
        J4, J5 = fy / tz, -(fy * ty) / (tz * tz)
        m0 = J0[:, None] * view[:3, 0][None, :] + J2[:, None] * view[:3, 2][None, :]
        m1 = J4[:, None] * view[:3, 1][None, :] + J5[:, None] * view[:3, 2][None, :]
        ms0, ms1 = np.einsum("nc,ncd->nd", m0, S), np.einsum("nc,ncd->nd", m1, S)
        a = (ms0 * m0).sum(1) + f(0.3)
        b = (ms0 * m1).sum(1)
        c = (ms1 * m1).sum(1) + f(0.3)
        det = a * c - b * b
        mid = f(0.5) * (a + c)
        sq = np.sqrt(np.maximum(f(0.1), mid * mid - det))
        lm = np.maximum(mid + sq, mid - sq)
        rad = np.ceil(f(3) * np.sqrt(lm))
        px = ((ndcx + f(1)) * f(W) - f(1)) * f(0.5)
        py = ((ndcy + f(1)) * f(H) - f(1)) * f(0.5)
        rtx, rty = (W + RT - 1) // RT, (H + RT - 1) // RT
        tx0 = np.clip(np.trunc((px - rad) / f(RT)), 0, rtx)
        ty0 = np.clip(np.trunc((py - rad) / f(RT)), 0, rty)
        tx1 = np.clip(np.trunc((px + rad + f(RT - 1)) / f(RT)), 0, rtx)
        ty1 = np.clip(np.trunc((py + rad + f(RT - 1)) / f(RT)), 0, rty)
        return (pv[:, 2] > f(np.float32(0.2))) & (det != 0) & ((tx1 - tx0) * (ty1 - ty0) > 0)


# ---- cameras --------------------------------------------------------------------------------------------------------------------------------
def camera_block(cam):
    """The 37 floats of a camera dict (camera.make_camera) as the rasterizer reads them, from the package's host statement of them."""
    from dreamwaltz_g_amd import camera
    view, proj, campos, tanx, tany = camera.raster_matrices({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in cam.items()})
    return np.concatenate([view.numpy().reshape(-1), proj.numpy().reshape(-1), campos.numpy().reshape(-1),
                           np.array([tanx, tany])]).astype(np.float32)


def box_camera(where, H, W, device="cpu"):
    """A camera of the playback benchmark's geometry (fovy 55) in, at a corner of, or outside the 8 x 3 x 8 m box of box_scene."""
    from dreamwaltz_g_amd import camera
    kw = {"inside": dict(radius=2.4, azimuth=20.0, elevation=80.0), "corner": dict(radius=2.4, azimuth=45.0, elevation=80.0, at=(2.0, 0.0, 2.0)),
          "outside": dict(radius=12.0, azimuth=20.0, elevation=70.0)}[where]
    return camera.make_camera(fovy=55.0, height=H, width=W, device=device, **kw)


def world_from_camera(block, pv):
    """World positions (fp32) whose camera-space coordinates under `block` are pv [N, 3] (float64), up to fp32 rounding."""
    view = np.asarray(block, np.float64)[:16].reshape(4, 4)
    return ((pv - view[3, :3]) @ np.linalg.inv(view[:3, :3])).astype(np.float32)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def _quats(r, n):
    q = r.standard_normal((n, 4)).astype(np.float32)
    q /= np.maximum(np.sqrt((q * q).sum(1, keepdims=True, dtype=np.float32)), np.float32(1e-12))       # F.normalize in fp32
    q[::97] = 0.0                                                                                        # the zero quaternion: R = I
    return q


def box_scene(n, seed=0):
    """The playback benchmark's room: n Gaussians in an 8 x 3 x 8 m box, 1-3 cm across -> (positions, activated scales, quaternions)."""
    r = np.random.RandomState(seed)
    pos = ((r.rand(n, 3) * 2 - 1) * np.array([4.0, 1.5, 4.0])).astype(np.float32)
    return pos, np.exp(r.rand(n, 3) * 1.1 - 5.0).astype(np.float32), _quats(r, n)


def anisotropic_scene(n, seed=1):
    """Log-uniform anisotropic scales 1e-4 .. 5 m, positions in a box twice the room."""
    r = np.random.RandomState(seed)
    pos = ((r.rand(n, 3) * 2 - 1) * np.array([8.0, 3.0, 8.0])).astype(np.float32)
    return pos, np.exp(r.uniform(np.log(1e-4), np.log(5.0), size=(n, 3))).astype(np.float32), _quats(r, n)


def near_plane_cluster(n, block, seed=2):
    """Gaussians whose camera-space depth lies within 1e-5 of the near plane z = 0.2, across and beyond the field of view."""
    r = np.random.RandomState(seed)
    z = 0.2 + r.uniform(-1e-5, 1e-5, size=n)
    pv = np.stack([r.uniform(-0.3, 0.3, size=n), r.uniform(-0.3, 0.3, size=n), z], axis=1)
    return world_from_camera(block, pv), np.exp(r.uniform(np.log(1e-4), np.log(0.05), size=(n, 3))).astype(np.float32), _quats(r, n)


def behind_camera(n, block, seed=3):
    """Everything behind the camera (camera-space z < 0), large Gaussians included."""
    r = np.random.RandomState(seed)
    pv = np.stack([r.uniform(-4, 4, size=n), r.uniform(-4, 4, size=n), -r.uniform(0.01, 8.0, size=n)], axis=1)
    return world_from_camera(block, pv), np.exp(r.uniform(np.log(1e-4), np.log(5.0), size=(n, 3))).astype(np.float32), _quats(r, n)


GENERATORS = ("box_inside", "box_corner", "box_outside", "anisotropic", "near_plane", "behind")


def case(name, n, H, W, seed=0):
    """(positions, scales, quaternions, camera dict) of one named generator."""
    where = {"box_inside": "inside", "box_corner": "corner", "box_outside": "outside"}.get(name, "inside")
    cam = box_camera(where, H, W)
    block = camera_block(cam)
    if name.startswith("box_"):
        arrays = box_scene(n, seed)
    elif name == "anisotropic":
        arrays = anisotropic_scene(n, seed + 1)
    elif name == "near_plane":
        arrays = near_plane_cluster(n, block, seed + 2)
    elif name == "behind":
        arrays = behind_camera(n, block, seed + 3)
    else:
        raise KeyError(name)
    return arrays + (cam,)


def background_arrays(positions, scales, quats, seed=0):
    """GaussianBackground.from_tensors arguments whose ACTIVATED scales and quaternions are the given ones up to fp32 rounding (log and an
    already normalised quaternion), with random colours and mostly opaque opacities."""
    g = torch.Generator().manual_seed(seed)
    n = positions.shape[0]
    u = lambda *s: torch.rand(*s, generator=g)           # noqa: E731
    return dict(positions=torch.from_numpy(np.ascontiguousarray(positions)), sh_features_dc=u(n, 1, 3) * 3 - 1.5,
                sh_features_rest=(u(n, 15, 3) - 0.5) * 0.4, opacities=u(n, 1) * 6 - 1,
                scales=torch.log(torch.from_numpy(np.ascontiguousarray(scales))), quaternions=torch.from_numpy(np.ascontiguousarray(quats)))


# ---- csrc/cull_math.h on the host ---------------------------------------------------------------------------------------------------------------
def _sources():
    here = os.path.join(ROOT, "tests", "hostmath")
    hdrs = [os.path.join(ROOT, "dreamwaltz-g_amd", "csrc", h) for h in ("cull_math.h", "scene_cull_args.h")]
    return here, os.path.join(here, "cull_math_host.cpp"), hdrs + [os.path.join(ROOT, "include", "dwg_scene_cull.h")]


def hostlib():
    """csrc/cull_math.h and csrc/scene_cull_args.h compiled by g++ (tests/hostmath/cull_math_host.cpp)."""
    here, src, hdrs = _sources()
    out = os.path.join(here, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libcull_math_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror", "-o", so, src, "-lm"], check=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.host_cull_flags.argtypes = [ctypes.c_int64, vp, vp, ctypes.c_int32, vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp]
    L.host_cull_flags.restype = None
    L.host_cull_check_flags.argtypes = [ctypes.c_int64, vp, vp, ctypes.c_int32, vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp]
    L.host_cull_check_compact.argtypes = [ctypes.c_int64, vp, vp, vp, vp]
    L.host_cull_check_gather.argtypes = [ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32, vp]
    return L


def host_flags(L, positions, scales, blocks, H, W):
    """uint8 [N]: the flags of dwg_scene_cull_flags from the host build; blocks [C, 37]."""
    p, s, b = (np.ascontiguousarray(a, dtype=np.float32) for a in (positions, scales, np.atleast_2d(blocks)))
    out = np.zeros(p.shape[0], np.uint8)
    L.host_cull_flags(p.shape[0], p.ctypes.data, s.ctypes.data, b.shape[0], b.ctypes.data, b.shape[1], H, W, out.ctypes.data)
    return out
