"""Host-only checks of the NeRF-stage ray marcher seam (boundary B6): the drop-in modules' surface and argument checks, the
self-consistency of the CPU restatement (tests/raymarch_cases.py), and -- when the reference tree is present -- that its raymarching.py
binds to our modules through PYTHONPATH without building anything."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import raymarch_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
REFERENCE = "/root/reference"
NAMES = {"flatten_rays", "packbits", "near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "march_rays_train",
         "composite_rays_train_forward", "composite_rays_train_backward", "march_rays", "composite_rays"}


def _modules():
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import _raymarchinglatent
    import _raymarchingrgb
    return _raymarchingrgb, _raymarchinglatent


def test_dropins_import_and_expose_the_binding_names():
    for m in _modules():
        public = {n for n in dir(m) if not n.startswith("_")}
        assert public == NAMES, sorted(public ^ NAMES)
        assert all(callable(getattr(m, n)) for n in NAMES)
    rgb, lat = _modules()
    co = rgb.composite_rays_train_forward.__code__
    assert co.co_varnames[:co.co_argcount] == ("sigmas", "rgbs", "ts", "rays", "M", "N", "T_thresh", "binarize", "weights", "weights_sum",
                                               "depth", "image")
    co = lat.composite_rays.__code__
    assert "binarize" not in co.co_varnames[:co.co_argcount] and co.co_argcount == 11
    co = rgb.march_rays_train.__code__
    assert co.co_argcount == 18 and co.co_varnames[12:15] == ("xyzs", "dirs", "ts")


def _calls(m, latent, t):
    """every backend function with buffers built by t(shape, dtype)"""
    f, i, u8 = torch.float32, torch.int32, torch.uint8
    N, M = 4, 6
    b = () if latent else (False,)
    ch = 4 if latent else 3
    return [
        lambda: m.flatten_rays(t((N, 2), i), N, M, t((M,), i)),
        lambda: m.packbits(t((64,), f), 8, 0.5, t((8,), u8)),
        lambda: m.near_far_from_aabb(t((N, 3), f), t((N, 3), f), t((6,), f), N, 0.05, t((N,), f), t((N,), f)),
        lambda: m.sph_from_ray(t((N, 3), f), t((N, 3), f), 2.0, N, t((N, 2), f)),
        lambda: m.morton3D(t((N, 3), i), N, t((N,), i)),
        lambda: m.morton3D_invert(t((N,), i), N, t((N, 3), i)),
        lambda: m.march_rays_train(t((N, 3), f), t((N, 3), f), t((2 * 16 ** 3 // 8,), u8), 1.0, False, 0.0, 64, N, 2, 16, t((N,), f),
                                   t((N,), f), None, None, None, t((N, 2), i), t((1,), i), t((N,), f)),
        lambda: m.composite_rays_train_forward(t((M,), f), t((M, ch), f), t((M, 2), f), t((N, 2), i), M, N, 1e-4, *b, t((M,), f), t((N,), f),
                                               t((N,), f), t((N, ch), f)),
        lambda: m.composite_rays_train_backward(t((M,), f), t((N,), f), t((N,), f), t((N, ch), f), t((M,), f), t((M, ch), f), t((M, 2), f),
                                                t((N, 2), i), t((N,), f), t((N,), f), t((N, ch), f), M, N, 1e-4, *b, t((M,), f), t((M, ch), f)),
        lambda: m.march_rays(N, 2, t((N,), i), t((N,), f), t((N, 3), f), t((N, 3), f), 1.0, False, 0.0, 64, 2, 16, t((2 * 16 ** 3 // 8,), u8),
                             t((N,), f), t((N,), f), t((2 * N, 3), f), t((2 * N, 3), f), t((2 * N, 2), f), t((N,), f)),
        lambda: m.composite_rays(N, 2, 1e-2, *b, t((N,), i), t((N,), f), t((2 * N,), f), t((2 * N, ch), f), t((2 * N, 2), f), t((N,), f),
                                 t((N,), f), t((N, ch), f)),
    ]


@pytest.mark.parametrize("latent", [False, True])
def test_every_function_rejects_cpu_tensors(latent):
    m = _modules()[int(latent)]
    calls = _calls(m, latent, lambda s, d: torch.zeros(s, dtype=d))
    assert len(calls) == 11
    for c in calls:
        with pytest.raises(RuntimeError, match="CUDA"):
            c()


@pytest.mark.gpu
@pytest.mark.parametrize("latent", [False, True])
def test_every_function_rejects_wrong_dtypes_and_sizes(latent):
    m = _modules()[int(latent)]
    dev = torch.device("cuda")

    def wrong_dtype(s, d):
        return torch.zeros(s, dtype=torch.int64 if d != torch.int64 else torch.float32, device=dev)

    def wrong_size(s, d):
        s = (s[0] + 1,) + tuple(s[1:])
        return torch.zeros(s, dtype=d, device=dev)
    for maker in (wrong_dtype, wrong_size):
        for c in _calls(m, latent, maker):
            with pytest.raises(RuntimeError):
                c()


def test_non_contiguous_rejected_before_the_device_check():
    rgb, _ = _modules()
    x = torch.zeros(4, 6)[:, ::2]
    with pytest.raises(RuntimeError):
        rgb.near_far_from_aabb(x, x, torch.zeros(6), 4, 0.05, torch.zeros(4), torch.zeros(4))


def test_morton_round_trip():
    rng = np.random.RandomState(0)
    c = rng.randint(0, 1024, size=(5000, 3))
    idx = rc.morton3d(c[:, 0], c[:, 1], c[:, 2])
    assert np.array_equal(rc.morton3d_invert(idx), c)
    H = 8
    allc = rc.morton3d_invert(np.arange(H ** 3))
    assert np.array_equal(rc.morton3d(allc[:, 0], allc[:, 1], allc[:, 2]), np.arange(H ** 3))
    assert allc.max() == H - 1 and len({tuple(v) for v in allc}) == H ** 3


def test_packbits_restatement():
    g = np.arange(32, dtype=np.float32) % 3
    b = rc.packbits(g, 1.5)
    for j in range(4):
        for i in range(8):
            assert ((b[j] >> i) & 1) == (g[8 * j + i] > 1.5)


@pytest.mark.parametrize("binarize", [False])
def test_composite_formula_equals_autograd_of_the_forward(binarize):
    """with grad_weights = 0 the reference's formula is the exact gradient of (weights_sum, depth, image) in float64, as long as the
    stop sample does not move (T_thresh tiny here)"""
    rng = np.random.RandomState(1)
    counts = np.array([0, 1, 7, 40, 3])
    rays = np.stack([np.concatenate([[0], np.cumsum(counts)[:-1]]), counts], 1)
    M, N, C = counts.sum(), len(counts), 3
    sig = rng.uniform(0, 30, M); rgb = rng.uniform(0, 1, (M, C))
    ts = np.stack([np.cumsum(rng.uniform(0.005, 0.02, M)), rng.uniform(0.005, 0.02, M)], 1)
    gws, gd, gi = rng.randn(N), rng.randn(N), rng.randn(N, C)
    gs, gr = rc.composite_backward(np.zeros(M), gws, gd, gi, sig, rgb, ts, rays, 1e-12, binarize)
    s_t = torch.tensor(sig, requires_grad=True); r_t = torch.tensor(rgb, requires_grad=True)
    loss = 0
    for n in range(N):
        off, cnt = rays[n]
        if cnt == 0:
            continue
        a = 1 - torch.exp(-s_t[off:off + cnt] * torch.tensor(ts[off:off + cnt, 1]))
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1 - a[:-1]]), 0)
        w = a * T
        loss = loss + gws[n] * w.sum() + gd[n] * (w * torch.tensor(ts[off:off + cnt, 0])).sum() + (torch.tensor(gi[n]) * (w[:, None] * r_t[off:off + cnt]).sum(0)).sum()
    loss.backward()
    assert np.allclose(gs, s_t.grad.numpy(), rtol=1e-9, atol=1e-12)
    assert np.allclose(gr, r_t.grad.numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("contract,dt_gamma", [(False, 0.0), (True, 1.0 / 256)])
def test_march_restatement_is_self_consistent(contract, dt_gamma):
    C, H, bound, max_steps = 2, 32, 2.0, 256
    grid, bits = rc.make_grid(C, H, bound)
    o, d = rc.make_cameras(1, 24, 24, seed=3)
    nears, fars = rc.near_far(o, d, np.array([-bound] * 3 + [bound] * 3), 0.05)
    noises = np.random.RandomState(0).rand(len(o)).astype(np.float32)
    counts, xyzs, dirs, ts = rc.march_train(o, d, bits, bound, contract, dt_gamma, max_steps, C, H, nears, fars, noises)
    assert counts.sum() == len(xyzs) > 0 and counts.max() <= max_steps
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    for n in np.nonzero(counts)[0]:
        t = ts[offs[n]:offs[n] + counts[n], 0]
        assert np.all(np.diff(t) > 0), n
        assert np.array_equal(dirs[offs[n]], d[n])
    # every sample lies in an occupied cell: recompute the cell of the sample's pre-step position from t - dt
    mr = rc._Marcher(o, d, bits, bound, contract, dt_gamma, max_steps, C, H)
    ray = np.repeat(np.arange(len(o)), counts)
    tn, occ, cx, cy, cz, dt = mr.iterate(ray, (ts[:, 0] - ts[:, 1]).astype(np.float32))
    ok = occ | (np.abs(tn - ts[:, 0]) > 0)     # t - dt is the pre-step t up to one rounding; it lands in the same cell
    assert occ.mean() > 0.99 and ok.all()


def test_near_far_restatement_cases():
    o = np.array([[0, 0, -3], [0, 0, 0], [5, 5, 5], [0.5, 0, -3]], np.float32)
    d = np.array([[0, 0, 1], [1, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    n, f = rc.near_far(o, d, np.array([-1, -1, -1, 1, 1, 1], np.float32), 0.05)
    assert n[0] == 2 and f[0] == 4
    assert n[1] == np.float32(0.05) and f[1] == 1
    assert n[2] == f[2] == rc.FLT_MAX
    assert n[3] == 2 and f[3] == 4


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core", "nerf", "raymarching")), reason="reference tree not present")
def test_reference_get_backend_binds_to_the_dropins():
    code = r"""
import sys, types
sys.path.insert(0, %r)
sys.path.insert(1, %r)
import torch.utils.cpp_extension as ce
def _refuse(*a, **k):
    raise SystemExit("cpp_extension.load was called")
ce.load = _refuse
import importlib.util
for variant, name in (("rgb", "_raymarchingrgb"), ("latent", "_raymarchinglatent")):
    path = %r + "/core/nerf/raymarching/" + variant + "/raymarching.py"
    spec = importlib.util.spec_from_file_location("ref_raymarching_" + variant, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    be = mod.get_backend()
    assert be.__name__ == name and be.__file__.startswith(%r), (be.__name__, be.__file__)
print("BOUND")
""" % (DROPIN, ROOT, REFERENCE, DROPIN)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "BOUND" in r.stdout, r.stdout + r.stderr
