"""CPU checks of the avatar-construction boundary (B11, include/dwg_avatar_init.h, dreamwaltz_g_amd.avatar_init): argument errors are
reported before any launch, empty calls launch nothing, the Python functions refuse CPU tensors, wrong dtypes and a K out of range, the
float64 oracles check themselves, and the binding of the reference's find_nearest_triangles / knn_points / LBSUtils.initialize_lbs_weights
(in a subprocess with the real reference modules; skipped when the reference tree is absent)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from tests import avatar_init_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
REFERENCE = "/root/reference"

FAKE = ctypes.c_void_p(4096)          # aligned, never dereferenced: every call below must fail (or succeed) before a launch
FAKE2 = ctypes.c_void_p(1 << 30)
FAKE3 = ctypes.c_void_p(1 << 31)
E = -1


def _each_null(fn, base, positions):
    for k in positions:
        args = list(base)
        args[k] = None
        assert fn(*args) == E, k


def test_bad_arguments_return_arg_error_before_any_launch():
    L = _lib.lib()
    b = [4, FAKE, FAKE, 8, FAKE, 6, FAKE, FAKE, FAKE, FAKE, None]
    _each_null(L.dwg_avinit_barycentric, b, (1, 2, 4, 6, 7, 8, 9))
    for k in (0, 3, 5):
        args = list(b)
        args[k] = -1
        assert L.dwg_avinit_barycentric(*args) == E, k
    i = [4, 55, 8, FAKE, FAKE, FAKE, FAKE, None]
    _each_null(L.dwg_avinit_lbs_interp, i, (3, 4, 5, 6))
    for k in (0, 1, 2):
        args = list(i)
        args[k] = -1
        assert L.dwg_avinit_lbs_interp(*args) == E, k
    k_ = [100, FAKE, 200, FAKE, 30, FAKE, FAKE, None]
    _each_null(L.dwg_avinit_knn, k_, (1, 3, 5, 6))
    for K in (0, -1, 65, 201):
        args = list(k_)
        args[4] = K
        assert L.dwg_avinit_knn(*args) == E, K
    assert L.dwg_avinit_knn(100, FAKE, 64, FAKE, 65, FAKE, FAKE, None) == E
    assert L.dwg_avinit_knn(100, FAKE, 29, FAKE, 30, FAKE, FAKE, None) == E           # K > Nr
    assert L.dwg_avinit_knn(-1, FAKE, 200, FAKE, 30, FAKE, FAKE, None) == E
    assert L.dwg_avinit_knn(100, FAKE, -1, FAKE, 30, FAKE, FAKE, None) == E
    w = [100, 30, FAKE, FAKE, FAKE, 1, 0.01, 0.01, FAKE, FAKE, None]
    _each_null(L.dwg_avinit_knn_weights, w, (2, 3, 4, 8, 9))
    for bad in ((0, -1), (1, 0), (1, 65), (6, 0.02), (6, float('nan')), (7, float('nan'))):        # high < low, NaN thresholds
        args = list(w)
        args[bad[0]] = bad[1]
        assert L.dwg_avinit_knn_weights(*args) == E, bad
    s = [100, 55, 30, FAKE, FAKE, FAKE, FAKE, FAKE2, FAKE3, 5, None]
    _each_null(L.dwg_avinit_smooth, s, (3, 4, 5, 6, 7, 8))
    for bad in ((0, -1), (1, -1), (2, 0), (2, 65), (9, -1)):
        args = list(s)
        args[bad[0]] = bad[1]
        assert L.dwg_avinit_smooth(*args) == E, bad
    # overlapping buffers: in == out, tmp == in, tmp == out, and a partial overlap (100 x 55 x 4 bytes each)
    for a_in, a_tmp, a_out in ((FAKE, FAKE2, FAKE), (FAKE, FAKE, FAKE3), (FAKE, FAKE3, FAKE3), (FAKE, FAKE2, ctypes.c_void_p(4096 + 21996))):
        args = list(s)
        args[6], args[7], args[8] = a_in, a_tmp, a_out
        assert L.dwg_avinit_smooth(*args) == E
    # a scratch buffer is needed from the second sweep on only
    args = list(s)
    args[7], args[9] = None, 2
    assert L.dwg_avinit_smooth(*args) == E


def test_empty_calls_launch_nothing():
    L = _lib.lib()
    assert L.dwg_avinit_barycentric(0, None, None, 0, None, 0, None, None, None, None, None) == 0
    assert L.dwg_avinit_lbs_interp(0, 55, 8, None, None, None, None, None) == 0
    assert L.dwg_avinit_lbs_interp(4, 0, 8, None, None, None, None, None) == 0
    assert L.dwg_avinit_knn(0, None, 200, None, 30, None, None, None) == 0
    assert L.dwg_avinit_knn_weights(0, 30, None, None, None, 1, 0.01, 0.01, None, None, None) == 0
    assert L.dwg_avinit_smooth(0, 55, 30, None, None, None, None, None, None, 5000, None) == 0
    assert L.dwg_avinit_smooth(100, 0, 30, None, None, None, None, None, None, 5000, None) == 0


def test_python_functions_refuse_cpu_tensors_wrong_dtypes_and_k_out_of_range():
    from dreamwaltz_g_amd import avatar_init as ai
    V, F = ac.make_sphere()
    Vt, Ft, P = torch.from_numpy(V), torch.from_numpy(F), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        ai.find_nearest_triangles(P, Vt, Ft)
    with pytest.raises(RuntimeError, match="float32|CUDA"):
        ai.find_nearest_triangles(P.double(), Vt, Ft)
    with pytest.raises(RuntimeError):
        ai.find_nearest_triangles(P, Vt, Ft.float())
    with pytest.raises(RuntimeError, match="CUDA"):
        ai.knn(P, P, 2)
    with pytest.raises(RuntimeError, match="CUDA"):
        ai.knn_points(P[None], P[None], K=2)
    with pytest.raises(RuntimeError):
        ai.knn_points(P, P, K=2)                                      # no batch dimension
    with pytest.raises(RuntimeError, match="CUDA"):
        ai.initialize_lbs_weights(torch.zeros(len(V), 55), {'vertex_indices': torch.zeros(4, 3, dtype=torch.int64),
                                                          'barycentric_coords': torch.zeros(4, 3)})
    with pytest.raises(RuntimeError, match="CUDA"):
        ai.smooth_sweeps(torch.zeros(4, 55), torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2), torch.zeros(4), 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ai.knn_weights(torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2), torch.zeros(4))
    for K in (0, 65, -3):                                             # the range of K is refused before anything else
        with pytest.raises(RuntimeError, match="K = "):
            ai.knn(P, P, K)
        with pytest.raises(RuntimeError, match="K = "):
            ai.knn_points(P[None], P[None], K=K)


def test_prune_points_close_to_mesh_is_the_reference_statement():
    from dreamwaltz_g_amd import avatar_init as ai
    pos = torch.arange(18, dtype=torch.float32).reshape(6, 3)
    buf = {'squared_distances': torch.tensor([1e-6, 4e-4, 1e-6, 9e-2, 1e-6, 1e-6]), 'triangle_indices': torch.tensor([3, 3, 7, 5, 9, 5]),
           'vertex_indices': torch.arange(18).reshape(6, 3), 'nearest_vertex_indices': torch.arange(6),
           'barycentric_coords': torch.rand(6, 3)}
    keep_b = buf['barycentric_coords'].clone()
    p2, b2 = ai.prune_points_close_to_mesh(pos, buf, torch.tensor([3, 5]), threshold=0.01)
    # faces 3 / 5 and closer than 0.01: rows 0 and 5 go; row 1 (d = 0.02) and row 3 (d = 0.3) stay
    assert b2 is buf and p2.tolist() == pos[[1, 2, 3, 4]].tolist()
    assert b2['triangle_indices'].tolist() == [3, 7, 5, 9] and b2['nearest_vertex_indices'].tolist() == [1, 2, 3, 4]
    assert torch.equal(b2['barycentric_coords'], keep_b[[1, 2, 3, 4]]) and b2['vertex_indices'].shape == (4, 3)
    p3, b3 = ai.prune_points_close_to_mesh(p2, b2, [3, 5], threshold=None)
    assert p3.tolist() == pos[[2, 4]].tolist() and b3['triangle_indices'].tolist() == [7, 9]


def test_oracles_check_themselves():
    """Ericson's regions against the enumeration (interior projection, three edges, three corners); KNN against a full sort; one smoothing
    sweep against a loop."""
    rng = np.random.default_rng(0)
    A, B, C = rng.normal(size=(3, 500, 3))
    P = rng.normal(size=(500, 3)) * 2
    q, bary = ac.closest_on_triangles(P, A, B, C)
    assert np.abs(np.einsum('nk,nkc->nc', bary, np.stack([A, B, C], 1)) - q).max() < 1e-12 and bary.min() > -1e-12
    cands = []
    n = np.cross(B - A, C - A)
    proj = P - ((P - A) * n).sum(-1, keepdims=True) / (n * n).sum(-1, keepdims=True) * n
    _, pb = ac.closest_on_triangles(proj, A, B, C)
    inside = np.abs(np.einsum('nk,nkc->nc', pb, np.stack([A, B, C], 1)) - proj).max(-1) < 1e-9
    cands.append(np.where(inside, ((proj - P) ** 2).sum(-1), np.inf))
    for X, Y in ((A, B), (B, C), (C, A)):
        t = np.clip(((P - X) * (Y - X)).sum(-1) / ((Y - X) ** 2).sum(-1), 0, 1)
        cands.append(((X + t[:, None] * (Y - X) - P) ** 2).sum(-1))
    assert np.abs(np.min(cands, 0) - ((q - P) ** 2).sum(-1)).max() < 1e-10
    L = ac.lattice(5)
    idx, d2 = ac.knn(L, L, 7)
    full = ((L[:, None].astype(np.float64) - L[None]) ** 2).sum(-1)
    for r in (0, 62, 124):
        order = sorted(range(len(L)), key=lambda j: (full[r, j], j))[:7]
        assert idx[r].tolist() == order and (d2[r] == full[r, order]).all()
    w = ac.sparse_table(20, 5, seed=1).astype(np.float64)
    nb = np.stack([np.roll(np.arange(20), s) for s in (1, 2, 3)], 1)
    a, u = ac.smoothing_weights(nb, rng.uniform(0.01, 0.1, (20, 3)), rng.uniform(1e-5, 4e-4, 20), low=0.01)
    assert np.abs(a.sum(1) - 1).max() < 1e-14 and set(np.unique(u)) == {0.0, 1.0}
    one = ac.smooth(w, nb, a, u, 1)
    for r in range(20):
        want = w[r] if u[r] == 0 else sum(a[r, k] * w[nb[r, k]] for k in range(3))
        assert np.abs(one[r] - want).max() < 1e-15
    assert np.abs(ac.smooth(w, nb, a, u, 3) - ac.smooth(ac.smooth(w, nb, a, u, 2), nb, a, u, 1)).max() == 0


_BIND_CODE = r"""
import inspect, json, os, sys
sys.dont_write_bytecode = True
ROOT, DROPIN, REF = %r, %r, %r
sys.path.insert(0, ROOT); sys.path.insert(0, DROPIN); sys.path.insert(0, os.path.join(ROOT, "tests", "golden")); sys.path.insert(0, REF)
from oracle import animate as oa
import _ref_stubs
_ref_stubs.install(oa)
import torch
import core.system.avatar as am                      # imported BEFORE the hooks: install() patches what is already there
ref = {"fnt": am.find_nearest_triangles, "knn": am.knn_points, "init": am.LBSUtils.__dict__["initialize_lbs_weights"]}
calls = []
def fnt_stub(points, vertices, triangles, device=None):
    calls.append("fnt"); return {"stub": True}
def knn_stub(query_points, reference_points, K=3, device=None):
    calls.append(("knn", K)); return "knn-stub"
def init_stub(lbs_model, nearest_triangles_buffer, positions=None, smooth=False, smooth_K=None, smooth_N=None, use_sqrt=True,
              valid_dist_threshold=0.01):
    calls.append(("init", smooth_K)); return "init-stub"
import dwg_bind
dwg_bind.install()
out = {}
f, k, i = am.find_nearest_triangles, am.knn_points, am.LBSUtils.__dict__["initialize_lbs_weights"]
out["patched"] = [bool(getattr(x, "__dwg_bound__", False)) for x in (f, k, getattr(i, "__func__", i))]
out["static"] = isinstance(i, staticmethod)
out["wrapped_is_reference"] = (getattr(f, "__wrapped__", None) is ref["fnt"] and getattr(k, "__wrapped__", None) is ref["knn"]
                               and getattr(getattr(i, "__func__", i), "__wrapped__", None) is ref["init"].__func__)
out["same_signatures"] = all(str(inspect.signature(a)) == str(inspect.signature(b)) for a, b in
                             ((f, ref["fnt"]), (k, ref["knn"]), (i.__func__, ref["init"].__func__)))
out["subclass_sees_it"] = am.DreamWaltzG.initialize_lbs_weights is am.LBSUtils.initialize_lbs_weights
out["avatar_still_hooked"] = bool(getattr(am.build_gaussian_avatar, "__dwg_bound__", False))
dwg_bind.uninstall()
out["restored"] = (am.find_nearest_triangles is ref["fnt"] and am.knn_points is ref["knn"]
                   and am.LBSUtils.__dict__["initialize_lbs_weights"].__func__ is ref["init"].__func__
                   and isinstance(am.LBSUtils.__dict__["initialize_lbs_weights"], staticmethod))
# without a device the wrappers call what they wrapped: stubs in the originals' places, the device probe answering "none"
am.find_nearest_triangles, am.knn_points = fnt_stub, knn_stub
am.LBSUtils.initialize_lbs_weights = staticmethod(init_stub)
dwg_bind.install()
dwg_bind._hip_device = lambda: None
r1 = am.find_nearest_triangles(torch.zeros(2, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.long))
r2 = am.knn_points(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3), K=2)
r3 = am.LBSUtils.initialize_lbs_weights(None, {}, smooth_K=11)
r4 = am.DreamWaltzG.initialize_lbs_weights(None, {}, smooth_K=12)
out["fallback"] = [r1, r2, r3, r4]
out["calls"] = calls
out["rewrapped"] = bool(getattr(am.knn_points, "__dwg_bound__", False))
print(json.dumps(out))
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core")), reason="reference tree not present")
def test_b11_binding_of_the_reference_avatar_module():
    code = _BIND_CODE % (ROOT, DROPIN, REFERENCE)
    env = dict(os.environ)
    env.pop("DWG_BIND_INIT", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["patched"] == [True, True, True] and out["static"] and out["wrapped_is_reference"] and out["same_signatures"], out
    assert out["subclass_sees_it"] and out["avatar_still_hooked"] and out["restored"], out
    assert out["fallback"] == [{"stub": True}, "knn-stub", "init-stub", "init-stub"] and out["rewrapped"], out
    assert out["calls"] == ["fnt", ["knn", 2], ["init", 11], ["init", 12]], out
    env["DWG_BIND_INIT"] = "0"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["patched"] == [False, False, False] and out["static"] and out["avatar_still_hooked"], out
    assert out["fallback"] == [{"stub": True}, "knn-stub", "init-stub", "init-stub"] and not out["rewrapped"], out      # the stubs themselves
