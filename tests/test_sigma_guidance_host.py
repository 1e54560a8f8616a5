"""CPU checks of the sigma guidance boundary (B8, include/dwg_sigma.h, dreamwaltz_g_amd.sigma_guidance): argument errors are reported
before any launch, empty calls launch nothing, the Python wrappers refuse CPU tensors and wrong dtypes, the float64 restatement
checks itself, and the binding of the reference's Trainer.calc_sigma_loss (in a subprocess; skipped when the reference tree is absent)."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from tests import sigma_guidance_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
REFERENCE = "/root/reference"

FAKE = ctypes.c_void_p(4096)          # 16-byte aligned, never dereferenced: every call below must fail (or succeed) before a launch
ODD = ctypes.c_void_p(4100)


def test_bad_arguments_return_arg_error_before_any_launch():
    L = _lib.lib()
    E = -1
    # face records
    assert L.dwg_sigma_face_records(-1, FAKE, 4, FAKE, FAKE, None, None) == E
    assert L.dwg_sigma_face_records(4, FAKE, -1, FAKE, FAKE, None, None) == E
    assert L.dwg_sigma_face_records(4, None, 4, FAKE, FAKE, None, None) == E
    assert L.dwg_sigma_face_records(4, FAKE, 4, None, FAKE, None, None) == E
    assert L.dwg_sigma_face_records(4, FAKE, 4, FAKE, None, None, None) == E
    assert L.dwg_sigma_face_records(4, FAKE, 4, FAKE, ODD, None, None) == E
    # area CDF
    assert L.dwg_sigma_area_cdf(-1, FAKE, FAKE, None) == E
    assert L.dwg_sigma_area_cdf(4, None, FAKE, None) == E and L.dwg_sigma_area_cdf(4, FAKE, None, None) == E
    # vertex normals
    assert L.dwg_sigma_vertex_normals(-1, FAKE, FAKE, FAKE, FAKE, FAKE, None) == E
    for k in range(5):
        args = [FAKE] * 5
        args[k] = None
        assert L.dwg_sigma_vertex_normals(4, *args, None) == E, k
    # sample
    base = [4, FAKE, 4, FAKE, 4, FAKE, FAKE, FAKE, 0.05, FAKE, FAKE, FAKE, FAKE, None]
    for k in (1, 3, 5, 6, 7, 9, 10, 11, 12):
        args = list(base)
        args[k] = None
        assert L.dwg_sigma_sample(*args) == E, k
    for k in (0, 2, 4):
        args = list(base)
        args[k] = -1
        assert L.dwg_sigma_sample(*args) == E, k
    args = list(base)
    args[4] = 0                                                            # samples need a face
    assert L.dwg_sigma_sample(*args) == E
    args = list(base)
    args[8] = float('nan')
    assert L.dwg_sigma_sample(*args) == E
    # distance
    need = L.dwg_sigma_distance_workspace_bytes(5000, 20480)
    assert need > 0 and L.dwg_sigma_distance_workspace_bytes(0, 20480) == 0 and L.dwg_sigma_distance_workspace_bytes(5000, 0) == 0
    assert L.dwg_sigma_distance_workspace_bytes(-3, 7) == 0
    d = [5000, FAKE, 20480, FAKE, FAKE, FAKE, FAKE, FAKE, need, None]
    for k in (1, 3, 4, 5, 7):
        args = list(d)
        args[k] = None
        assert L.dwg_sigma_point_mesh_distance(*args) == E, k
    for k in (3, 7):
        args = list(d)
        args[k] = ODD
        assert L.dwg_sigma_point_mesh_distance(*args) == E, k
    args = list(d)
    args[8] = need - 1
    assert L.dwg_sigma_point_mesh_distance(*args) == E
    args = list(d)
    args[2] = 0
    assert L.dwg_sigma_point_mesh_distance(*args) == E
    assert L.dwg_sigma_point_mesh_distance(-1, FAKE, 4, FAKE, FAKE, FAKE, None, FAKE, need, None) == E
    # keep mask
    m = [4, FAKE, FAKE, 0.005, 4, None, FAKE, FAKE, None]
    for k in (1, 2, 6, 7):
        args = list(m)
        args[k] = None
        assert L.dwg_sigma_keep_mask(*args) == E, k
    args = list(m)
    args[3] = float('nan')
    assert L.dwg_sigma_keep_mask(*args) == E
    assert L.dwg_sigma_keep_mask(-1, FAKE, FAKE, 0.005, 4, None, FAKE, FAKE, None) == E


def test_empty_calls_launch_nothing():
    """N = 0 points or P = 0 faces / vertices: success without touching a pointer (all NULL here)."""
    L = _lib.lib()
    assert L.dwg_sigma_face_records(0, None, 0, None, None, None, None) == 0
    assert L.dwg_sigma_area_cdf(0, None, None, None) == 0
    assert L.dwg_sigma_vertex_normals(0, None, None, None, None, None, None) == 0
    assert L.dwg_sigma_sample(0, None, 0, None, 0, None, None, None, 0.05, None, None, None, None, None) == 0
    assert L.dwg_sigma_point_mesh_distance(0, None, 0, None, None, None, None, None, 0, None) == 0
    assert L.dwg_sigma_keep_mask(0, None, None, 0.005, 0, None, None, None, None) == 0


def test_python_wrappers_raise_on_cpu_tensors_and_wrong_dtypes():
    from dreamwaltz_g_amd import sigma_guidance as sg
    V, F = sc.make_icosphere(1)
    Vt, Ft, P = torch.from_numpy(V), torch.from_numpy(F), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        sg.point_mesh_squared_distance(P, Vt, Ft)
    with pytest.raises(RuntimeError, match="CUDA"):
        sg.sample_surface(Vt, Ft, 10)
    with pytest.raises(RuntimeError, match="float32|CUDA"):
        sg.point_mesh_squared_distance(P.double(), Vt, Ft)
    with pytest.raises(RuntimeError):
        sg.sample_surface(Vt.double(), Ft, 10)
    with pytest.raises(RuntimeError):
        sg.sample_surface(Vt, Ft.float(), 10)
    with pytest.raises(RuntimeError, match="outside"):
        sg.PartMesh(np.array([[0, 1, 99]]), 10, "cpu")


def test_part_mesh_csr_table_lists_incident_corners_in_face_order():
    from dreamwaltz_g_amd import sigma_guidance as sg
    V, F = sc.make_icosphere(3)
    pf, wf = sc.make_part(V, F)
    part = sg.PartMesh(F[pf], len(V), "cpu", wrist=np.isin(pf, wf), part_fids=pf)
    off, items = part.vf_offsets.numpy(), part.vf_items.numpy()
    assert off[0] == 0 and off[-1] == 3 * len(pf)
    f = F[pf]
    for v in range(len(V)):
        it = items[off[v]:off[v + 1]]
        assert np.all(np.diff(it) > 0)
        assert np.all(f.reshape(-1)[it] == v)
        assert len(it) == int((f == v).sum())
    assert part.wrist.numpy().sum() == len(wf) > 0


def test_restatement_closest_point_equals_enumeration():
    """Ericson's regions in float64 against the interior projection + every edge + every vertex, including degenerate faces."""
    V, F = sc.make_icosphere(3)
    V, F = sc.add_degenerate(V, F)
    g = torch.Generator().manual_seed(0)
    n = 6000
    P = torch.rand(n, 3, generator=g, dtype=torch.float64) * 2.6 - 1.3
    fid = torch.randint(0, len(F), (n,), generator=g)
    fid[:800] = torch.arange(len(F) - 4, len(F)).repeat(200)
    d_a, q_a = sc.point_face_d2(P, V, F, fid)
    d_b, q_b = sc.point_face_d2(P, V, F, fid, enumerated=True)
    assert float((q_a - q_b).abs().max()) <= 1e-12
    assert float((d_a - d_b).abs().max()) <= 1e-12
    # points on the faces themselves: distance zero
    lam = torch.rand(n, 3, generator=g, dtype=torch.float64)
    lam = lam / lam.sum(1, keepdim=True)
    tri = torch.from_numpy(V).double()[torch.from_numpy(F)[fid]]
    on = (lam[:, :, None] * tri).sum(1)
    d_on, _ = sc.point_face_d2(on, V, F, fid)
    assert float(d_on.max()) <= 1e-24


def test_restatement_samples_lie_in_their_triangles():
    V, F = sc.make_icosphere(3)
    draws = sc.stratified_draws(5000, seed=3)
    pts, fid, pn, noisy = sc.sample(V, F, draws, 0.05)
    d2, _ = sc.point_face_d2(pts, V, F, fid)
    assert float(d2.max()) <= 1e-26
    assert float((pn.norm(dim=1) - 1).abs().max()) <= 1e-12
    off = (noisy - pts).norm(dim=1)
    assert float(off.max()) <= 0.025 + 1e-12
    # a point normal on a sphere's part mesh points outwards
    assert float((pn * pts).sum(1).min()) > 0.9


def test_restatement_part_boundary_normals_differ_from_the_whole_mesh():
    V, F = sc.make_icosphere(3)
    pf, _ = sc.make_part(V, F)
    whole, part = sc.vertex_normals(V, F), sc.vertex_normals(V, F[pf])
    rim = np.unique(F[pf].reshape(-1))
    diff = (whole[rim] - part[rim]).norm(dim=1)
    assert float(diff.max()) > 1e-3                                # boundary vertices see only the part's faces
    assert float(part[np.setdiff1d(np.arange(len(V)), rim)].abs().max()) == 0.0


_BIND_CODE = r"""
import inspect, json, os, sys
sys.dont_write_bytecode = True
ROOT, DROPIN, REF = %r, %r, %r
sys.path.insert(0, ROOT); sys.path.insert(0, DROPIN); sys.path.insert(0, os.path.join(ROOT, "tests", "golden")); sys.path.insert(0, REF)
from oracle import animate as oa
import _ref_stubs
_ref_stubs.install(oa)
import dwg_bind
dwg_bind.install()
import core.trainer as tr
f = tr.Trainer.calc_sigma_loss
orig = getattr(f, "__wrapped__", None)
out = {"patched": bool(getattr(f, "__dwg_bound__", False)),
       "sig": str(inspect.signature(f)),
       "orig_sig": str(inspect.signature(orig)) if orig is not None else None,
       "orig_is_reference": orig is not None and orig.__module__ == "core.trainer" and not getattr(orig, "__dwg_bound__", False),
       "module": f.__module__}
dwg_bind.uninstall()
out["after_uninstall"] = bool(getattr(tr.Trainer.calc_sigma_loss, "__dwg_bound__", False))
print(json.dumps(out))
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core")), reason="reference tree not present")
def test_b8_binding_of_the_reference_trainer():
    code = _BIND_CODE % (ROOT, DROPIN, REFERENCE)
    env = dict(os.environ)
    env.pop("DWG_BIND_SIGMA", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["patched"] and out["orig_is_reference"], out
    assert out["sig"] == out["orig_sig"] and "selected_parts" in out["sig"] and "wo_wrist" in out["sig"], out
    assert not out["after_uninstall"]
    env["DWG_BIND_SIGMA"] = "0"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert not out["patched"] and out["orig_sig"] is None and out["module"] == "core.trainer", out
