"""CPU checks of the depth-map boundary (B9, include/dwg_depthmap.h, dreamwaltz_g_amd.condition / .pretrain): the binding table,
argument errors reported before any launch, the Python layer's refusals, a self-check of the float64 helper against the golden
keypoint rays, and the binding of the reference's Trainer.pretrain_forward (in a subprocess; skipped when the reference tree is absent)."""
import ctypes
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from oracle import condition as oc
from tests import depthmap_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
REFERENCE = "/root/reference"

FAKE = ctypes.c_void_p(4096)          # 16-byte aligned, never dereferenced: every call below must fail before a launch
ODD = ctypes.c_void_p(4100)
E_ARG = -1


def test_the_binding_table_holds_every_symbol_of_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dwg_depthmap.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dwg_[a-z0-9_]+)\s*\(", src))
    assert names == {"dwg_depthmap_workspace_bytes", "dwg_depthmap_cast", "dwg_depthmap_image", "dwg_pretrain_loss_workspace_bytes",
                     "dwg_pretrain_loss_forward", "dwg_pretrain_loss_backward"}
    assert names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n
    assert "parity unpinned" in open(os.path.join(ROOT, "include", "dwg_depthmap.h")).read().lower()


def test_workspace_is_a_fixed_function_of_the_sizes():
    L = _lib.lib()
    f = L.dwg_depthmap_workspace_bytes
    assert f(0, 512, 100) == 0 and f(512, -1, 100) == 0 and f(512, 512, -1) == 0
    assert f(512, 512, 0) >= 8 and f(512, 512, 0) % 16 == 0
    assert f(512, 512, 20908) == f(64, 64, 20908) >= 20908 * 8                      # nothing per pixel, nothing per (tile, triangle)
    assert f(512, 512, 20908) <= 4 << 20 and f(512, 512, 20909) > f(512, 512, 20908)
    g = L.dwg_pretrain_loss_workspace_bytes
    assert g(0) == 0 and g(-5) == 0 and 0 < g(1) <= g(512 * 512) <= g(1 << 30) <= 1 << 16


def test_bad_arguments_return_arg_error_before_any_launch():
    L = _lib.lib()
    need = L.dwg_depthmap_workspace_bytes(64, 64, 100)
    base = [64, 64, FAKE, FAKE, 50, FAKE, 100, FAKE, FAKE, None, 0, FAKE, need, None]
    for k, bad in ((0, 0), (0, -1), (1, 0), (1, -7), (0, 16385), (1, 16385), (4, -1), (6, -1), (4, 0),
                   (2, None), (3, None), (5, None), (7, None), (8, None),
                   (11, None), (11, ODD), (12, need - 1), (12, 0)):
        args = list(base)
        args[k] = bad
        assert L.dwg_depthmap_cast(*args) == E_ARG, (k, bad)
    img = [64, 64, FAKE, 0, FAKE, None, FAKE, 64, None]
    for k, bad in ((0, 0), (1, -1), (0, 16385), (2, None), (4, None), (6, None), (6, ODD), (7, 8)):
        args = list(img)
        args[k] = bad
        assert L.dwg_depthmap_image(*args) == E_ARG, (k, bad)
    n = 25 * 44
    need = L.dwg_pretrain_loss_workspace_bytes(n)
    fwd = [0, n, FAKE, FAKE, FAKE, FAKE, FAKE, need, None]
    for k, bad in ((0, 1), (0, 7), (1, 0), (1, -3), (2, None), (3, None), (4, None), (5, None), (6, None), (6, ODD), (7, need - 1)):
        args = list(fwd)
        args[k] = bad
        assert L.dwg_pretrain_loss_forward(*args) == E_ARG, (k, bad)
    bwd = [2, n, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]
    for k, bad in ((0, 3), (1, 0), (2, None), (3, None), (4, None), (5, None)):
        args = list(bwd)
        args[k] = bad
        assert L.dwg_pretrain_loss_backward(*args) == E_ARG, (k, bad)
    args = list(bwd)
    args[6] = args[7] = None                                      # no gradient asked for
    assert L.dwg_pretrain_loss_backward(*args) == E_ARG


def _cond():
    from dreamwaltz_g_amd import condition as cd, configs
    return cd, cd.SMPL2Condition(configs.PromptConfig())


def test_cpu_tensors_and_unsupported_options_raise():
    from dreamwaltz_g_amd import pretrain
    cd, cond = _cond()
    v, t = dr.golden_mesh()
    E, K = dr.camera("front", 64, 64)
    cam = dict(extrinsic=torch.from_numpy(E), intrinsics=torch.from_numpy(K), width=64, height=64)
    with pytest.raises(RuntimeError):
        cd.build_ray_casting_scene(torch.from_numpy(v), t)
    with pytest.raises(RuntimeError):
        cond.export_depth(None, raw=True, **cam)
    with pytest.raises(RuntimeError):
        cond.export_normal_raw(object(), **cam)
    with pytest.raises(RuntimeError):
        cond.depth_image(torch.zeros(8, 8))
    with pytest.raises(RuntimeError):
        cond(types.SimpleNamespace(vertices=torch.from_numpy(v)[None], joints=None), t,
             dict(extrinsic=torch.from_numpy(E)[None], intrinsics=torch.from_numpy(K)[None]), "depth_raw", 64, 64)
    with pytest.raises(NotImplementedError):
        cd.build_ray_casting_scene(torch.zeros(2, 5, 3), t)       # [N > 1, V, 3]: one person per condition image, before any device use
    # flag combinations whose result is platform-defined in the reference: refused before the scene is looked at
    for kw in (dict(inverse=False), dict(normalize=False), dict(inverse=False, normalize=False)):
        with pytest.raises(NotImplementedError):
            cond.export_depth(None, **kw, **cam)
        with pytest.raises(NotImplementedError):
            cond.export_depth_chw(None, **kw, **cam)
    with pytest.raises(NotImplementedError):
        cond.export_normal_raw(None, raw=False, **cam)
    for kind in ("depth", "normal", "mesh"):                      # before any argument is touched
        with pytest.raises(NotImplementedError):
            cond(None, None, None, kind, 64, 64)
    z = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError):
        pretrain.depth_mask_loss(z, z, z)
    tr = types.SimpleNamespace(time_to_snapshot=False, render=lambda data: {"image": z, "depth": z.permute(0, 2, 3, 1), "weights_sum": z.permute(0, 2, 3, 1)})
    with pytest.raises(RuntimeError):
        pretrain.pretrain_forward(tr, {"cond_images": [np.zeros((4, 4), dtype=np.float32)]})


def test_depth_map_converts_like_the_reference_array():
    from dreamwaltz_g_amd import condition as cd
    a = np.array([[1.5, np.inf], [np.inf, 2.0]], dtype=np.float32)
    m = cd.DepthMap(torch.from_numpy(a))
    assert m.shape == (2, 2) and np.array_equal(np.asarray(m), a) and np.asarray(m, dtype=np.float64).dtype == np.float64
    assert np.array_equal(np.nan_to_num(m, posinf=0.0, neginf=0.0), np.array([[1.5, 0], [0, 2.0]], dtype=np.float32))


@pytest.mark.parametrize("name", ["front", "side", "wide"])
def test_helper_rays_reproduce_the_golden_keypoint_rays(name):
    """Self-check of tests/depthmap_ref.py: its pinhole rays, aimed at the keypoints' own (fractional) pixel positions, are the golden
    keypoint rays up to their length -- so t along them, times that length, is the golden t_hit.  Both sides round their own ray to
    float32 once, and one such rounding moves the depth on this mesh by s <= 9e-7 (depthmap_ref.sensitivity): bar 2 s + margin = 3e-6."""
    E = np.asarray(dr.G["cond.%s.extrinsic" % name], dtype=np.float32)
    K = np.asarray(dr.G["cond.%s.intrinsics" % name], dtype=np.float32)
    kp = np.asarray(dr.G["cond.keypoints"], dtype=np.float32).astype(np.float64).reshape(-1, 3)
    cam = kp @ E[:3, :3].astype(np.float64).T + E[:3, 3].astype(np.float64)
    front = cam[:, 2] > 0
    x = float(K[0, 0]) * cam[front, 0] / cam[front, 2] + float(K[0, 2]) - 0.5
    y = float(K[1, 1]) * cam[front, 1] / cam[front, 2] + float(K[1, 2]) - 0.5
    o, d = dr.pixel_rays(E, K, x, y)
    v, t = dr.golden_mesh()
    got = oc.ray_cast(o, d, v, t) * np.linalg.norm(d.astype(np.float64), axis=1)
    want = np.asarray(dr.G["cond.%s.t_hit" % name], dtype=np.float64)[front]
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.isfinite(want).sum() > 40
    ok = np.isfinite(want)
    assert (np.abs(got[ok] - want[ok]) / want[ok]).max() <= 3e-6


def test_helper_image_statements_are_float32_and_truncate():
    t = np.array([[1.0, 2.0, 4.0], [np.inf, 8.0, 1.0]], dtype=np.float32)
    img = dr.depth_image(t)
    assert img.dtype == np.uint8 and img.shape == (2, 3, 3) and (img[..., 0] == img[..., 1]).all()
    assert img[..., 0].tolist() == [[255, 127, 63], [0, 31, 255]]           # 255 / t: 255, 127.5, 63.75 | 0, 31.875, 255
    assert dr.depth_image(np.full((2, 2), np.inf, dtype=np.float32)).max() == 0


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
f = tr.Trainer.pretrain_forward
orig = getattr(f, "__wrapped__", None)
out = {"patched": bool(getattr(f, "__dwg_bound__", False)),
       "sig": str(inspect.signature(f)),
       "orig_sig": str(inspect.signature(orig)) if orig is not None else None,
       "orig_is_reference": orig is not None and orig.__module__ == "core.trainer" and not getattr(orig, "__dwg_bound__", False),
       "module": f.__module__,
       "sigma_patched": bool(getattr(tr.Trainer.calc_sigma_loss, "__dwg_bound__", False))}
dwg_bind.uninstall()
out["after_uninstall"] = bool(getattr(tr.Trainer.pretrain_forward, "__dwg_bound__", False))
out["restored"] = tr.Trainer.pretrain_forward is orig
print(json.dumps(out))
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core")), reason="reference tree not present")
def test_b9_binding_of_the_reference_trainer():
    code = _BIND_CODE % (ROOT, DROPIN, REFERENCE)
    env = dict(os.environ)
    env.pop("DWG_BIND_PRETRAIN", None)
    env.pop("DWG_BIND_SIGMA", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["patched"] and out["orig_is_reference"] and out["sigma_patched"], out
    assert out["sig"] == out["orig_sig"] == "(self, data)", out
    assert not out["after_uninstall"] and out["restored"]
    env["DWG_BIND_PRETRAIN"] = "0"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert not out["patched"] and out["orig_sig"] is None and out["module"] == "core.trainer" and out["sigma_patched"], out


def test_bound_pretrain_forward_hands_cpu_renders_to_the_original():
    """The wrapper renders once and decides on the render: a CPU render goes to the method it wraps, with that render."""
    sys.path.insert(0, DROPIN)
    try:
        import dwg_bind
    finally:
        sys.path.remove(DROPIN)
    calls = []

    class Trainer:
        def pretrain_forward(self, data):
            calls.append(self.render(data=data))
            return "reference"

        def render(self, data):
            self.renders = getattr(self, "renders", 0) + 1
            return {"depth": torch.zeros(1, 4, 4, 1)}

    mod = types.SimpleNamespace(Trainer=Trainer)
    orig = Trainer.pretrain_forward
    old = os.environ.pop("DWG_BIND_PRETRAIN", None)
    try:
        dwg_bind._patch_trainer_pretrain(mod)
    finally:
        if old is not None:
            os.environ["DWG_BIND_PRETRAIN"] = old
    assert getattr(Trainer.pretrain_forward, "__dwg_bound__", False) and Trainer.pretrain_forward.__wrapped__ is orig
    t = Trainer()
    assert t.pretrain_forward({}) == "reference" and t.renders == 1 and len(calls) == 1
    dwg_bind._patch_trainer_pretrain(mod)                         # idempotent
    assert Trainer.pretrain_forward.__wrapped__ is orig
