"""CPU checks of the image-loss boundary (B17, include/dwg_image_loss.h, dreamwaltz_g_amd.image_loss): the Python layer's refusals (raised
before the library is touched), the exported symbols and their argument checks (before any launch), the oracle's self-check, its
agreement with a second float64 form, and the binding of the reference's Trainer.init_losses / pretrain_nerf2gs_forward (in a
subprocess; skipped when the reference tree is absent)."""
import ctypes
import json
import os
import re
import subprocess
import sys
import types

import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from tests import image_loss_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
FAKE = ctypes.c_void_p(4096)          # aligned, never dereferenced: every call below must fail before a launch
ODD = ctypes.c_void_p(4098)
E_ARG = -1


@pytest.fixture
def no_library(monkeypatch):
    def touched():
        raise AssertionError("the library was touched before the refusal")
    monkeypatch.setattr(_lib, "lib", touched)


def test_refusals_are_raised_before_the_library_is_touched(no_library):
    from dreamwaltz_g_amd import image_loss as il
    x, y = torch.rand(1, 3, 12, 12), torch.rand(1, 3, 12, 12)
    loss = il.ImageReconstructionLoss()
    for f in (loss, il.l1_loss, il.ssim):
        with pytest.raises(RuntimeError, match="GPU only"):
            f(x, y)                                                   # CPU tensors
        with pytest.raises(TypeError):
            f(x.double(), y.double())
        with pytest.raises(TypeError):
            f(x, y.half())
        with pytest.raises(ValueError):
            f(x, y[..., :-1])                                         # mismatched shapes
        with pytest.raises(ValueError):
            f(x[:, :, :0], y[:, :, :0])                               # an empty image
        with pytest.raises(ValueError):
            f(x[0, 0], y[0, 0])                                       # not an image
        with pytest.raises(RuntimeError, match="target"):
            f(x, y.clone().requires_grad_(True))
    for ws in (7, 9, 13, 0):
        with pytest.raises(ValueError, match="window_size"):
            il.ssim(x, y, window_size=ws)
    with pytest.raises(ValueError):
        il.ImageReconstructionLoss(lambda_dssim=1.5)
    assert il.ImageReconstructionLoss().lambda_dssim == 0.2
    tr = types.SimpleNamespace(render=lambda data: {"image_fg": x.permute(0, 2, 3, 1)}, nerf_guidance=None, losses={})
    with pytest.raises(RuntimeError, match="GPU only"):
        il.nerf2gs_forward(tr, {})                                    # a CPU render, before the teacher is asked for anything


def test_the_library_exports_the_headers_three_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dwg_image_loss.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dwg_[a-z0-9_]+)\s*\(", src))
    assert names == {"dwg_image_loss_workspace_bytes", "dwg_image_loss_forward", "dwg_image_loss_backward"}
    assert names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n


def test_workspace_is_two_doubles_per_tile_and_plane():
    f = _lib.lib().dwg_image_loss_workspace_bytes
    assert f(1, 3, 16, 16) == 3 * 16 and f(1, 3, 17, 33) == 3 * 2 * 3 * 16 and f(2, 3, 37, 53) == 6 * 3 * 4 * 16
    assert f(1, 3, 1024, 1024) == 3 * 64 * 64 * 16
    assert f(0, 3, 16, 16) == 0 and f(1, 0, 16, 16) == 0 and f(1, 3, -1, 16) == 0 and f(1, 3, 16, 32769) == 0 and f(256, 256, 16, 16) == 0


def test_bad_arguments_return_arg_error_before_any_launch():
    L = _lib.lib()
    B, C, H, W = 2, 3, 20, 24
    need = L.dwg_image_loss_workspace_bytes(B, C, H, W)
    nchw = [C * H * W, H * W, W, 1]
    fwd = [B, C, H, W, 11, 0.2, FAKE] + nchw + [FAKE] + nchw + [FAKE, None, None, FAKE, need, None]
    bad_fwd = [(0, 0), (1, -1), (2, 0), (3, 32769), (0, 65536), (4, 7), (4, 12), (5, -0.1), (5, 1.5), (5, float("nan")),
               (6, None), (6, ODD), (7, 0), (8, -1), (9, 0), (10, 0), (10, 1 << 41), (11, None), (11, ODD), (12, -1), (15, -4),
               (16, None), (16, ODD), (17, ODD), (18, ODD), (19, None), (19, ctypes.c_void_p(4100)), (20, need - 1), (20, 0)]
    for k, bad in bad_fwd:
        args = list(fwd)
        args[k] = bad
        assert L.dwg_image_loss_forward(*args) == E_ARG, (k, bad)
    bwd = [B, C, H, W, 11, -0.2 / 100, 0.8 / 100, FAKE] + nchw + [FAKE] + nchw + [FAKE, FAKE, 0, FAKE, None]
    bad_bwd = [(0, 0), (2, -3), (3, 0), (4, 9), (5, float("nan")), (6, float("nan")), (7, None), (7, ODD), (8, 0), (11, 0), (12, None),
               (13, -1), (17, None), (17, ODD), (18, None), (18, ODD), (20, None), (20, ODD)]
    for k, bad in bad_bwd:
        args = list(bwd)
        args[k] = bad
        assert L.dwg_image_loss_backward(*args) == E_ARG, (k, bad)
    # a stride is read only along a dimension longer than 1, and the target may repeat itself (stride 0) where x may not
    one = [1, C, H, W, 11, 0.2, FAKE, 0] + nchw[1:] + [FAKE, 0, 0, W, 1] + [None, None, None, FAKE, need, None]
    assert L.dwg_image_loss_forward(*one) == E_ARG                   # only `scalars` is wrong here
    args = list(bwd)
    args[5], args[17] = 0.0, None                                    # the L1 term alone needs no maps ...
    args[18] = None                                                  # ... and this call fails on the missing upstream gradient only
    assert L.dwg_image_loss_backward(*args) == E_ARG


def test_the_oracle_checks_itself():
    out = ic.self_check()
    assert out["ssim_batch"].shape == (1,) and out["ssim_batch"][0] == 1.0


@pytest.mark.parametrize("name", ["smaller_than_window", "batch_ragged"])
def test_the_oracle_agrees_with_a_second_float64_form(name):
    c = ic.case(name)
    loss, l1, ssim = ic.numpy_form(c["x"], c["y"])
    assert abs(loss - c["want"]["loss"]) <= 1e-12 and abs(l1 - c["want"]["l1"]) <= 1e-12 and abs(ssim - c["want"]["ssim"]) <= 1e-12


def test_cases_reach_what_they_are_for():
    T = ic.TILE
    assert T == 16                                                    # the table of shapes is the one for 16 x 16 tiles
    c = ic.case("blob_shifted")
    same = (c["x"] == c["y"])
    assert 0.5 < float(same.float().mean()) < 0.95 and bool(((c["x"] != 0) & same).any())       # equal on the background AND inside the blob
    assert int((c["want"]["grad"] == 0).sum()) > 100 and int((c["want"]["grad"] != 0).sum()) > 100
    assert ic.case("near_zero_loss")["want"]["loss"] < 2e-3
    for name, (shape, layouts, _) in ic.CASES.items():
        e = ic.case(name)["e_ref"]
        assert all(v < 1e-4 for v in e.values()), (name, e)         # the fp32 composition is a sane yardstick


def _bind_check(env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "image_loss_bind_check.py")], capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DWG_IMAGE_LOSS_BIND_CHECK ")][-1]
    out = json.loads(line[len("DWG_IMAGE_LOSS_BIND_CHECK "):])
    if "missing" in out:
        pytest.skip("the reference's trainer module needs the package %r, which is not installed" % out["missing"])
    return out


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core")), reason="reference tree not present")
def test_b17_binding_of_the_reference_trainer():
    env = dict(os.environ)
    for k in ("DWG_BIND_NERF2GS", "DWG_BIND_PRETRAIN", "DWG_BIND_SIGMA"):
        env.pop(k, None)
    out = _bind_check(env)
    for attr, sig in (("init_losses", "(self) -> Dict[str, Callable]"), ("pretrain_nerf2gs_forward", "(self, data)")):
        assert out[attr]["patched"] and out[attr]["orig_is_reference"], out
        assert out[attr]["sig"] == out[attr]["orig_sig"] == sig, out
    assert out["original_raises"] == "pytorch3d.ops", out                                   # the absence the hook is for
    for k in ("with_pytorch3d", "without_pytorch3d"):
        assert out[k]["native"] and out[k]["keys"] == ["image", "mse", "sparsity"] and out[k]["flag_after"] is True, out
    assert out["without_pytorch3d"]["lambda_dssim"] == 0.2
    assert out["flag_off_keys"] == ["mse", "sparsity"]
    assert out["other_exception"] == "AttributeError" and out["flag_after_other_exception"] is True, out
    assert out["restored"] == {"init_losses": True, "pretrain_nerf2gs_forward": True} and out["pretrain_patched"]
    env["DWG_BIND_NERF2GS"] = "0"
    out = _bind_check(env)
    for attr in ("init_losses", "pretrain_nerf2gs_forward"):
        assert not out[attr]["patched"] and out[attr]["orig_sig"] is None, out
    assert out["pretrain_patched"], out


def test_bound_nerf2gs_forward_hands_cpu_renders_to_the_original():
    """The wrapper renders once and decides on the render: a CPU render goes to the method it wraps, with that render."""
    dropin = os.path.join(ROOT, "dropin")
    sys.path.insert(0, dropin)
    try:
        import dwg_bind
    finally:
        sys.path.remove(dropin)

    class Trainer:
        def init_losses(self):
            return {}

        def pretrain_nerf2gs_forward(self, data):
            return "reference", self.render(data=data)

        def render(self, data):
            self.renders = getattr(self, "renders", 0) + 1
            return {"image_fg": torch.zeros(1, 4, 4, 3)}

    mod = types.SimpleNamespace(Trainer=Trainer)
    orig = Trainer.pretrain_nerf2gs_forward
    old = os.environ.pop("DWG_BIND_NERF2GS", None)
    try:
        dwg_bind._patch_trainer_nerf2gs(mod)
        dwg_bind._patch_trainer_nerf2gs(mod)                          # idempotent
    finally:
        if old is not None:
            os.environ["DWG_BIND_NERF2GS"] = old
    assert getattr(Trainer.pretrain_nerf2gs_forward, "__dwg_bound__", False) and Trainer.pretrain_nerf2gs_forward.__wrapped__ is orig
    t = Trainer()
    assert t.pretrain_nerf2gs_forward({})[0] == "reference" and t.renders == 1
