"""The scene cull's visibility test on the host (boundary B25, no GPU): csrc/cull_math.h built by g++ against a float64 and a float32 numpy
restatement of the rasterizer's own keep decision (tests/scene_cull_cases.py) -- the bound never drops what the rasterizer keeps, and it
is not vacuous -- the argument checks of csrc/scene_cull_args.h, the stand-alone self-check program, and the refusals and cache key of the
Python layer that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from tests import gs_background_cases as gc
from tests import scene_cull_cases as cc

N = 40000


@pytest.fixture(scope="module")
def L():
    return cc.hostlib()


@pytest.mark.parametrize("hw", cc.IMAGES, ids=lambda hw: "%dx%d" % (hw[1], hw[0]))
@pytest.mark.parametrize("name", cc.GENERATORS)
def test_nothing_the_rasterizer_keeps_is_dropped(L, name, hw):
    """The contract: a Gaussian that k_preprocess gives radius > 0 -- by its float64 or by its float32 restatement -- is never flagged 0."""
    H, W = hw
    pos, scales, quats, cam = cc.case(name, N, H, W)
    block = cc.camera_block(cam)
    flags = cc.host_flags(L, pos, scales, block, H, W).astype(bool)
    for dtype in (np.float64, np.float32):
        keeps = cc.preprocess_keeps(pos, scales, quats, block, H, W, dtype)
        dropped = keeps & ~flags
        print("%s %dx%d %s: rasterizer keeps %d of %d, cull keeps %d, false drops %d"
              % (name, W, H, dtype.__name__, keeps.sum(), N, flags.sum(), dropped.sum()))
        assert not dropped.any(), "dropped although visible: indices %s" % np.nonzero(dropped)[0][:8]
    if name == "behind":
        assert not flags.any()


def test_the_union_over_cameras_keeps_what_any_camera_keeps(L):
    H, W = 64, 64
    pos, scales, quats, _ = cc.case("box_inside", N, H, W)
    blocks = np.stack([cc.camera_block(cc.box_camera(w, H, W)) for w in ("inside", "corner", "outside")])
    each = [cc.host_flags(L, pos, scales, b, H, W) for b in blocks]
    assert np.array_equal(cc.host_flags(L, pos, scales, blocks, H, W), each[0] | each[1] | each[2])
    assert 0 < each[0].sum() < each[2].sum() <= N


def test_the_bound_is_not_vacuous(L):
    """The playback benchmark's geometry (camera inside the box, 1024^2, tan(fov / 2) of fovy 55): the cull keeps at most 1.15 x what the
    rasterizer's float64 restatement keeps, and far from everything."""
    H = W = 1024
    pos, scales, quats, cam = cc.case("box_inside", 200000, H, W)
    block = cc.camera_block(cam)
    kept = int(cc.host_flags(L, pos, scales, block, H, W).sum())
    visible = int(cc.preprocess_keeps(pos, scales, quats, block, H, W, np.float64).sum())
    print("camera inside the box: the rasterizer keeps %d of %d (%.1f %%), the cull %d (%.3f x)"
          % (visible, pos.shape[0], 100.0 * visible / pos.shape[0], kept, kept / visible))
    assert visible > 0 and kept <= 1.15 * visible
    assert kept < 0.5 * pos.shape[0]


def test_what_is_not_a_number_is_kept(L):
    H, W = 64, 64
    block = cc.camera_block(cc.box_camera("inside", H, W))
    pos = np.array([[np.nan, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    scales = np.array([[0.01] * 3, [np.nan, 0.01, 0.01], [np.inf, 0.01, 0.01]], np.float32)
    assert cc.host_flags(L, pos, scales, block, H, W).tolist() == [1, 1, 1]


def test_argument_checks(L):
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = lambda **kw: L.host_cull_check_flags(*[dict(dict(n=4, pos=p, sc=p, C=1, cams=p, stride=37, H=64, W=64, flags=p), **kw)[k]     # noqa: E731
                                               for k in ("n", "pos", "sc", "C", "cams", "stride", "H", "W", "flags")])
    assert ok() == 1 and ok(n=0, pos=None, sc=None, cams=None, flags=None) == 1
    for bad in (dict(n=-1), dict(n=1 << 31), dict(C=0), dict(C=65), dict(stride=36), dict(H=0), dict(W=0), dict(W=1 << 20), dict(pos=None),
                dict(sc=p + 2), dict(cams=None), dict(flags=None)):
        assert ok(**bad) == 0, bad
    assert L.host_cull_check_compact(4, p, p, p, p) == 1 and L.host_cull_check_compact(0, None, None, p, None) == 1
    for bad in ((-1, p, p, p, p), (4, None, p, p, p), (4, p, p + 1, p, p), (4, p, p, None, p), (4, p, p, p, None), (0, None, None, None, None)):
        assert L.host_cull_check_compact(*bad) == 0, bad
    from dreamwaltz_g_amd.background import CULL_MAX_ROWS, CullRowsC
    rows = (CullRowsC * (CULL_MAX_ROWS + 1))()
    for i, r in enumerate(rows):
        r.src, r.dst, r.width = p, p + 128, 1 + i
    g = lambda kept=2, index=p, total=4, n=2, tables=rows: L.host_cull_check_gather(kept, index, total, n, ctypes.addressof(tables) if tables else None)   # noqa: E731
    assert g() == 1 and g(n=CULL_MAX_ROWS) == 1 and g(kept=0, index=None, tables=None) == 1 and g(n=0, tables=None) == 1
    for bad in (dict(kept=5), dict(kept=-1), dict(total=1 << 31), dict(n=CULL_MAX_ROWS + 1), dict(n=-1), dict(index=None), dict(tables=None)):
        assert g(**bad) == 0, bad
    rows[1].width = 65
    assert g() == 0
    rows[1].width, rows[1].dst = 4, p
    assert g() == 0


def test_the_stand_alone_self_check_program(tmp_path):
    """tests/hostmath/cull_math_host.cpp with its own main: the test over every combination of edge values (zeros, denormal-sized, the
    near plane, huge, infinite, NaN) under three cameras and five image sizes, and the argument checks.  (Built with
    -fsanitize=address,undefined the same program is the sanitizer run of this code.)"""
    _, src, _ = cc._sources()
    exe = str(tmp_path / "cull_selfcheck")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-DCULL_SELFCHECK_MAIN", "-o", exe, src, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 wrong argument checks" in r.stdout


def test_python_layer_without_a_device():
    """cull_key needs no device and no launch: it follows the camera tensors, the scene's parameters and the image size; the switch is
    refused without a Gaussian scene."""
    from dreamwaltz_g_amd import configs, scene as sc
    from dreamwaltz_g_amd.background import GaussianBackground
    bg = GaussianBackground.from_tensors(**gc.scene_arrays(9))
    cam = cc.box_camera("inside", 64, 64)
    k0 = bg.cull_key(cam, 64, 64)
    assert bg.cull_key(cam, 64, 64) == k0 and bg.cull_key([cam], 64, 64) == k0
    assert bg.cull_key(cam, 64, 48) != k0 and bg.cull_key([cam, cc.box_camera("corner", 64, 64)], 64, 64) != k0
    cam['extrinsic'].mul_(1.0)
    k1 = bg.cull_key(cam, 64, 64)
    assert k1 != k0
    with torch.no_grad():
        bg._positions.add_(0.0)
    k2 = bg.cull_key(cam, 64, 64)
    assert k2 != k1
    with torch.no_grad():
        bg._scales.add_(0.0)
    assert bg.cull_key(cam, 64, 64) != k2
    blocks = torch.zeros(2, 37)
    assert bg.cull_key(blocks, 64, 64) == bg.cull_key(blocks, 64, 64) != bg.cull_key(blocks.clone(), 64, 64)
    with pytest.raises(TypeError, match="cameras"):
        bg.cull_key(["not a camera"], 64, 64)
    assert bg.cull_launches == 0

    class Avatar(torch.nn.Module):
        pass
    cfg = configs.TrainConfig(); cfg.device = "cpu"
    with pytest.raises(ValueError, match="cull_scene=True culls a Gaussian scene background"):
        sc.Scene(cfg, [Avatar()], background=None, cull_scene=True)
    scene = sc.Scene(cfg, [Avatar()], background=bg)
    assert scene.cull_scene is False
    with pytest.raises(ValueError, match="cull_scene=True culls a Gaussian scene background"):
        sc.Scene(cfg, [Avatar()]).forward_frames({}, [], cull_scene=True)
    with pytest.raises(ValueError, match="at most 64 per-frame cameras, got 65"):
        scene.forward_frames([cam] * 65, [None] * 65, cull_scene=True)
    with pytest.raises(ValueError, match="tanfov_dev"):
        scene.forward_frames(dict(cam, tanfov_dev=torch.zeros(2)), [None], cull_scene=True)
    assert bg.cull_launches == 0
    cfg.render.use_fixed_n_gaussians = 5
    with pytest.raises(ValueError, match="cull_scene with use_fixed_n_gaussians"):
        sc.Scene(cfg, [Avatar()], background=bg, cull_scene=True).forward_frames(cam, [None])
