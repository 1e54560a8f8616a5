"""Video background (boundary B5, dreamwaltz_g_amd.background), host side: Scene's acceptance of a VideoBackground, the bound build_scene
with `--render.use_video_background` on the real reference module, the C-ABI's argument checks, host index rules, and self-checks of
the resampling restatement (tests/video_background_cases.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import dwg_import  # noqa: F401
from tests import video_background_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    from dreamwaltz_g_amd import configs
    cfg = configs.TrainConfig()
    cfg.device = "cpu"
    return cfg


def test_scene_accepts_a_video_background_and_rejects_the_other_kinds():
    from dreamwaltz_g_amd import scene as sc
    from dreamwaltz_g_amd.background import VideoBackground
    bg = VideoBackground.from_frames(vc.make_frames(3, 8, 10), fps=24)
    s = sc.Scene(_cfg(), [nn.Module()], background=bg)
    assert s.background is bg
    assert sc.Scene(_cfg(), [nn.Module()]).background is None

    class MLPBackground(nn.Module):
        pass

    class GaussianModel(nn.Module):
        pass
    for other in (MLPBackground(), GaussianModel()):
        with pytest.raises(NotImplementedError):
            sc.Scene(_cfg(), [nn.Module()], background=other)


def test_config_default_is_the_references():
    from dreamwaltz_g_amd import configs
    assert configs.RenderConfig().use_video_background is None


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference checkout (build container only)")
def test_bound_build_scene_adopts_the_references_video_background():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "video_background_bind_check.py")], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DWG_VIDEO_BIND_CHECK ")][-1]
    d = json.loads(line[len("DWG_VIDEO_BIND_CHECK "):])
    assert d["scene_class"] == "dreamwaltz_g_amd.scene.Scene"
    assert d["background_class"] == "dreamwaltz_g_amd.background.VideoBackground"
    assert d["reference_constructed_with"] == ["motionx_reenact,clip"] and d["reference_kept"]
    assert d["attributes"] == [25, 5, 20, 12] and d["frames_equal"]
    assert d["alive_while_scene_lives"] and d["released_with_scene"]
    assert d["other_backgrounds_raise"] == {"use_mlp_background": True, "use_gs_background": True}


def test_from_frames_and_from_reference_surface():
    from dreamwaltz_g_amd.background import VideoBackground
    fr = vc.make_frames(4, 6, 9, seed=2)
    a = VideoBackground.from_frames(fr, fps=30)
    assert (a.fps, a.frame_count, a.frame_width, a.frame_height) == (30, 4, 9, 6)
    b = VideoBackground.from_frames(torch.from_numpy(fr), fps=12)
    assert torch.equal(b._host, a._host)

    class Ref:                                      # a reference object built with preload=False: frames come from get_background
        fps, frame_count, frame_cache = 25, 4, None

        def get_background(self, i):
            return fr[i]
    c = VideoBackground.from_reference(Ref())
    assert c.fps == 25 and np.array_equal(c._host.numpy(), fr) and isinstance(c.reference, Ref)
    with pytest.raises(ValueError):
        VideoBackground.from_frames(fr.astype(np.float32))
    with pytest.raises(ValueError):
        VideoBackground.from_frames(fr[..., :2])


def test_path_constructor_needs_cv2_or_reports_the_missing_file():
    from dreamwaltz_g_amd.background import VideoBackground
    try:
        import cv2  # noqa: F401
        expected = FileNotFoundError
    except ImportError:
        expected = ImportError
    with pytest.raises(expected):
        VideoBackground(os.path.join(ROOT, "no_such_video.mp4"))


def test_host_frame_indices_behave_like_the_references_list():
    from dreamwaltz_g_amd.background import VideoBackground
    bg = VideoBackground.from_frames(vc.make_frames(5, 2, 2))
    lst = list(range(5))
    for i in (0, 4, -1, -5, np.int64(3)):
        assert bg.wrap(i) == lst[i]
    for i in (5, -6, 100):
        with pytest.raises(IndexError):
            lst[i]
        with pytest.raises(IndexError):
            bg.wrap(i)


def test_cabi_argument_errors_return_nonzero_before_any_launch():
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    fwd, bwd = L.dwg_video_composite_forward, L.dwg_video_composite_backward
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)           # never dereferenced: every call below fails its host checks

    def f(F=1, H=4, W=4, fg=p, alpha=p, sf=48, sp=3, sc=1, frames=p, T=2, h=4, w=4, idx=p, image=p, image_bg=p):
        return fwd(F, H, W, fg, alpha, sf, sp, sc, frames, T, h, w, idx, image, image_bg, None)

    def b(F=1, H=4, W=4, d=p, sf=48, sp=3, sc=1, frames=p, T=2, h=4, w=4, idx=p, d_alpha=p):
        return bwd(F, H, W, d, sf, sp, sc, frames, T, h, w, idx, d_alpha, None)
    for k in ("F", "H", "W", "T", "h", "w"):
        for v in (0, -1):
            assert f(**{k: v}) != 0 and b(**{k: v}) != 0, (k, v)
    for k in ("frames", "idx"):
        assert f(**{k: None}) != 0 and b(**{k: None}) != 0, k
    assert f(fg=None) != 0 and f(alpha=None) != 0 and f(image=None) != 0
    assert f(fg=None, alpha=None, image=None, image_bg=None) != 0                  # nothing to write
    assert b(d=None) != 0 and b(d_alpha=None) != 0
    for k in ("fg", "alpha", "image", "image_bg", "idx"):
        assert f(**{k: odd}) != 0, k
    for k in ("d", "d_alpha", "idx"):
        assert b(**{k: odd}) != 0, k
    assert f(sc=-1) != 0 and b(sp=-3) != 0
    assert f(F=70000) != 0                                                           # one grid row per frame


def test_restatement_identity_resize_is_a_copy():
    fr = vc.make_frames(1, 13, 17, seed=4)[0]
    out = vc.resize_u8(fr, 17, 13)
    assert out is not fr and np.array_equal(out, fr)
    # one axis equal: its coefficients are (2048, 0), so a 1-pixel-high stripe of equal rows resamples like a copy along it
    stripe = np.repeat(fr[:1], 5, axis=0)
    assert np.array_equal(vc.resize_u8(stripe, 17, 9), np.repeat(fr[:1], 9, axis=0))
    assert np.array_equal(vc.reference_background_u8(fr, 13, 17), fr[..., ::-1])


@pytest.mark.parametrize("size", [(7, 11), (26, 34), (40, 40), (6, 8), (13, 17)])
def test_restatement_keeps_a_constant_image_constant(size):
    H, W = size
    for v in (0, 1, 77, 128, 254, 255):
        c = np.full((13, 17, 3), v, np.uint8)
        assert (vc.resize_u8(c, W, H) == v).all(), (size, v)
    assert vc.is_area2x(26, 34, 13, 17) and not vc.is_area2x(39, 51, 13, 17) and not vc.is_area2x(26, 34, 13, 16)


def test_restatement_is_within_one_of_float_bilinear():
    """The 11-bit rule against the same half-pixel bilinear in float64 (edge-clamped): at most 1 apart on every value."""
    fr = vc.make_frames(1, 31, 45, seed=6)[0]
    for H, W in ((20, 28), (64, 97), (31, 13)):
        got = vc.resize_u8(fr, W, H).astype(np.float64)
        ys = np.clip((np.arange(H) + 0.5) * 31 / H - 0.5, 0, 30)
        xs = np.clip((np.arange(W) + 0.5) * 45 / W - 0.5, 0, 44)
        y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
        y1, x1 = np.minimum(y0 + 1, 30), np.minimum(x0 + 1, 44)
        fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
        s = fr.astype(np.float64)
        want = (s[y0][:, x0] * (1 - fy) * (1 - fx) + s[y0][:, x1] * (1 - fy) * fx + s[y1][:, x0] * fy * (1 - fx) + s[y1][:, x1] * fy * fx)
        assert np.abs(got - want).max() <= 1.0, (H, W)
