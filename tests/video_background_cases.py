"""Restatement of the reference's video background (core/system/background.py:140-155, core/system/scene.py:157-160) in numpy / torch
on the host, for tests/test_video_background_*.py.

OpenCV is not installed here, so cv2.resize(frame, (W, H)) with its default INTER_LINEAR is restated for 8-bit images as OpenCV's
resize.cpp computes it (the rule include/dwg_background.h documents):
  scale = 1 / (dst / src) in double
  exact 2x downscale in both directions: the fast area path, (s00 + s01 + s10 + s11 + 2) >> 2
  otherwise: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; columns clamp s and zero f at the edges, rows clamp the two
  source rows only; 11-bit coefficients rint((1 - f) * 2048), rint(f * 2048); a horizontal pass into integers, then
  ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.
Against cv2 itself this is UNVERIFIED: the documented claim is +-1 on the uint8 value (SIMD / IPP builds may round differently)."""
import numpy as np
import torch

COEF_SCALE = 2048


def make_frames(T, h, w, seed=0):
    """T random BGR uint8 frames [T, h, w, 3], as cv2 decodes them."""
    return np.random.RandomState(seed).randint(0, 256, size=(T, h, w, 3)).astype(np.uint8)


def _axis(dst, src, clamp_coef):
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_coef:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= src - 1
        f[hi], s[hi] = 0, src - 1
    c0 = np.rint((np.float32(1) - f) * np.float32(COEF_SCALE)).astype(np.int64)
    c1 = np.rint(f * np.float32(COEF_SCALE)).astype(np.int64)
    return s, c0, c1


def is_area2x(h, w, H, W):
    sx, sy = 1.0 / (float(W) / w), 1.0 / (float(H) / h)
    ix, iy = int(round(sx)), int(round(sy))
    eps = np.finfo(np.float64).eps
    return abs(sx - ix) < eps and abs(sy - iy) < eps and ix == 2 and iy == 2


def resize_u8(src, W, H):
    """cv2.resize(src, (W, H)) for a uint8 [h, w, C] image, restated (see the module docstring)."""
    h, w = src.shape[:2]
    if (h, w) == (H, W):
        return src.copy()
    s = src.astype(np.int64)
    if is_area2x(h, w, H, W):
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = _axis(W, w, True)
    sy, b0, b1 = _axis(H, h, False)
    x1 = np.minimum(sx + 1, w - 1)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)

    def hpass(rows):
        r = s[rows]                                                   # [H, w, C]
        return r[:, sx] * a0[None, :, None] + r[:, x1] * a1[None, :, None]
    S0, S1 = hpass(y0), hpass(y1)
    out = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def reference_background_u8(frame_bgr, H, W):
    """cvtColor(BGR2RGB), then the resize when the sizes differ: the uint8 RGB frame the reference divides."""
    rgb = np.ascontiguousarray(frame_bgr[..., ::-1])
    if rgb.shape[0] != H or rgb.shape[1] != W:
        rgb = resize_u8(rgb, W, H)
    return rgb


def reference_background(frame_bgr, H, W):
    """get_background_like: torch.from_numpy(frame).float() / 255.0 on the host (a true division) -> CPU float32 [H, W, 3]."""
    return torch.from_numpy(reference_background_u8(frame_bgr, H, W)).float() / 255.0


def reference_composite(image, alpha, bg):
    """scene.py:158-160 as torch computes it on the device: image + image_bg * (1 - alpha)."""
    return image + bg.to(image) * (1 - alpha)
