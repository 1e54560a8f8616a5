"""Cases and float64 restatement for the tests of the stage-II learned MLP background (boundary B23, dreamwaltz_g_amd.background).
Imports nothing of the reference.

  SIZES                        (H, W): one partial 64-ray tile, whole tiles, tiles plus a remainder
  GOLDEN                       the ((H, W), F) runs recorded in tests/golden/mlp_background.npz (capture_golden_mlp_background.py)
  camera(f, H, W)              camera f: c2w [4, 4] (a rotation that mixes all axes, a translation) and intrinsics [3, 3] with the principal
                               point OFF the centre
  weights(seed)                the network's four tensors [w0 (16, 27), b0 (16), w1 (3, 16), b1 (3)] fp32
  cotangent / foreground       seeded d_image, and (image_fg, alpha) with alpha exactly 0, exactly 1 and in between
  dirs(c2w, K, H, W, dtype)    get_rays' direction (pixel centre + 0.5, safe_normalize, rotation) then d / ||d||
  image(dirs, wb, dtype)       degree-4 encoding [x, sin x, cos x, sin 2x, cos 2x, ...] -> Linear / ReLU -> Linear -> sigmoid
  composite(fg, alpha, bg)     fg + bg (1 - alpha)
"""
import numpy as np
import torch

from tests import nerf_background_cases as bc

f32 = np.float32
SIZES = [(5, 7), (16, 16), (33, 21)]
GOLDEN = [((5, 7), 3), ((16, 16), 1)]
DEGREE, HIDDEN = 4, 16
SHAPES = [(16, 27), (16,), (3, 16), (3,)]


def camera(f, H, W):
    r = np.random.RandomState(100 + f)
    q, _ = np.linalg.qr(r.randn(3, 3))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    c2w = np.eye(4)
    c2w[:3, :3] = q
    c2w[:3, 3] = r.randn(3)
    fx, fy = 1.1 * W + 0.3 * f, 0.9 * W + 0.2 * f
    K = np.array([[fx, 0.0, 0.5 * W + 1.25 + f], [0.0, fy, 0.5 * H - 0.75 - 0.5 * f], [0.0, 0.0, 1.0]])
    return c2w.astype(f32), K.astype(f32)


def cameras(F, H, W):
    cs = [camera(f, H, W) for f in range(F)]
    return np.stack([c for c, _ in cs]), np.stack([k for _, k in cs])


def weights(seed=7):
    r = np.random.RandomState(seed)
    out = []
    for s in SHAPES:
        bound = 1.0 / (27 if s[-1] == 27 or s == (16,) else 16) ** 0.5
        out.append(((r.rand(*s) * 2 - 1) * bound * 3).astype(f32))        # 3 x nn.Linear's scale: the sigmoid leaves its linear range
    return out


def cotangent(F, H, W, seed=11):
    return np.random.RandomState(seed + H * W + F).randn(F, H, W, 3).astype(f32)


def foreground(F, H, W, seed=13):
    """image_fg [F, H, W, 3] and alpha [F, H, W, 1]: a third of the pixels at alpha exactly 0, a third exactly 1, the rest in between."""
    r = np.random.RandomState(seed + H * W + F)
    fg = r.rand(F, H, W, 3).astype(f32)
    alpha = r.rand(F, H, W, 1).astype(f32)
    kind = r.randint(0, 3, size=(F, H, W, 1))
    alpha[kind == 0] = 0.0
    alpha[kind == 1] = 1.0
    return fg, alpha


def dirs(c2w, K, H, W, dtype=torch.float64):
    """c2w [F, 4, 4], K [F, 3, 3] tensors -> [F * H * W, 3]."""
    c2w, K = c2w.to(dtype), K.to(dtype)
    j, i = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing='ij')
    i, j = i.reshape(1, -1) + 0.5, j.reshape(1, -1) + 0.5
    xs = (i - K[:, 0, 2:3]) / K[:, 0, 0:1]
    ys = (j - K[:, 1, 2:3]) / K[:, 1, 1:2]
    d = torch.stack([xs, ys, torch.ones_like(xs)], -1)
    d = d / torch.sqrt(torch.clamp((d * d).sum(-1, keepdim=True), min=1e-20))
    d = d @ c2w[:, :3, :3].transpose(-1, -2)
    d = d / torch.norm(d, dim=-1, keepdim=True)
    return d.reshape(-1, 3)


def image(d, wb, dtype=torch.float64):
    """d [N, 3], wb = [w0, b0, w1, b1] tensors -> [N, 3]."""
    h = bc.encode(d, DEGREE, dtype)
    h = torch.relu(torch.nn.functional.linear(h, wb[0].to(dtype), wb[1].to(dtype)))
    return torch.sigmoid(torch.nn.functional.linear(h, wb[2].to(dtype), wb[3].to(dtype)))


def composite(fg, alpha, bg):
    return fg + bg * (1 - alpha)


def oracle(c2w, K, H, W, wb, d_image, fg=None, alpha=None):
    """float64: -> dict(dirs, image, grads [4]) for the cotangent d_image [F, H, W, 3] on the image; with fg / alpha also composite and
    d_alpha / d_bg of the composite under the same cotangent."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    F = c2w.shape[0]
    params = [t(w).double().requires_grad_(True) for w in wb]
    d = dirs(t(c2w), t(K), H, W)
    img = image(d, params).view(F, H, W, 3)
    img.backward(t(d_image).double())
    out = {"dirs": d, "image": img.detach(), "grads": [p.grad for p in params]}
    if fg is not None:
        a, b = t(alpha).double().requires_grad_(True), img.detach().clone().requires_grad_(True)
        comp = composite(t(fg).double(), a, b)
        comp.backward(t(d_image).double())
        out.update(composite=comp.detach(), d_alpha=a.grad, d_bg=b.grad)
    return out
