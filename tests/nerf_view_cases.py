"""Restatements for the tests of the view around the NeRF render (boundary B20, dreamwaltz_g_amd.nerf_view).  float64 numpy on the
fp32 inputs; imports nothing of the reference.

  camera(H, W)              an off-centre camera: cx != W / 2, fx != fy, a rotation with no zero entry, an origin from which some rays
                            of the image hit the box [-bound, bound]^3 and some miss it
  rays(c2w, K, H, W)        get_rays with N = -1 (core/nerf/nerf_utils.py:72-137): rays_o, rays_d [H W, 3]
  ws_vector()               2145 values of weights_sum: exact 0, exact 1, values below 1e-6 and above 1 - 1e-6, the rest spread over (0, 1)
  LAMBDAS                   the sparsity cases: each lambda alone and all three together
  sparsity_terms / sparsity_loss / sparsity_grad      SparsityLoss (core/nerf/nerf_loss.py:17-56) and its derivative
  mix / mix_grads           image_fg + (1 - ws) * bg and its gradients
"""
import numpy as np

f32 = np.float32
U = 2.0 ** -24                      # half an ulp of 1: the error of one fp32 rounding, relative
RAY_BOUND = 16 * U                  # per component of rays_d (the issue's count of roundings)
SIZES = [(5, 7), (33, 65)]
N_WS = 2145                         # 33 * 65
LAMBDAS = {"opacity": (1e-3, 0.0, 0.0), "entropy": (0.0, 2e-3, 0.0), "emptiness": (0.0, 0.0, 1.0), "all": (5e-3, 1e-3, 0.5)}
MULTIPLIER, SPARSITY_STEP, MAX_ITER = 20, 0.4, 100
STEPS = {"before": 10, "after": 60}          # current_step / MAX_ITER below and above SPARSITY_STEP
EPS = 1e-6
LO, HI = float(f32(1e-6)), float(f32(1 - 1e-6))      # torch clamps the fp32 tensor against the Python doubles rounded to fp32


def camera(H, W, bound=1.0):
    """-> c2w [4, 4], intrinsics [3, 3] fp32."""
    a, b, c = 0.35, -0.5, 0.2
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    c2w = np.eye(4)
    c2w[:3, :3] = R
    c2w[:3, 3] = -R[:, 2] * 3.2 * bound + np.array([0.15, -0.1, 0.05]) * bound      # looks at the box from 3.2 bounds away
    K = np.array([[0.9 * W, 0, 0.5 * W + 1.25], [0, 1.3 * W, 0.5 * H - 0.75], [0, 0, 1]])
    assert (np.abs(R) > 1e-3).all()
    return c2w.astype(f32), K.astype(f32)


def rays(c2w, K, H, W):
    c2w, K = np.asarray(c2w, np.float64), np.asarray(K, np.float64)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    i, j = i.reshape(-1) + 0.5, j.reshape(-1) + 0.5
    d = np.stack([(i - K[0, 2]) / K[0, 0], (j - K[1, 2]) / K[1, 1], np.ones_like(i)], -1)
    d = d / np.sqrt(np.maximum((d * d).sum(-1, keepdims=True), 1e-20))
    rays_d = d @ c2w[:3, :3].T
    return np.broadcast_to(c2w[:3, 3], rays_d.shape).copy(), rays_d


def ws_vector(seed=0):
    r = np.random.RandomState(seed)
    ws = r.rand(N_WS).astype(f32)
    ws[:40] = 0.0
    ws[40:80] = 1.0
    ws[80:120] = (r.rand(40) * 0.9e-6).astype(f32)                              # below the entropy clamp
    ws[120:160] = f32(1.0) - (r.randint(1, 8, 40) * f32(2.0 ** -24)).astype(f32)  # above 1 - 1e-6 (1e-6 is about 17 ulps below 1)
    ws[160:200] = (1e-6 + r.rand(40) * 1e-4).astype(f32)                        # just inside the clamp
    ws[200:240] = (r.rand(40) * 0.05 + 0.95).astype(f32)
    ws[240:260] = 0.5
    assert (ws[120:160] > 1 - EPS).all() and (ws[120:160] < 1).all() and (ws[160:200] > EPS).all()
    return r.permutation(ws)


def sparsity_terms(ws):
    w = np.asarray(ws, np.float64)
    a = np.clip(w, LO, HI)
    return w * w + 0.01, -a * np.log2(a) - (1 - a) * np.log2(1 - a), np.log(1 + 10 * w)


def sparsity_loss(ws, lambdas, mult=1.0):
    lo, le, lm = lambdas
    t0, t1, t2 = sparsity_terms(ws)
    loss = 0.0
    if lo > 0:
        loss += lo * np.sqrt(t0.mean())
    if le > 0:
        loss += le * t1.mean()
    if lm > 0:
        loss += lm * (10000 * t2.mean())
    return mult * loss


def sparsity_grad(ws, lambdas, mult=1.0):
    lo, le, lm = lambdas
    w = np.asarray(ws, np.float64)
    n = w.size
    t0 = sparsity_terms(w)[0]
    g = np.zeros_like(w)
    if lo > 0:
        g += lo * w / (n * np.sqrt(t0.mean()))
    if le > 0:
        inside = (w >= LO) & (w <= HI)
        a = np.clip(w, LO, HI)
        g += le * np.where(inside, np.log2(1 - a) - np.log2(a), 0.0) / n
    if lm > 0:
        g += lm * 10000 * 10 / ((1 + 10 * w) * n)
    return mult * g


def multiplier(step):
    return MULTIPLIER if step / MAX_ITER >= SPARSITY_STEP else 1.0


def mix(fg, ws, bg):
    """fg [N, C], ws [N], bg [C] or [N, C] -> float64 [N, C]."""
    fg, ws, bg = (np.asarray(a, np.float64) for a in (fg, ws, bg))
    return fg + (1 - ws)[:, None] * np.broadcast_to(bg, fg.shape)


def mix_grads(d, ws, bg, detach_ws=False):
    """d [N, C] = d image -> d_fg, d_ws (mix term), d_bg, and sum_c |bg_c d_c| [N]."""
    d, ws = np.asarray(d, np.float64), np.asarray(ws, np.float64)
    bgf = np.broadcast_to(np.asarray(bg, np.float64), d.shape)
    d_ws = np.zeros_like(ws) if detach_ws else -(bgf * d).sum(-1)
    return d, d_ws, (1 - ws)[:, None] * d, np.abs(bgf * d).sum(-1)
