"""CPU check of the hand-derived backward of the shaded training render (csrc/shade_math.h compiled for the host with gcc
-ffp-contract=off) against float64 torch autograd of the reference's statements (core/nerf/nerf_model.py:84-105, 155-168) on the same
fp32 inputs.  Needs no device.

THE BOUND.  Per component of dsigma_fd: 32 * 2^-23 * |dn|_2 * 0.5 / (eps max(|g|, 1e-10)); for dalbedo 32 * 2^-23 * max |grad_rgb|.
With u = 2^-24 (half an ulp, the error of one rounding) the bound is 64 u S, S = |dn| / (2 eps len) being the largest magnitude a
component of the result can have (ds = 0.5 dg / eps and |dg| = |du - n (n.du)| / len <= |du| / len).  Counting first-order relative
errors, every one taken at its worst and all aligned:
  g_k: a difference and a quotient, 2 u;  len = sqrt(clamp(sum g^2)): (2 2 + 1 + 2) / 2 + 1 = 4.5 u;  n_k = g_k / len: 7.5 u;
  dn (lambert shadings): dlam is summed in double and rounded once, then two products: 3 u of |dn|; 'normal': dn = grad / 2, exact;
  dlen = -sum du_k (n_k / len): per term 7.5 + 4.5 + 1 + 1 = 14 u, two adds: 16 u of |du| / len (Cauchy, |n| = 1);
  dd = dlen / (2 len): 21.5 u;  dd g_k + dd g_k: 25 u of |n_k| |du| / len;  du_k / len: 5.5 u;  their sum 1 u;  / eps 1 u;  * -0.5 exact.
That is (25 + 5.5 + 2 + 2 * 3) u = 38.5 u of S, under 64 u: 32 ulps hold with room and without any measured figure.  Below the clamp
len is sqrt(1e-20f), dd is 0 and only du_k / len remains.  dalbedo = grad lam with lam <= 1 known to 16 u (three normals of 7.5 u in a
three-term product sum, one product, one add): 17 u of |grad|.
Measured on this file's rows (printed by the tests): at most 0.064 of the bound for dsigma_fd and 0.028 for dalbedo."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
EPS = f32(1e-3)
RATIO = f32(0.1)
LIGHT = (np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])).astype(f32)
SHADINGS = {'normal': 1, 'textureless': 2, 'lambertian': 3}
FACTOR = 32 * 2.0 ** -23


def _hostlib():
    src = os.path.join(HERE, "hostmath", "shade_math_host.c")
    out = os.path.join(HERE, "hostmath", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libshade_math_host.so")
    hdr = os.path.join(HERE, "..", "dreamwaltz-g_amd", "csrc", "shade_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src, "-lm"], check=True)
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _host(shading, s, alb, light, grad):
    """shade_math.h on fp32 rows -> normals, rgbs, dsigma_fd, dalbedo."""
    L = _hostlib()
    M = len(s)
    s, alb, grad, light = (np.ascontiguousarray(a, f32) for a in (s, alb, grad, light))
    n, rgb, ds, da = np.zeros((M, 3), f32), np.zeros((M, 3), f32), np.zeros((M, 6), f32), np.zeros((M, 3), f32)
    L.host_shade_forward(SHADINGS[shading], M, _p(s), _p(alb), _p(light), ctypes.c_float(RATIO), ctypes.c_float(EPS), _p(n), _p(rgb))
    L.host_shade_backward(SHADINGS[shading], M, _p(s), _p(alb), _p(light), ctypes.c_float(RATIO), ctypes.c_float(EPS), _p(grad), _p(ds), _p(da))
    return n, rgb, ds, da


def _autograd(shading, s, alb, light, grad, dtype):
    """The reference's statements in `dtype` on the fp32 values -> g, normal, dot, rgb, dn, dsigma_fd, dalbedo (numpy float64)."""
    s = torch.tensor(np.asarray(s, f32)).to(dtype).requires_grad_(True)
    alb = torch.tensor(np.asarray(alb, f32)).to(dtype).requires_grad_(True)
    l = torch.tensor(np.asarray(light, f32)).to(dtype)
    # the Python scalars as the fp32 kernels get them: epsilon, ratio and 1 - ratio rounded to fp32
    epsilon, ratio, omr = float(EPS), float(RATIO), float(f32(1.0 - float(RATIO)))
    g = - 0.5 * torch.stack([s[:, 0] - s[:, 1], s[:, 2] - s[:, 3], s[:, 4] - s[:, 5]], dim=-1) / epsilon
    normal = g / torch.sqrt(torch.clamp(torch.sum(g * g, -1, keepdim=True), min=1e-20))
    normal = torch.nan_to_num(normal)
    normal.retain_grad()
    dot = normal @ -l
    if shading == 'normal':
        color = (normal + 1.0) / 2.0
    else:
        lambertian = ratio + omr * dot.clamp(min=0)
        color = lambertian.unsqueeze(-1).repeat(1, 3) if shading == 'textureless' else alb * lambertian.unsqueeze(-1)
    color.backward(torch.tensor(np.asarray(grad, f32)).to(dtype))
    da = alb.grad if alb.grad is not None else torch.zeros_like(alb)
    return tuple(t.detach().double().numpy() for t in (g, normal, dot, color, normal.grad, s.grad, da))


def _rows(seed=0):
    """-> sigma_fd [M, 6], and the index ranges of the crafted rows."""
    rng = np.random.RandomState(seed)
    rand = np.exp(rng.randn(4096, 6) * 1.5).astype(f32)                 # densities over three decades: |g| from ~1 to ~1e5
    flat = np.repeat(np.exp(rng.randn(64, 3)).astype(f32), 2, axis=1)   # s+ == s- on every axis: g = 0
    tiny = np.zeros((64, 6), f32)                                       # |g| = 0.25e-10 .. 0.5e-10 (below the clamp) and 2e-10 .. 4e-10 (above)
    for i in range(64):
        mag = (0.5e-13 if i < 32 else 4e-13) * (1 + (i % 8) / 8.0)      # s+ - s- = 2 eps |g|
        tiny[i, 2 * (i % 3)] = mag * (2 if i & 1 else 1)
        tiny[i, 2 * (i % 3) + 1] = mag * (1 if i & 1 else 2)
        tiny[i, 2 * ((i + 1) % 3)] = mag * 0.5 * (i % 4 == 0)
    s = np.concatenate([rand, flat, tiny])
    return s, {"rand": slice(0, 4096), "flat": slice(4096, 4160), "tiny": slice(4160, 4224)}


def _compare(shading, s, alb, light, grad):
    n, rgb, ds, da = _host(shading, s, alb, light, grad)
    g64, n64, dot64, rgb64, dn64, ds64, da64 = _autograd(shading, s, alb, light, grad, torch.float64)
    assert np.abs(n - n64).max() <= 16 * 2.0 ** -23 and np.abs(rgb - rgb64).max() <= 16 * 2.0 ** -23
    glen = np.sqrt((g64 * g64).sum(-1))
    scale = np.sqrt((dn64 * dn64).sum(-1)) * 0.5 / (float(EPS) * np.maximum(glen, 1e-10))
    bound = FACTOR * scale[:, None]
    err = np.abs(ds - ds64)
    worst = float((err / np.maximum(bound, 1e-300))[bound[:, 0] > 0].max()) if (bound > 0).any() else 0.0
    assert (err <= bound).all(), (shading, worst)
    gmax = float(np.abs(grad).max())
    worst_a = float(np.abs(da - da64).max() / (FACTOR * gmax))
    assert worst_a <= 1.0, (shading, worst_a)
    print("shade_math %s: dsigma_fd error / bound %.3g, dalbedo error / bound %.3g" % (shading, worst, worst_a))
    return dict(n=n, ds=ds, da=da, g=g64, dot=dot64, ds64=ds64, da64=da64, glen=glen)


@pytest.mark.parametrize("shading", ['normal', 'textureless', 'lambertian'])
def test_backward_against_float64_autograd(shading):
    s, idx = _rows()
    rng = np.random.RandomState(1)
    alb = rng.uniform(0.05, 0.95, (len(s), 3)).astype(f32)
    grad = rng.randn(len(s), 3).astype(f32)
    r = _compare(shading, s, alb, LIGHT, grad)
    # the rows reach their branches
    assert (r["glen"][idx["flat"]] == 0).all() and (r["n"][idx["flat"]] == 0).all()
    below = r["glen"][idx["tiny"]] ** 2 < 1e-20
    assert 16 <= below.sum() <= 48 and (r["glen"][idx["tiny"]] > 0).all()
    assert (r["glen"][idx["rand"]] ** 2 > 1e-20).all()
    if shading == 'normal':
        # below the clamp the gradient is dn / 1e-10 (no projection): the reference's huge value
        assert (np.abs(r["ds"][idx["flat"]]).max(-1) > 1e8).all()
        assert r["da"].max() == 0 and r["da"].min() == 0
    else:
        lit = r["dot"][idx["rand"]] > 0
        assert 0.4 <= lit.mean() <= 0.6, lit.mean()
        unlit_rows = np.nonzero(~lit)[0]
        assert (r["ds"][unlit_rows] == 0).all() and (np.abs(r["ds"][np.nonzero(lit)[0]]).max(-1) > 0).all()
        # a zero normal has n . -l == 0: the clamp passes the gradient there
        assert (np.abs(r["ds"][idx["flat"]]).max(-1) > 0).all()
    if shading == 'lambertian':
        assert (np.abs(r["da"]).max(-1) > 0).all()


@pytest.mark.parametrize("shading", ['textureless', 'lambertian'])
def test_the_clamp_passes_the_gradient_at_exactly_zero(shading):
    """g along +-x and a light in the yz plane: n = (+-1, 0, 0) and n . -l == 0 exactly, in fp32 and in float64.  clamp(min=0) passes
    the gradient where its input is >= 0, so the y and z densities get one."""
    rng = np.random.RandomState(2)
    s = np.repeat(np.exp(rng.randn(32, 3)).astype(f32), 2, axis=1)
    s[:, 0] = s[:, 1] * f32(1.5)
    s[16:, 0] = s[16:, 1] * f32(0.5)
    alb = rng.uniform(0.05, 0.95, (32, 3)).astype(f32)
    grad = rng.randn(32, 3).astype(f32)
    light = np.array([0.0, 0.6, 0.8], f32)
    r = _compare(shading, s, alb, light, grad)
    assert (r["dot"] == 0).all() and (np.abs(r["n"][:, 0]) == 1).all()
    assert (np.abs(r["ds"][:, 2:]).min(-1) > 0).all() and (np.abs(r["ds64"][:, 2:]).min(-1) > 0).all()


@pytest.mark.parametrize("shading", ['normal', 'textureless', 'lambertian'])
def test_non_finite_densities_travel_as_in_fp32_autograd(shading):
    """Rows with a NaN or an infinite density against fp32 CPU torch autograd: NaN where it has NaN, zero where it has zero, and the
    finite values within the bound (taken from fp32 autograd's own dn and g where those are finite)."""
    rng = np.random.RandomState(3)
    s = np.exp(rng.randn(96, 6)).astype(f32)
    for i in range(96):
        s[i, i % 6] = [np.nan, np.inf, -np.inf][i % 3]
        if i >= 48:
            s[i, (i + 3) % 6] = [np.inf, np.nan, np.inf][i % 3]
    alb = rng.uniform(0.05, 0.95, (96, 3)).astype(f32)
    grad = rng.randn(96, 3).astype(f32)
    with np.errstate(all="ignore"):
        n, rgb, ds, da = _host(shading, s, alb, LIGHT, grad)
        g32, n32, _, rgb32, dn32, ds32, da32 = _autograd(shading, s, alb, LIGHT, grad, torch.float32)
        assert np.array_equal(np.isnan(rgb), np.isnan(rgb32)) and np.array_equal(np.isnan(ds), np.isnan(ds32))
        assert np.array_equal(np.isnan(da), np.isnan(da32))
        assert np.array_equal(ds == 0, ds32 == 0) and np.array_equal(da == 0, da32 == 0)
        fin = np.isfinite(ds) & np.isfinite(ds32)
        glen = np.sqrt((g32 * g32).sum(-1))
        scale = np.sqrt((dn32 * dn32).sum(-1)) * 0.5 / (float(EPS) * np.maximum(glen, 1e-10))
        bound = np.broadcast_to(FACTOR * scale[:, None], ds.shape)
        assert (np.abs(ds - ds32)[fin] <= np.nan_to_num(bound[fin], nan=0.0, posinf=0.0)).all()
        fa = np.isfinite(da) & np.isfinite(da32)
        assert (np.abs(da - da32)[fa] <= FACTOR * float(np.abs(grad).max())).all()
    print("non-finite rows: %d NaN and %d zero components of dsigma_fd" % (int(np.isnan(ds).sum()), int((ds == 0).sum())))
