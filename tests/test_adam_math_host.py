"""Host-side test of the fused Adam's arithmetic: csrc/adam_math.h compiled for the host (gcc -O2 -ffp-contract=off) against a float64
restatement of torch.optim.Adam's statements, itself pinned to torch.optim.Adam on float64 tensors.

The host build is uncontracted and the device build is not (adam_math.h says why), so this cannot assert the device's bits; it asserts the
optimizer's bound instead.  THE BOUND on the parameters after every step is tests/test_adam_gpu.py's: |err| <= 2e-6 + 2e-5 |ref|.  The
moments take a handful of fp32 roundings a step (the scaled gradient, two products and a sum; g g (1 - b2) one more), each at most 2^-24 of
the largest term: |err| <= 5 steps 2^-24 max(|ref|, |scaled g|) for m, and the same with the squares for v."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32
N, STEPS, ZEROS = 1000, 5, 16           # the first ZEROS elements never see a gradient


def _hostlib():
    src = os.path.join(HERE, "hostmath", "adam_math_host.c")
    out = os.path.join(HERE, "hostmath", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libadam_math_host.so")
    hdr = os.path.join(ROOT, "dreamwaltz-g_amd", "csrc", "adam_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src, "-lm"], check=True)
    L = ctypes.CDLL(so)
    fl, vp = ctypes.c_float, ctypes.c_void_p
    L.host_adam_row.argtypes = [fl, fl, fl, ctypes.c_int32, fl, fl, vp]
    L.host_adam_update.argtypes = [ctypes.c_int64, vp, fl, fl, fl] + [vp] * 4
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _inputs():
    rng = np.random.RandomState(5)
    p0 = rng.randn(N).astype(f32)
    grads = rng.randn(STEPS, N).astype(f32) * np.logspace(-3, 1, N).astype(f32)      # gradients from 1e-3 to 10 in magnitude
    grads[:, :ZEROS] = 0.0
    return p0, grads


def _float64_adam(p0, grads, lr, betas, eps, factor):
    """torch.optim.Adam's statements (amsgrad=False, weight_decay=0) in float64 on gradients multiplied by `factor` -> per step (p, m, v)."""
    p, m, v = p0.astype(np.float64), np.zeros(N), np.zeros(N)
    out = []
    for t, g in enumerate(grads, 1):
        g = g.astype(np.float64) * factor
        m = betas[0] * m + (1.0 - betas[0]) * g
        v = betas[1] * v + (1.0 - betas[1]) * g * g
        p = p - lr / (1.0 - betas[0] ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - betas[1] ** t) + eps)
        out.append((p, m, v))
    return out


# (lr, betas, eps, grad_scale, scale): the avatar's eps 1e-15 and torch's default 1e-8, a plain step, the multi-view mean (grad_scale 1/2)
# and a step under a loss scaler
CASES = [(1e-2, (0.9, 0.99), 1e-15, 1.0, 1.0), (1e-3, (0.9, 0.999), 1e-8, 1.0, 1.0), (1e-2, (0.9, 0.999), 1e-15, 0.5, 1.0),
         (3e-3, (0.9, 0.99), 1e-8, 0.25, 3.0)]


@pytest.mark.parametrize("lr,betas,eps,grad_scale,scale", CASES)
def test_adam_math_h_against_float64_adam(lr, betas, eps, grad_scale, scale):
    L = _hostlib()
    p0, grads = _inputs()
    # the hyper-parameters as the C ABI receives them: fp32
    lr, eps, b1, b2 = (float(f32(x)) for x in (lr, eps, betas[0], betas[1]))
    factor = float(f32(grad_scale)) / float(f32(scale))
    want = _float64_adam(p0, grads, lr, (b1, b2), eps, factor)
    p, m, v = p0.copy(), np.zeros(N, f32), np.zeros(N, f32)
    ulp = 2.0 ** -24
    for t, g in enumerate(grads, 1):
        row = np.zeros(4, f32)
        L.host_adam_row(lr, b1, b2, t, grad_scale, scale, _p(row))
        assert row[2] == f32(factor) and row[3] == 0.0
        L.host_adam_update(N, _p(row), b1, b2, eps, _p(g), _p(p), _p(m), _p(v))
        rp, rm, rv = want[t - 1]
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
        ep = np.abs(p - rp)
        print("step %d: max param err %.3g, worst err / bound %.3g" % (t, ep.max(), (ep / (2e-6 + 2e-5 * np.abs(rp))).max()))
        assert (ep <= 2e-6 + 2e-5 * np.abs(rp)).all(), (t, ep.max())
        gs = np.abs(grads[:t].astype(np.float64) * factor).max(0)
        assert (np.abs(m - rm) <= 5 * t * ulp * np.maximum(np.abs(rm), gs)).all(), t
        assert (np.abs(v - rv) <= 5 * t * ulp * np.maximum(rv, gs * gs)).all(), t
        # v = 0 with g = 0: 0 / (0 + eps) is 0, the parameter keeps its bits
        assert np.array_equal(p[:ZEROS].view(np.uint32), p0[:ZEROS].view(np.uint32))
        assert not m[:ZEROS].any() and not v[:ZEROS].any()
    assert not np.array_equal(p[ZEROS:], p0[ZEROS:])


def test_float64_restatement_is_torch_adam():
    p0, grads = _inputs()
    lr, betas, eps = 1e-2, (0.9, 0.99), 1e-15
    want = _float64_adam(p0, grads, lr, betas, eps, 0.5)
    q = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps)
    for t, g in enumerate(grads, 1):
        q.grad = torch.from_numpy(g).double() * 0.5
        opt.step()
        st = opt.state[q]
        for got, ref in ((q.detach(), want[t - 1][0]), (st["exp_avg"], want[t - 1][1]), (st["exp_avg_sq"], want[t - 1][2])):
            assert np.allclose(got.numpy(), ref, rtol=1e-12, atol=1e-14), t
