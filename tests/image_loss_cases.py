"""Cases and oracle of the image reconstruction loss (boundary B17, dreamwaltz_g_amd.image_loss).  Imports nothing of the reference.

  window2d()          the reference's window, built its way in fp32 (gaussian_loss.py:17-26): exp() in double rounded to fp32, divided by the
                      fp32 sum, outer product in fp32
  composition(...)    the reference's statements (gaussian_loss.py:9-10,40-60,135-138) in the dtype of its inputs: direct 11 x 11 grouped
                      conv2d, zero padding.  In float64 (window widened) it is THE ORACLE; in float32 it is the reference's own arithmetic,
                      whose error against the oracle sets the tolerance of the GPU tests
  evaluate(x, y, dt)  loss, l1, ssim, ssim per batch item and dloss/dx (autograd) of composition() in dtype dt
  numpy_form(x, y)    a second float64 form written without torch: the 2-D window applied row by row on a zero-padded array
  case(name)          the inputs of a case (fp32, NCHW values; `layout` says how the GPU test lays them out in memory), its oracle results
                      and the fp32 composition's errors e_ref -- computed once, shared, never modified
  self_check()        two identical images: ssim == 1 and loss == 0 exactly; the gradient is zero to the rounding of autograd's quotient rule

Inputs are generated in fp32 and widened for the oracle, so x == y means the same on both sides.
"""
import functools
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

WINDOW_SIZE, SIGMA = 11, 1.5
LAMBDA = 0.2
TILE = 16                                 # DWG_IMAGE_LOSS_TILE: the shapes below are chosen around it
SCALAR_FLOOR = 8 * 2.0 ** -24             # the terms of 1 - mean are O(1): eight fp32 roundings of an O(1) value
GRAD_FLOOR = 32 * 2.0 ** -24              # times max |g64|, max-norm over the image

#        name: (B, C, H, W), layouts, content
CASES = {
    "smaller_than_window": ((1, 3, 7, 9), ("nchw",), "noise"),
    "one_tile": ((1, 3, 16, 16), ("nchw",), "noise"),
    "one_past_a_tile": ((1, 3, 17, 33), ("nchw",), "noise"),
    "batch_ragged": ((2, 3, 37, 53), ("nchw", "nhwc"), "noise"),
    "single_plane": ((1, 1, 40, 24), ("nchw",), "noise"),
    "four_channels": ((1, 4, 21, 19), ("nhwc",), "noise"),
    "blob_shifted": ((1, 3, 48, 40), ("nhwc",), "blob"),
    "near_zero_loss": ((1, 3, 33, 17), ("nchw",), "near"),
}


def window1d():
    gauss = torch.Tensor([exp(-(x - WINDOW_SIZE // 2) ** 2 / float(2 * SIGMA ** 2)) for x in range(WINDOW_SIZE)])
    return gauss / gauss.sum()


def window2d():
    w = window1d().unsqueeze(1)
    return w.mm(w.t()).float()


def composition(x, y, lambda_dssim=LAMBDA):
    """-> (loss, l1, ssim, ssim per batch item), in x's dtype."""
    C = x.shape[1]
    window = window2d().unsqueeze(0).unsqueeze(0).expand(C, 1, WINDOW_SIZE, WINDOW_SIZE).contiguous().to(x.dtype)
    conv = lambda t: F.conv2d(t, window, padding=WINDOW_SIZE // 2, groups=C)      # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(x * x) - mu1_sq
    sigma2_sq = conv(y * y) - mu2_sq
    sigma12 = conv(x * y) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    ssim = ssim_map.mean()
    l1 = torch.abs(x - y).mean()
    loss = (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim)
    return loss, l1, ssim, ssim_map.mean(1).mean(1).mean(1)


def evaluate(x32, y32, dtype):
    x = x32.to(dtype).clone().requires_grad_(True)
    loss, l1, ssim, per_item = composition(x, y32.to(dtype))
    loss.backward()
    return {"loss": float(loss.detach().double()), "l1": float(l1.detach().double()), "ssim": float(ssim.detach().double()),
            "ssim_batch": per_item.detach().double().numpy(), "grad": x.grad.detach().double().numpy()}


def numpy_form(x32, y32, lambda_dssim=LAMBDA):
    """loss, l1, ssim in float64 numpy.  (A rank-1 separable form cannot agree with the oracle to 1e-12: the reference's window is the
    fp32-ROUNDED outer product, 2^-24 relative off the exact one per weight.  So each of the window's eleven rows is applied as a 1-D
    filter along the image rows, and the eleven results are added down the columns.)"""
    w2 = window2d().numpy().astype(np.float64)
    x, y = x32.numpy().astype(np.float64), y32.numpy().astype(np.float64)
    R = WINDOW_SIZE // 2
    H, W = x.shape[-2:]

    def filt(a):
        p = np.zeros(a.shape[:-2] + (H + 2 * R, W + 2 * R))
        p[..., R:R + H, R:R + W] = a
        out = np.zeros_like(a)
        for i in range(WINDOW_SIZE):
            row = np.zeros(a.shape[:-2] + (H, W))
            for j in range(WINDOW_SIZE):
                row += w2[i, j] * p[..., i:i + H, j:j + W]
            out += row
        return out
    mu1, mu2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    ssim, l1 = m.mean(), np.abs(x - y).mean()
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim), l1, ssim


def _inputs(shape, content, seed):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    if content == "noise":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if content == "near":
        x = torch.rand(shape, generator=g)
        return x, (x + 1e-3 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)
    # a flat-coloured disc on zeros; the target is the disc 2.5 pixels to the right: the mean of the discs 2 and 3 pixels to the right,
    # so the colour inside (0.5 c + 0.5 c) and the zeros outside are exactly the image's
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    colour = torch.tensor([0.8, 0.4, 0.2, 0.6][:C]).reshape(1, C, 1, 1)
    disc = lambda dx: (((xx - dx - 0.45 * W) ** 2 + (yy - 0.5 * H) ** 2) < (0.28 * min(H, W)) ** 2).float().reshape(1, 1, H, W)      # noqa: E731
    x = (disc(0.0) * colour).expand(B, C, H, W).contiguous()
    y = ((0.5 * disc(2.0) + 0.5 * disc(3.0)) * colour).expand(B, C, H, W).contiguous()
    return x, y


@functools.lru_cache(maxsize=None)
def case(name):
    shape, layouts, content = CASES[name]
    x, y = _inputs(shape, content, seed=1 + sorted(CASES).index(name))
    want = evaluate(x, y, torch.float64)
    ref32 = evaluate(x, y, torch.float32)
    e_ref = {k: float(np.max(np.abs(np.asarray(ref32[k]) - np.asarray(want[k])))) for k in want}
    return {"name": name, "shape": shape, "layouts": layouts, "x": x, "y": y, "want": want, "e_ref": e_ref}


def bound(c, key):
    """max(4 e_ref, floor): the factor 4 covers a different but equally long summation order (11 + 11 separable terms against 121 direct)."""
    floor = GRAD_FLOOR * float(np.max(np.abs(c["want"]["grad"]))) if key == "grad" else SCALAR_FLOOR
    return max(4.0 * c["e_ref"][key], floor)


def self_check():
    """Two identical images.  The SSIM map's numerator and denominator are then the same floating-point expressions, so ssim == 1 and
    loss == 0 EXACTLY.  The gradient is zero in exact arithmetic; autograd's quotient rule forms it as g / D - g N / D^2, which at N == D
    cancels to the rounding of those two quotients (measured 4.5e-19 on 1 x 3 x 17 x 33), so it is held to one float64 ulp of the O(1) map."""
    x, _ = _inputs((1, 3, 17, 33), "noise", seed=99)
    out = evaluate(x, x.clone(), torch.float64)
    assert out["ssim"] == 1.0 and out["loss"] == 0.0 and out["l1"] == 0.0, out
    assert float(np.max(np.abs(out["grad"]))) <= 2.0 ** -52, float(np.max(np.abs(out["grad"])))
    return out
