"""Times the L1 + D-SSIM image loss (boundary B17), forward + backward, at 1 x 3 x 512 x 512 and 1 x 3 x 1024 x 1024, beside the
composition it replaces -- the reference's statements (core/gaussian/gaussian_loss.py:9-60,131-138: five grouped 11 x 11 conv2d calls and
the element-wise launches around them, autograd for the way back) written out below with torch on the same GPU in the same process --
and the nerf2gs step of a c2-sized avatar (100 000 Gaussians, 512 x 512) against a fixed target image.

    python tools/bench_image_loss.py [--reps 100] [--windows 7] [--gaussians 100000]

Per case: microseconds per call, the median over --windows event-timed windows of --reps back-to-back calls each, with the fastest and
slowest window; the fused pair and the composition take turns window by window, so drift of the clocks hits both.  Per-kernel times (the mean
of twenty fused calls) come from the library's own launch profiler.  Both sides read the same NCHW inputs; the fused pair is also timed on the
[B, H, W, C] layout the renders have (the composition would first copy those).  The last line is the whole table as JSON.
"""
import argparse
import json
import os
import sys
from math import exp

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import _lib, image_loss, sds_step  # noqa: E402


def _window(channel, device):
    gauss = torch.Tensor([exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    w = (gauss / gauss.sum()).unsqueeze(1)
    return w.mm(w.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, 11, 11).contiguous().to(device)


def composition(img1, img2, lambda_dssim=0.2):
    """The reference's ImageReconstructionLoss.__call__, statement by statement (the window is rebuilt and uploaded per call, as there)."""
    channel = img1.size(-3)
    window = _window(channel, img1.device).type_as(img1)
    mu1 = F.conv2d(img1, window, padding=5, groups=channel)
    mu2 = F.conv2d(img2, window, padding=5, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=5, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=5, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=5, groups=channel) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    Ll1 = torch.abs((img1 - img2)).mean()
    return (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim_map.mean())


def _window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _stat(ts):
    return [round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)]


def _alternate(fns, reps, windows):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            ts[k].append(_window_us(fn, reps))
    return {k: _stat(v) for k, v in ts.items()}


def _kernels_us(fn, calls=20):
    fn()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = {k: round(v[1] * 1e3 / max(v[0], 1), 2) for k, v in _lib.prof_table().items() if k.startswith("image_loss_")}
    _lib.prof_enable(False)
    return out


class _FixedTarget:
    def __init__(self, target):
        self.target = target

    def render(self, data, shading='albedo'):
        return {"image_fg": self.target}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--gaussians", type=int, default=100000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    dev = torch.device("cuda:0")
    loss_fn = image_loss.ImageReconstructionLoss()
    rows = []
    print("# MI355X, B17 image loss, forward + backward through autograd; microseconds per call (median [fastest, slowest] of %d windows "
          "of %d calls)" % (args.windows, args.reps))
    gen = torch.Generator(device=dev).manual_seed(0)
    for size in (512, 1024):
        x = torch.rand(1, 3, size, size, device=dev, generator=gen).requires_grad_(True)
        y = (x.detach() + 0.1 * torch.randn(1, 3, size, size, device=dev, generator=gen)).clamp(0, 1)
        xh = x.detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)      # the renders' [B, H, W, C]
        yh = y.permute(0, 2, 3, 1).contiguous()

        def fused():
            x.grad = None
            loss_fn(x, y).backward()

        def fused_nhwc():
            xh.grad = None
            loss_fn(xh.permute(0, 3, 1, 2), yh.permute(0, 3, 1, 2)).backward()

        def composed():
            x.grad = None
            composition(x, y).backward()

        def fused_forward():
            with torch.no_grad():
                loss_fn(x, y)
        fused()
        g_fused, l_fused = x.grad.clone(), loss_fn(x, y).item()
        composed()
        g_comp, l_comp = x.grad.clone(), composition(x, y).item()
        t = _alternate({"fused": fused, "composition": composed, "fused_nhwc": fused_nhwc, "fused_forward_only": fused_forward},
                       args.reps, args.windows)
        row = {"size": size, "fused_us": t["fused"], "composition_us": t["composition"], "fused_nhwc_us": t["fused_nhwc"],
               "fused_forward_only_us": t["fused_forward_only"], "kernels_us": _kernels_us(fused),
               "loss_fused": l_fused, "loss_composition": l_comp,
               "grad_max_abs_diff_over_max": float((g_fused - g_comp).abs().max() / g_comp.abs().max())}
        rows.append(row)
        print("1 x 3 x %4d x %-4d fused %s  composition %s  fused on [B,H,W,C] %s  fused forward only %s" % (
            size, size, row["fused_us"], row["composition_us"], row["fused_nhwc_us"], row["fused_forward_only_us"]))
        print("            kernels: %s | loss %.7f vs %.7f, gradient max |diff| / max %.2e" % (
            row["kernels_us"], l_fused, l_comp, row["grad_max_abs_diff_over_max"]), flush=True)
    # the nerf2gs step of a c2-sized avatar: render forward + image loss + backward + fused Adam
    step = sds_step.SDSStep(n_gaussians=args.gaussians, res=512, device=str(dev), guidance=False)
    data = step.data
    data["smpl_inputs"] = {k: v.to(dev) for k, v in sds_step.synth.random_smpl_inputs(seed=0, device="cpu").items()}
    teacher = _FixedTarget(torch.rand(1, 512, 512, 3, device=dev, generator=gen))
    reps = max(args.reps // 4, 10)
    t = _alternate({"nerf2gs_step": lambda: step.trainer.nerf2gs_step(data, teacher), "c2_train_step": lambda: step.trainer.train_step(data)},
                   reps, args.windows)
    row = {"gaussians": step.G, "size": 512, "nerf2gs_step_us": t["nerf2gs_step"], "c2_train_step_us": t["c2_train_step"],
           "redone_frames": step.trainer.redone_frames}
    rows.append(row)
    print("nerf2gs_step, %d Gaussians, 512 x 512, fixed target: %s  | the c2 step (render forward + backward + Adam, sum(image * W) loss) %s"
          "  (windows of %d steps)" % (step.G, row["nerf2gs_step_us"], row["c2_train_step_us"], reps), flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
