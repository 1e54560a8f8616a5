"""Times the NeRF-stage ray marcher (boundary B6) at the stage-I shapes.

    python tools/bench_raymarch.py [--reps 10]

Rays of one camera at 64^2 .. 512^2 (radius 1-2, 40-70 degree fov, looking at the origin), grid H=128, C=2, bound=2, max_steps=1024,
dt_gamma=0, for a body-sized occupancy blob and a dense grid.  For each of the march (count + scan + write, the reference's protocol
with its one host read of M), composite forward and composite backward it prints milliseconds (median of --reps, CUDA events), M, the
algorithmic bytes (32 B / sample written by the march, 28 B read+written by the forward, 44 B by the backward) and the fraction of the
8 TB/s HBM peak those bytes make.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import raymarch as rm  # noqa: E402
from tests import raymarch_cases as rc  # noqa: E402

PEAK = 8e12
BYTES = {"march": 32, "composite_fwd": 28, "composite_bwd": 44}


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    C, H, bound, max_steps = 2, 128, 2.0, 1024
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, device="cuda")
    rows = []
    print("%-6s %-5s %-14s %9s %10s %10s %7s" % ("rays", "grid", "stage", "ms", "M", "MB", "HBM%"))
    for kind in ("body", "dense"):
        _, bits = rc.make_grid(C, H, bound, kind)
        bits = torch.from_numpy(bits).cuda()
        for W in (64, 128, 256, 512):
            o, d = rc.make_cameras(1, W, W, seed=1)
            o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
            nears, fars = rm.near_far_from_aabb(o, d, aabb, 0.05)
            N = o.shape[0]

            def march():
                return rm.march_rays_train(o, d, bound, bits, C, H, nears, fars, False, 0.0, max_steps)
            xyzs, dirs, ts, rays = march()
            M = xyzs.shape[0]
            g = torch.Generator(device="cuda").manual_seed(0)
            sig = torch.rand(M, device="cuda", generator=g) * 20
            col = torch.rand(M, 3, device="cuda", generator=g)
            w = torch.zeros(M, device="cuda"); ws = torch.empty(N, device="cuda"); dep = torch.empty(N, device="cuda")
            img = torch.empty(N, 3, device="cuda")
            gw, gws, gd, gi = (torch.randn(s, device="cuda", generator=g) for s in ((M,), (N,), (N,), (N, 3)))
            gs = torch.zeros(M, device="cuda"); gr = torch.zeros(M, 3, device="cuda")

            def fwd():
                rm.composite_rays_train_forward_into(sig, col, ts, rays, M, N, 1e-4, False, w, ws, dep, img, 3)

            def bwd():
                rm.composite_rays_train_backward_into(gw, gws, gd, gi, sig, col, ts, rays, ws, dep, img, M, N, 1e-4, False, gs, gr, 3)
            fwd()
            for stage, fn in (("march", march), ("composite_fwd", fwd), ("composite_bwd", bwd)):
                ms = _time(fn, args.reps)
                nbytes = BYTES[stage] * M
                frac = nbytes / (ms * 1e-3) / PEAK
                rows.append(dict(rays=W * W, grid=kind, stage=stage, ms=round(ms, 4), M=M, bytes=nbytes, hbm_frac=round(frac, 4)))
                print("%-6s %-5s %-14s %9.3f %10d %10.1f %6.1f%%" % ("%d^2" % W, kind, stage, ms, M, nbytes / 1e6, 100 * frac))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
