"""Times the NeRF stage's field network (boundary B7) at the sample counts stage I marches: the fused kernel (dreamwaltz_g_amd.nerf, f16
as the recipe's --optim.fp16 runs it) against the composition a bound user gets without it -- the package GridEncoder (B2) plus
torch.nn.Linear layers under torch.autocast(fp16), tests/nerf_field_cases._NeRFNetwork.common_forward.

    python tools/bench_nerf_field.py [--reps 5] [--sizes 64,128,256,512] [--grids body,dense]

Points come from the B6 march over tests/raymarch_cases.make_grid (body-shaped and dense occupancy grids), as tools/bench_raymarch.py
draws them.  Per case: M, forward and forward + backward ms (median of CUDA events), peak memory above the inputs
(torch.cuda.max_memory_allocated), and for the fused kernel its nominal bytes per point and the HBM fraction they imply.  A composition
that runs out of memory is reported as OOM, one that an argument limit of its kernels refuses as FAIL.  The last line is the whole table as JSON.
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
from dreamwaltz_g_amd import nerf  # noqa: E402
from dreamwaltz_g_amd import raymarch as rm  # noqa: E402
from tests import nerf_field_cases as nc  # noqa: E402
from tests import raymarch_cases as rc  # noqa: E402

PEAK = 8e12
# nominal HBM bytes per point of the fused kernel (L = 16, rgb, f16): forward reads x (12) and writes sigma + albedo (4 + 6); the
# backward reads x, dsigma, dalbedo (22), writes and reads d_enc [32] fp32 and the normalised x (2 x 140), and the slab-binned table
# gradient writes and reads 16 levels x 8 corners of 16-byte records (2 x 2048)
BYTES_FWD = 22
BYTES_FWD_BWD = 22 + 22 + 280 + 4096


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _measure(fn, reps):
    """(median ms, peak bytes above what was allocated before) or ("OOM", None)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        ms = _time(fn, reps)
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return "OOM", None
    except RuntimeError as e:          # an argument limit, e.g. the B2 encoder's B * L < 2^32 at the dense 512^2 case; anything else ends the run
        if "DWG error -1" not in str(e) and "DWG error -3" not in str(e):
            raise
        print("  (%s)" % str(e).splitlines()[0][:120])
        torch.cuda.empty_cache()
        return "FAIL", None
    torch.cuda.synchronize()
    return ms, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,128,256,512")
    ap.add_argument("--grids", default="body,dense")
    args = ap.parse_args()
    C, H, bound, max_steps = 2, 128, nc.BOUND, 1024
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, device="cuda")
    net = nc.make_network(seed=0).cuda()
    rows = []
    print("%-6s %-5s %10s  %-11s %9s %9s %9s %9s %7s" % ("rays", "grid", "M", "path", "fwd ms", "f+b ms", "peak MB", "B/pt", "HBM%"))
    for kind in args.grids.split(","):
        _, bits = rc.make_grid(C, H, bound, kind)
        bits = torch.from_numpy(bits).cuda()
        for W in (int(s) for s in args.sizes.split(",")):
            o, d = rc.make_cameras(1, W, W, seed=1)
            o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
            nears, fars = rm.near_far_from_aabb(o, d, aabb, 0.05)
            xyzs = rm.march_rays_train(o, d, bound, bits, C, H, nears, fars, False, 0.0, max_steps)[0]
            M = xyzs.shape[0]
            g = torch.Generator(device="cuda").manual_seed(0)
            ds = torch.randn(M, device="cuda", generator=g)
            da = torch.randn(M, 3, device="cuda", generator=g).half()

            def run(path, backward):
                def fn():
                    for p in net.parameters():
                        p.grad = None
                    with torch.autocast("cuda", dtype=torch.float16), torch.set_grad_enabled(backward):
                        if path == "fused":
                            s, a = nerf.nerf_field(xyzs, net.encoder, net.sigma_net, net.sigma_scale, net.bound)
                        else:
                            s, a = net.common_forward(xyzs)
                    if backward:
                        ((s * ds).sum() + (a.float() * da.float()).sum()).backward()
                return fn
            for path in ("fused", "composition"):
                f_ms, _ = _measure(run(path, False), args.reps)
                fb_ms, peak = _measure(run(path, True), args.reps)
                row = dict(rays=W * W, grid=kind, M=M, path=path, fwd_ms=f_ms, fwd_bwd_ms=fb_ms, peak_bytes=peak)
                if path == "fused" and not isinstance(f_ms, str) and not isinstance(fb_ms, str):
                    row["bytes_per_point"] = BYTES_FWD_BWD
                    row["hbm_frac_fwd"] = round(BYTES_FWD * M / (f_ms * 1e-3) / PEAK, 4)
                    row["hbm_frac_fwd_bwd"] = round(BYTES_FWD_BWD * M / (fb_ms * 1e-3) / PEAK, 4)
                rows.append(row)

                def fmt(v):
                    return "%9s" % v if isinstance(v, str) else "%9.3f" % v
                print("%-6s %-5s %10d  %-11s %s %s %9s %9s %7s" % (
                    "%d^2" % W, kind, M, path, fmt(f_ms), fmt(fb_ms), "-" if peak is None else "%.0f" % (peak / 1e6),
                    row.get("bytes_per_point", "-"), ("%.1f%%" % (100 * row["hbm_frac_fwd_bwd"])) if "hbm_frac_fwd_bwd" in row else "-"))
            del xyzs, ds, da
            torch.cuda.empty_cache()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
