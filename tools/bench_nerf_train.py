"""Times the NeRF stage's training render (boundary B18, dreamwaltz_g_amd.nerf_render.render_rays_train) against the composition it
replaces -- raymarch.march_rays_train -> nerf.nerf_field -> raymarch.composite_rays_train, the entry points a bound network ran before
it -- in one process, on the body cases of tools/bench_nerf_field.py (C = 2, H = 128, f16 as the recipe's --optim.fp16 runs it).

    python tools/bench_nerf_train.py [--reps 7] [--sizes 128,256,512] [--limit 120] [--shading normal|textureless|lambertian]

--shading (boundary B19): the shaded training render against ITS composition, the statements a bound network's forward ran for the same
call: march_rays_train -> seven launches of the fused field (the points and their six shifts) -> the torch statements of the normal and
the shading (core/nerf/nerf_model.py:84-105, 146-169) -> composite_rays_train, and autograd through all of it.  'normal' runs under fp16
autocast like the 'albedo' table; 'textureless' and 'lambertian' run in f32, where both paths take them.  weights_sum and depth are
compared bit for bit, the image by its largest difference.

Density levels:
  present    the network of tools/bench_nerf_field.py as it is (random weights, no density prior)
  opaque     the same with the density bias raised by ln(9.2 / (10 dt_min)): at a pre-activation of 0 a ray is spent (T < 1e-4) within ten
             samples of the smallest step
  unculled   the present density with T_thresh = 0: nothing stops, M_live == M, and the native call does strictly more work than the
             composition (two scans, one gather, one 4-byte read): its overhead
Per case and level: M, M_live, the culled share, the median live count of the rays that have samples; forward (grad enabled, so the
native call's scan and gather are in it) and forward + backward ms as min / median / max over the repetitions, CUDA events, the two paths
alternating inside every repetition after one warm-up each; peak memory above the inputs (torch.cuda.max_memory_allocated) of one forward
+ backward.  Outputs are compared once per case (torch.equal).  Every timed step runs under a time limit of its own (faulthandler's
watchdog thread, which does not need the interpreter): a step that exceeds it, a hung device synchronise included, ends the process at
once; stderr names the step.  The last line is the whole table as JSON.
"""
import argparse
import contextlib
import faulthandler
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import nerf, nerf_render  # noqa: E402
from dreamwaltz_g_amd import raymarch as rm  # noqa: E402
from tests import nerf_field_cases as nc  # noqa: E402
from tests import raymarch_cases as rc  # noqa: E402

C, H, MAX_STEPS = 2, 128, 1024
KW = dict(density_activation='exp', density_prior='none', albedo_sigmoid=True)
AMBIENT, EPSILON = 0.1, 1e-3


def shaded_composition(field, bound, x, light, shading):
    """forward() and normal() of the reference's network over the fused field: (sigma, colour)."""
    def sigma_at(p):
        return nerf.nerf_field(p, *field, **KW)[0]
    sigma, albedo = nerf.nerf_field(x, *field, **KW)
    d = []
    for a in range(3):
        for sign in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[a] = sign * EPSILON
            d.append(sigma_at((x + torch.tensor([v], device=x.device)).clamp(-bound, bound)))
    normal = - 0.5 * torch.stack([d[0] - d[1], d[2] - d[3], d[4] - d[5]], dim=-1) / EPSILON
    normal = normal / torch.sqrt(torch.clamp(torch.sum(normal * normal, -1, keepdim=True), min=1e-20))
    normal = torch.nan_to_num(normal)
    if shading == 'normal':
        return sigma, (normal + 1.0) / 2.0
    lambertian = AMBIENT + (1 - AMBIENT) * (normal @ -light).clamp(min=0)
    if shading == 'textureless':
        return sigma, lambertian.unsqueeze(-1).repeat(1, 3)
    return sigma, albedo * lambertian.unsqueeze(-1)


@contextlib.contextmanager
def _limit(seconds, what):
    """faulthandler's watchdog is a C thread: it ends the process (traceback to stderr, exit status 1) even while the main thread sits in
    a blocking device synchronise, where a Python signal handler would never run."""
    sys.stderr.write("bench_nerf_train: %s (limit %d s)\n" % (what, seconds))
    sys.stderr.flush()
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ts):
    return {"min": float(np.min(ts)), "median": float(np.median(ts)), "max": float(np.max(ts))}


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--shading", default="albedo", choices=["albedo", "normal", "textureless", "lambertian"])
    args = ap.parse_args()
    shading = args.shading
    f16 = shading in ("albedo", "normal")
    light = torch.tensor([0.3, -0.5, 0.8]) / torch.tensor([0.3, -0.5, 0.8]).norm()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nerf_train needs a GPU")
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions")
    bound = nc.BOUND
    dt_min = 2.0 * math.sqrt(3.0) / MAX_STEPS
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, device="cuda")
    light = light.cuda()
    shade_kw = {} if shading == "albedo" else dict(shading=shading, light_d=light, ambient_ratio=AMBIENT, epsilon=EPSILON)
    _, bits = rc.make_grid(C, H, bound, "body")
    bits = torch.from_numpy(bits).cuda()
    nets = {"present": nc.make_network(seed=0).cuda(), "opaque": nc.make_network(seed=0).cuda()}
    with torch.no_grad():
        nets["opaque"].sigma_net.net[-1].bias[0] += math.log(9.2 / (10 * dt_min))
    levels = [("present", "present", 1e-4), ("opaque", "opaque", 1e-4), ("unculled", "present", 0.0)]
    rows = []
    print("%-6s %-9s %10s %10s %7s %6s  %-11s %-22s %-22s %8s" % ("rays", "density", "M", "M_live", "culled", "live~", "path",
                                                                 "fwd ms min/med/max", "f+b ms min/med/max", "peak MB"))
    for W in (int(s) for s in args.sizes.split(",")):
        o, d = rc.make_cameras(1, W, W, seed=1)
        o, d = torch.from_numpy(o).cuda().contiguous(), torch.from_numpy(d).cuda().contiguous()
        N = W * W
        nears, fars = rm.near_far_from_aabb(o, d, aabb, 0.05)
        noises = torch.zeros(N, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(0)
        g_ws, g_d, g_img = (torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g),
                            torch.randn(N, 3, device="cuda", generator=g))
        for level, which, T_thresh in levels:
            net = nets[which]
            field = (net.encoder, net.sigma_net, net.sigma_scale, bound)

            def native(stats=False):
                with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
                    return nerf_render.render_rays_train(o, d, nears, fars, bits, C, H, *field, **KW, noises=noises, max_steps=MAX_STEPS,
                                                         T_thresh=T_thresh, return_stats=stats, **shade_kw)

            def composition():
                with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
                    xyzs, dirs, ts, rays = rm.march_rays_train(o, d, bound, bits, C, H, nears, fars, False, 0, MAX_STEPS, noises=noises)
                    if shading == "albedo":
                        sigmas, rgbs = nerf.nerf_field(xyzs, *field, **KW)
                    else:
                        sigmas, rgbs = shaded_composition(field, bound, xyzs, light, shading)
                    return rm.composite_rays_train(sigmas, rgbs, ts, rays, T_thresh)[1:]

            def step(path, backward):
                def fn():
                    for p in net.parameters():
                        p.grad = None
                    out = path()[:3]
                    if backward:
                        torch.autograd.backward(out, [g_ws, g_d, g_img])
                return fn
            with _limit(args.limit, "%d^2 %s set-up" % (W, level)):
                *out_n, st = native(stats=True)
                out_c = composition()
                same = all(torch.equal(a, b) for a, b in zip(out_n[:2] if shade_kw else out_n, out_c))
                image_diff = float((out_n[2] - out_c[2]).abs().max()) if N else 0.0
                live = st["live"]
                has = live[live > 0]
                live_med = float(has.float().median()) if has.numel() else 0.0
                del out_n, out_c
            paths = (("native", native), ("composition", composition))
            times = {(name, bw): [] for name, _ in paths for bw in (False, True)}
            for rep in range(args.reps + 1):                      # repetition 0 is the warm-up of every (path, mode)
                for bw in (False, True):
                    for name, path in paths:
                        with _limit(args.limit, "%d^2 %s %s" % (W, level, name)):
                            t = _event_ms(step(path, bw))
                        if rep:
                            times[(name, bw)].append(t)
            for name, path in paths:
                with _limit(args.limit, "%d^2 %s %s peak" % (W, level, name)):
                    peak = _peak(step(path, True))
                row = dict(rays=N, density=level, T_thresh=T_thresh, M=st["M"], M_live=st["M_live"],
                           culled=(st["M"] - st["M_live"]) / max(st["M"], 1), live_median=live_med, path=name, outputs_equal=same, shading=shading, image_max_diff=image_diff,
                           fwd_ms=_stats(times[(name, False)]), fwd_bwd_ms=_stats(times[(name, True)]), peak_bytes=peak)
                rows.append(row)

                def fmt(s):
                    return "%6.2f /%6.2f /%6.2f" % (s["min"], s["median"], s["max"])
                print("%-6s %-9s %10d %10d %7.3f %6.0f  %-11s %-22s %-22s %8.0f" % (
                    "%d^2" % W, level, row["M"], row["M_live"], row["culled"], live_med, name, fmt(row["fwd_ms"]), fmt(row["fwd_bwd_ms"]),
                    peak / 1e6), flush=True)
            n, c_ = rows[-2], rows[-1]
            print("       %-9s native / composition: fwd %.3f, fwd + bwd %.3f (medians); composition's own f+b spread %.2f ms; outputs %s"
                  % (level, n["fwd_ms"]["median"] / c_["fwd_ms"]["median"], n["fwd_bwd_ms"]["median"] / c_["fwd_bwd_ms"]["median"],
                     c_["fwd_bwd_ms"]["max"] - c_["fwd_bwd_ms"]["min"],
                     ("bit-equal" if same else "DIFFER") + (" (weights_sum, depth; image max |diff| %.2g)" % image_diff if shade_kw else "")), flush=True)
        del o, d, nears, fars, noises
        torch.cuda.empty_cache()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
