"""Times the NeRF stage's inference render (boundary B14) on a synthetic grid-backbone field: the one-launch native render
(dreamwaltz_g_amd.nerf_render through the bound run_cuda) of a 512 x 512 and a 256 x 256 view at grid_size 128 / bound 2 (the shipped
recipe), in f16 (the trainer evaluates under autocast) and f32, with the evaluation defaults max_steps 1024 / T_thresh 1e-4.

    python tools/bench_nerf_render.py [--sizes 512,256] [--reps 20] [--composition-reps 5] [--out profiles/b14_bench_nerf_render.txt]
    python tools/bench_nerf_render.py --shading normal [...] [--out profiles/b15_bench_nerf_render.txt]

--shading normal (boundary B15) times the shaded view the trainer renders beside every albedo view: the network bound with
shaded_render=True against the composition of tests/nerf_shading_cases._NeRFNetwork.run_cuda (the reference's forward and normal over the
bound field: seven field launches per loop iteration).  ambient_ratio and light_d do not enter 'normal' shading.

The scene: a network with density_prior 'gaussian' and random parameters, its occupancy bitfield built by the native B13 update
(update_extra_state of the bound network).  Such a field is FOG, not a trained surface: outside the central blob the density is near 1,
about a third of the cells are occupied and most rays run to `far` with hundreds of samples -- the expensive end of what an evaluation
view costs.  The total number of composited samples is reported (counts.sum() of the native render).

Beside it the composition that the binding ran before is timed on the same device in the same process, BEFORE and AFTER the native runs
(two figures, so that clock drift shows).  That side is a LABELLED TORCH RESTATEMENT (tests/nerf_render_cases._NeRFNetwork.run_cuda: the
reference's statements nerf_renderer.py:311-402 over the package's march_rays / composite_rays and the fused field kernel through the
bound common_forward) -- the reference's own module is not importable without its dependencies.  Host synchronisations are counted, not
estimated (torch's sync debug mode).  Times are wall-clock milliseconds around a synchronised call, the median of --reps calls after one
warm-up (--composition-reps for the composition, whose single call takes seconds).  The last line is the table as JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import nerf, nerf_render, raymarch  # noqa: E402
from tests import nerf_render_cases as rc  # noqa: E402
from tests import nerf_shading_cases as sc  # noqa: E402
from tests import raymarch_cases as rmc  # noqa: E402


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def _count_syncs(fn):
    """Host synchronisations torch reports for one call (set_sync_debug_mode('warn') warns once per synchronising statement)."""
    import warnings
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    # torch's one-time notice that the debug mode is a prototype also speaks of "synchronizing operations": not a synchronisation
    return sum(1 for x in w if "synchroniz" in str(x.message) and "prototype feature" not in str(x.message))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,256")
    ap.add_argument("--grid", default="128:2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--composition-reps", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=1024)
    ap.add_argument("--shading", default="albedo", choices=["albedo", "normal"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    H, bound = (int(v) for v in a.grid.split(":"))
    nets = []
    for _ in range(2):
        make = rc.make_render_network if a.shading == "albedo" else sc.make_shading_network
        net = make(H, float(bound), gridtype='hash', interp='smoothstep').cuda().eval()
        assert nerf.bind_nerf_network(net, shaded_render=a.shading != "albedo") is None
        nets.append(net)
    native, composed = nets
    with torch.autocast("cuda", dtype=torch.float16):
        native.update_extra_state()                         # the B13 update: density_grid, mean_density, the bitfield
    with torch.no_grad():
        composed.density_bitfield.copy_(native.density_bitfield)
    del composed.__dict__["run_cuda"]                       # the class method over the bound field: the parent commit's path
    occupied = float(torch.sum(torch.tensor([bin(v).count("1") for v in range(256)], device="cuda")[native.density_bitfield.long()])) / (native.cascade * H ** 3)
    rows, lines = [], []
    for size in (int(v) for v in a.sizes.split(",")):
        o, d = rmc.make_cameras(1, size, size, seed=0)
        ro, rd = torch.from_numpy(np.ascontiguousarray(o)).cuda()[None], torch.from_numpy(np.ascontiguousarray(d)).cuda()[None]
        nears, fars = raymarch.near_far_from_aabb(ro[0], rd[0], native.aabb_infer)
        for f16 in (True, False):
            def run(net):
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=f16):
                    return net.run_cuda(ro, rd, light_d=ro[0, 0], shading=a.shading, max_steps=a.max_steps)
            before = _median_ms(lambda: run(composed), a.composition_reps)
            t_native = _median_ms(lambda: run(native), a.reps)
            after = _median_ms(lambda: run(composed), a.composition_reps)
            with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
                counts = nerf_render.render_rays(ro[0], rd[0], nears, fars, native.density_bitfield, native.cascade, H, native.encoder,
                                                 native.sigma_net, native.sigma_scale, native.bound, density_activation='exp',
                                                 density_prior='gaussian', albedo_sigmoid=True, max_steps=a.max_steps, return_counts=True)[3]
            a_out, b_out = run(native), run(composed)
            diff = float((a_out["image"] - b_out["image"]).abs().max())
            row = {"view": size, "rays": size * size, "grid_size": H, "bound": bound, "precision": "f16" if f16 else "f32", "max_steps": a.max_steps,
                   "occupied_share": occupied, "samples": int(counts.sum()), "max_count": int(counts.max()), "native_ms": t_native,
                   "composition_ms_before": before, "composition_ms_after": after, "native_host_syncs": _count_syncs(lambda: run(native)),
                   "composition_host_syncs": _count_syncs(lambda: run(composed)), "max_abs_image_diff": diff}
            rows.append(row)
            lines.append("view %4d^2  rays %7d  %s  samples %10d (max %4d per ray)  native %9.3f ms (%d host syncs)  torch composition %9.3f / %9.3f ms "
                         "(before / after, %d host syncs)  x%.1f  max |image diff| %.2g"
                         % (size, row["rays"], row["precision"], row["samples"], row["max_count"], t_native, row["native_host_syncs"], before, after,
                            row["composition_host_syncs"], min(before, after) / t_native, diff))
            print(lines[-1], flush=True)
    head = ("B14 inference render" if a.shading == "albedo" else "B15 inference render with shading '%s'" % a.shading) + ", %s, torch %s, grid_size %d bound %d (%.1f %% of the cells occupied), max_steps %d, reps %d / %d" % (
        torch.cuda.get_device_name(0), torch.__version__, H, bound, 100 * occupied, a.max_steps, a.reps, a.composition_reps)
    text = "\n".join([head] + lines + [json.dumps(rows)]) + "\n"
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write(text)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
