"""Times the NeRF stage's occupancy-grid update (boundary B13) on a synthetic grid-backbone field: the native update
(dreamwaltz_g_amd.occupancy.OccupancyGrid.update + the one stats() read) at grid_size 128 / bound 2 (the shipped recipe: two cascades of
2.1 M cells) and grid_size 64 / bound 1, in f16 (the trainer calls it under autocast) and f32.

    python tools/bench_occupancy.py [--sizes 128:2,64:1] [--reps 20] [--out profiles/b13_bench_occupancy.txt]

Beside it the composition that the binding ran before is timed on the same device in the same process, BEFORE and AFTER the native runs
(two figures, so that clock drift shows).  That side is a LABELLED TORCH RESTATEMENT (tests/occupancy_cases.OccNetwork.update_extra_state:
the reference's statements nerf_renderer.py:106-153 over the package's morton3D / packbits and the fused field kernel through the bound
common_forward) -- the reference's own module is not importable without its dependencies.  Both sides run the same field kernel on the
same points; the difference is the torch statements around it and what crosses to the host.  Host read-backs are counted, not estimated:
the native side does one (stats, 32 bytes), the composition three .item() calls and the masked gathers / scatter of the EMA (each boolean
mask index synchronises to size its result).  Times are wall-clock milliseconds around a synchronised call, the median of --reps calls
after one warm-up.  The last line is the table as JSON."""
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
from dreamwaltz_g_amd import nerf  # noqa: E402
from tests import occupancy_cases as occ  # noqa: E402


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
    return sum(1 for x in w if "synchroniz" in str(x.message))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128:2,64:1")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows, lines = [], []
    for size in a.sizes.split(","):
        H, bound = (int(v) for v in size.split(":"))
        nets = []
        for _ in range(2):
            net = occ.make_occ_network(H, bound=bound, gridtype='hash', interp='smoothstep', density_activation='exp', density_prior='gaussian').cuda()
            assert nerf.bind_nerf_network(net) is None
            nets.append(net)
        native, composed = nets
        del composed.__dict__["update_extra_state"]         # the class method over the bound field: the parent commit's path
        for f16 in (True, False):
            def run(net):
                with torch.autocast("cuda", dtype=torch.float16, enabled=f16):
                    net.update_extra_state()
            before = _median_ms(lambda: run(composed), a.reps)
            t_native = _median_ms(lambda: run(native), a.reps)
            after = _median_ms(lambda: run(composed), a.reps)
            row = {"grid_size": H, "bound": bound, "cascades": native.cascade, "cells": native.cascade * H ** 3, "precision": "f16" if f16 else "f32",
                   "native_ms": t_native, "composition_ms_before": before, "composition_ms_after": after,
                   "native_host_syncs": _count_syncs(lambda: run(native)), "composition_host_syncs": _count_syncs(lambda: run(composed))}
            rows.append(row)
            lines.append("H %4d  bound %d  cascades %d  cells %9d  %s  native %8.3f ms (%d host sync)  torch composition %8.3f / %8.3f ms (before / after, "
                         "%d host syncs)  x%.1f" % (H, bound, native.cascade, row["cells"], row["precision"], t_native, row["native_host_syncs"], before,
                                                    after, row["composition_host_syncs"], min(before, after) / t_native))
            print(lines[-1], flush=True)
        del nets, native, composed
        torch.cuda.empty_cache()
    text = "\n".join(["B13 occupancy-grid update, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__)] + lines + [json.dumps(rows)]) + "\n"
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write(text)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
