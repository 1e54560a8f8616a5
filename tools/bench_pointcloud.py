"""Times the NeRF-to-Gaussian point-cloud export (boundary B12) on a synthetic grid-backbone field: the native export
(dreamwaltz_g_amd.pointcloud.export_point_cloud) at resolution 256 / split 256 and resolution 400 / split 256 (the reference's shipped
default, core/trainer.py:549).

    python tools/bench_pointcloud.py [--sizes 256,400] [--split 256] [--keep 0.03] [--reps 3] [--out profiles/b12_bench_pointcloud.txt]

Beside it the reference's statements are timed on the same device in the same process, BEFORE and AFTER the native runs (two figures, so
that clock drift shows).  That side is a LABELLED TORCH RESTATEMENT (tests/pointcloud_cases.restate_export over the test-local network bound
with nerf.bind_nerf_network): the chunk loop, seven evaluations of the fused field kernel for every lattice point, latent_to_rgb,
safe_normalize, the mask, and the four host copies with their numpy concatenations per chunk -- the reference's own module is not
importable without its dependencies.  Both sides therefore run the same field kernel; the difference is how often, and what crosses to
the host.  The threshold is the (1 - keep) quantile of the lattice density, so that the share `keep` of the lattice survives.
Times are wall-clock milliseconds around a synchronised call (the export contains its own read-back); the native figure is the median of
--reps calls after one warm-up, the restatement one call each time.  The last line is the table as JSON."""
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
from dreamwaltz_g_amd import nerf, pointcloud as pc  # noqa: E402
from tests import nerf_field_cases as nc  # noqa: E402
from tests import pointcloud_cases as pcc  # noqa: E402


def _wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def restatement(net, R, split, thr):
    """The reference's loop with its host side: per chunk four .cpu().numpy() copies and four concatenations into float64 arrays."""
    arrays = {k: np.empty((0, 1 if k == "alphas" else 3)) for k in ("points", "colors", "alphas", "normals")}
    for xs in torch.linspace(-1, 1, R).split(split):
        for ys in torch.linspace(-1, 1, R).split(split):
            for zs in torch.linspace(-1, 1, R).split(split):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing='ij')
                pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).cuda()
                sigmas, albedos = net.common_forward(pts)
                sigmas = sigmas.reshape(-1, 1)
                albedos = pcc.latent_to_rgb(albedos)
                normals = pcc.normal(net, pts)
                sigmas.min().item(), sigmas.max().item()
                valid = (sigmas > thr).flatten()
                for k, v in (("points", pts), ("colors", albedos), ("alphas", sigmas), ("normals", normals)):
                    arrays[k] = np.concatenate((arrays[k], v[valid].cpu().numpy()), axis=0)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,400")
    ap.add_argument("--split", type=int, default=256)
    ap.add_argument("--keep", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    net = nc.make_network(gridtype='hash', interp='smoothstep', density_activation='exp', density_prior='gaussian', seed=3).cuda()
    assert nerf.bind_nerf_network(net) is None
    field = pc.field_spec(net.encoder, net.sigma_net, net.sigma_scale, net.bound, 'exp', 'gaussian', True, 0)
    rows, lines = [], []
    with torch.inference_mode():
        for R in (int(s) for s in a.sizes.split(",")):
            ax = pc.axis_table(R, "cuda")
            sigma, _ = pc.lattice_sigma(*field, ax, ax, ax, min(a.split, R))
            sample = sigma[torch.randperm(sigma.numel(), device="cuda")[:1 << 20]]
            thr = float(torch.quantile(sample, 1.0 - a.keep))
            del sigma, sample
            export = lambda: pc.export_point_cloud(net.encoder, net.sigma_net, net.sigma_scale, net.bound, resolution=R, split_size=a.split,      # noqa: E731
                                                   density_thresh=thr, density_activation='exp', density_prior='gaussian', precision=0)
            before, ref = _wall_ms(lambda: restatement(net, R, a.split, thr))
            export()
            ts = []
            for _ in range(a.reps):
                t, cloud = _wall_ms(export)
                ts.append(t)
            t_basic, basic = _wall_ms(cloud.to_basic)
            after, _ = _wall_ms(lambda: restatement(net, R, a.split, thr))
            same = (len(basic) == len(ref["points"]) and np.array_equal(basic.points, ref["points"]) and np.array_equal(basic.alphas, ref["alphas"])
                    and np.array_equal(basic.colors, ref["colors"]))
            row = {"resolution": R, "split": a.split, "lattice": R ** 3, "survivors": len(cloud), "native_ms": float(np.median(ts)),
                   "to_basic_ms": t_basic, "torch_restatement_ms_before": before, "torch_restatement_ms_after": after,
                   "same_points_alphas_colors": bool(same)}
            rows.append(row)
            lines.append("R %4d  split %3d  lattice %9d  survivors %8d (%.2f %%)  native %9.1f ms  (+ to_basic %7.1f ms)  torch restatement %9.1f / %9.1f ms "
                         "(before / after)  x%.1f  same cloud: %s" % (R, a.split, R ** 3, len(cloud), 100.0 * len(cloud) / R ** 3, row["native_ms"], t_basic,
                                                                      before, after, min(before, after) / (row["native_ms"] + t_basic), same))
            print(lines[-1], flush=True)
            del cloud, basic, ref
    text = "\n".join(["B12 point-cloud export, %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__)] + lines + [json.dumps(rows)]) + "\n"
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write(text)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
