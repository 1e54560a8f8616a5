"""Times the SMPL-X depth-map condition and the pretrain loss (boundary B9) at the recipe's sizes: 512 x 512 and 1024 x 1024 pixels against
a closed mesh of the body's triangle count (20 908), beside the existing pose-image pair (dwg_condition_keypoints + dwg_condition_draw)
on the same mesh at the same size, and the two loss calls at 512 x 512.

    python tools/bench_depth_condition.py [--reps 200] [--windows 7]

The mesh is a LABELLED STAND-IN for the posed SMPL-X body (no body model ships with the repository): the ellipsoid of
tests/depthmap_ref.py (radii 0.25 / 0.8 / 0.15 m, 146 x 72 quads) cut to its first 20 908 triangles, seen by the golden `front` camera.
Per case: microseconds per call, the median over --windows event-timed windows of --reps back-to-back calls each (so a window is
milliseconds of work, not one launch), with the fastest and slowest window, and per-kernel times of one call from the library's own
launch profiler.  There is no open3d here, so the reference's own time cannot be measured; nothing is compared.  The last line is
the whole table as JSON.
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
from dreamwaltz_g_amd import _lib, condition as cd, configs, pretrain  # noqa: E402
from tests import depthmap_ref as dr  # noqa: E402

BODY_TRIANGLES = 20908


def _time_us(fn, reps, windows):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return [round(float(np.median(ts)), 2), round(float(min(ts)), 2), round(float(max(ts)), 2)]


def _kernels_us(fn, prefixes):
    fn()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    out = {k: round(v[1] * 1e3 / max(v[0], 1), 2) for k, v in _lib.prof_table().items() if k.startswith(prefixes)}
    _lib.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    v, t = dr.ellipsoid(146, 72)
    t = t[:BODY_TRIANGLES]
    verts, tris = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
    scene = cd.build_ray_casting_scene(verts, tris)
    g = np.random.default_rng(0)
    kp = torch.from_numpy((v[g.integers(0, v.shape[0], 128)] * (1.0 + g.uniform(0, 0.2, (128, 1)))).astype(np.float32)).cuda()
    cfg = configs.PromptConfig()
    cfg.ignore_body_self_occlusion = False
    cond = cd.SMPL2Condition(cfg)
    rows = []
    print("# MI355X, B9 depth-map condition; microseconds per call (median [fastest, slowest] of %d windows of %d calls)" % (args.windows, args.reps))
    for size in (512, 1024):
        E, K = dr.camera("front", size, size)
        cam = dict(extrinsic=torch.from_numpy(E).cuda(), intrinsics=torch.from_numpy(K).cuda(), width=size, height=size)
        hits = int(torch.isfinite(cond.export_depth(scene, raw=True, **cam).t).sum())
        row = {"size": size, "triangles": int(t.shape[0]), "hit_pixels": hits,
               "depth_raw_us": _time_us(lambda: cond.export_depth(scene, raw=True, **cam), args.reps, args.windows),
               "depth_image_us": _time_us(lambda: cond.export_depth(scene, **cam), args.reps, args.windows),
               "depth_chw_us": _time_us(lambda: cond.export_depth_chw(scene, **cam), args.reps, args.windows),
               "normal_raw_us": _time_us(lambda: cond.export_normal_raw(scene, **cam), args.reps, args.windows),
               "pose_image_us": _time_us(lambda: cond.export_pose(kp, scene, **cam), args.reps, args.windows),
               "depth_kernels_us": _kernels_us(lambda: cond.export_depth(scene, **cam), ("depth_",)),
               "pose_kernels_us": _kernels_us(lambda: cond.export_pose(kp, scene, **cam), ("cond_",))}
        rows.append(row)
        print("%4d x %-4d F=%d hits=%d  depth_raw %s  depth image %s  depth chw %s  normals %s  | pose image (keypoints + draw) %s" % (
            size, size, t.shape[0], hits, row["depth_raw_us"], row["depth_image_us"], row["depth_chw_us"], row["normal_raw_us"], row["pose_image_us"]))
        print("            kernels: %s | %s" % (row["depth_kernels_us"], row["pose_kernels_us"]), flush=True)
    n = (1, 1, 512, 512)
    gen = torch.Generator(device="cuda").manual_seed(0)
    sd = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.3, 2.0 + torch.rand(n, device="cuda", generator=gen), torch.full(n, float("inf"), device="cuda"))
    for dtype in (torch.float32, torch.float16):
        depth = (torch.rand(n, device="cuda", generator=gen) * 3).to(dtype).requires_grad_(True)
        ws = torch.rand(n, device="cuda", generator=gen).to(dtype).requires_grad_(True)

        def fwd():
            return pretrain.depth_mask_loss(depth, ws, sd)

        def both():
            depth.grad = ws.grad = None
            fwd().backward()
        row = {"loss": str(dtype), "size": 512, "forward_us": _time_us(fwd, args.reps, args.windows),
               "forward_backward_autograd_us": _time_us(both, args.reps, args.windows), "kernels_us": _kernels_us(both, ("pretrain_",))}
        rows.append(row)
        print("loss 512 x 512 %-13s forward %s  forward + backward through autograd %s  kernels: %s" % (
            dtype, row["forward_us"], row["forward_backward_autograd_us"], row["kernels_us"]), flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
