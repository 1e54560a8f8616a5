"""Times the several-people pose condition image (boundary B16: dwg_condition_keypoints_people + dwg_condition_draw_people) at the recipe's
size: `export_pose_chw` at 512 x 512 against P = 1, 2, 4 closed meshes of the body's triangle count (20 908 each), and, for P = 1, the
same image through the existing one-person pair (dwg_condition_keypoints + dwg_condition_draw) in the same process.

    python tools/bench_condition_people.py [--reps 200] [--windows 7] [--out profiles/b16_bench_condition_people.txt]

The meshes are LABELLED STAND-INS for posed SMPL-X bodies (no body model ships with the repository): the ellipsoid of tests/depthmap_ref.py
(radii 0.25 / 0.8 / 0.15 m, 146 x 72 quads) cut to its first 20 908 triangles, person p moved 0.55 m further along x and 0.1 m along z, seen
by the golden `front` camera; 128 keypoints per person on and slightly off its surface.  Per case: microseconds per call, the median over
--windows event-timed windows of --reps back-to-back calls each, with the fastest and slowest window, per-kernel times (mean of five calls)
from the library's own launch profiler, and how many keypoints the culling removed.  There is no open3d and no OpenCV here, so the reference's
own time cannot be measured; nothing is compared with it.  The last line is the whole table as JSON; the same text goes to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import _lib, condition as cd, configs  # noqa: E402
from tests import depthmap_ref as dr  # noqa: E402

BODY_TRIANGLES = 20908
STEP = np.array([0.55, 0.0, 0.1], dtype=np.float32)


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


def _kernels_us(fn, prefixes, calls=5):
    """Per-kernel mean over `calls` profiled calls; one profiled call is thrown away first (the process's first profiled launch pays for the
    profiler's own set-up)."""
    fn()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    _lib.prof_enable(True)                                                  # starts the table again
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = {k: round(v[1] * 1e3 / max(v[0], 1), 2) for k, v in _lib.prof_table().items() if k.startswith(prefixes)}
    _lib.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "b16_bench_condition_people.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    v, t = dr.ellipsoid(146, 72)
    t = t[:BODY_TRIANGLES]
    g = np.random.default_rng(0)
    kp = (v[g.integers(0, v.shape[0], 128)] * (1.0 + g.uniform(0, 0.2, (128, 1)))).astype(np.float32)
    tris = torch.from_numpy(t).cuda()
    E, K = dr.camera("front", 512, 512)
    cam = dict(extrinsic=torch.from_numpy(E).cuda(), intrinsics=torch.from_numpy(K).cuda(), width=512, height=512)
    cfg = configs.PromptConfig()                                            # shipped defaults: body + hands, body SELF occlusion ignored
    cond = cd.SMPL2Condition(cfg)
    say("# MI355X, B16 several-people pose condition; export_pose_chw at 512 x 512, %d triangles per person; microseconds per call "
        "(median [fastest, slowest] of %d windows of %d calls)" % (t.shape[0], args.windows, args.reps))
    rows = []
    for P in (1, 2, 4):
        off = (np.arange(P, dtype=np.float32)[:, None] * STEP[None])[:, None, :]
        verts = torch.from_numpy((v[None] + off).astype(np.float32)).cuda()
        kps = torch.from_numpy((kp[None] + off).astype(np.float32)).cuda()
        scene = cd.build_people_scene(verts, tris)
        valid = int((cond.pose_rows(kps, scene, cam["extrinsic"], cam["intrinsics"])[..., 3] > 0.5).sum())
        row = {"people": P, "triangle_tests": P * P * 128 * int(t.shape[0]), "keypoints_drawn": valid, "keypoints": P * 128,
               "people_path_us": _time_us(lambda: cond.export_pose_chw(kps, scene, **cam), args.reps, args.windows),
               "people_kernels_us": _kernels_us(lambda: cond.export_pose_chw(kps, scene, **cam), ("cond_",))}
        line = "P = %d  fp64 triangle tests %.1f M  keypoints drawn %d / %d  people path %s  kernels %s" % (
            P, row["triangle_tests"] / 1e6, valid, P * 128, row["people_path_us"], row["people_kernels_us"])
        if P == 1:
            one = cd.build_ray_casting_scene(verts[0], tris)
            row["single_path_us"] = _time_us(lambda: cond.export_pose_chw(kps[0], one, **cam), args.reps, args.windows)
            row["single_kernels_us"] = _kernels_us(lambda: cond.export_pose_chw(kps[0], one, **cam), ("cond_",))
            row["people_over_single"] = round(row["people_path_us"][0] / row["single_path_us"][0], 3)
            same = torch.equal(cond.export_pose_chw(kps, scene, **cam), cond.export_pose_chw(kps[0], one, **cam))
            line += "\n       one-person path %s  kernels %s  people / one-person %.3f  same image: %s" % (
                row["single_path_us"], row["single_kernels_us"], row["people_over_single"], same)
        rows.append(row)
        say(line)
    say(json.dumps(rows))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
