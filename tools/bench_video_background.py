"""Times animation playback at 512^2 with and without a video background (boundary B5, csrc/background.hip) on one GPU: frames/s of
eager Scene.forward_frames with F = 1 and F = 4 frames per launch chain, and of player.GraphedAnimation replays (one graph per frame).

    python tools/bench_video_background.py [--gaussians 100000] [--frames 120] [--repeats 3]

Cases: no background; a device-resident video of 512^2 frames (equal size: no resample); a 1080p video resampled to 512^2 in the
kernel; and a LABELLED STAND-IN for the reference's per-frame path (cv2 is not installed here, so cvtColor / resize cannot be timed):
a numpy channel swap of the 512^2 host frame, `torch.from_numpy(frame).float() / 255.0` on the host, a pageable copy to the device
and the three torch ops of scene.py:160, after the no-background frame.  Per case the best of --repeats runs of --frames frames, each
run closed by one synchronisation.  The last line is the whole table as JSON.
"""
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
from dreamwaltz_g_amd import camera, configs, player, scene as sc, sds_step, synth  # noqa: E402
from dreamwaltz_g_amd.background import VideoBackground  # noqa: E402

RES = 512


def _fps(run, frames, repeats):
    run(min(frames, 8))
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(frames)
        torch.cuda.synchronize()
        best = max(best, frames / (time.perf_counter() - t0))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = configs.TrainConfig(); cfg.device = str(dev); cfg.render.bg_color = (0.5, 0.5, 0.5)
    avatar, _, _ = sds_step.build_synthetic_avatar(a.gaussians, dev, seed=0)
    data = camera.make_camera(radius=2.0, azimuth=20.0, elevation=80.0, fovy=55.0, height=RES, width=RES, device=dev)
    T = 32
    poses = [synth.random_smpl_inputs(seed=i, device=dev) for i in range(T)]
    rng = np.random.RandomState(0)
    src = {"none": None, "video_512": rng.randint(0, 256, (T, RES, RES, 3)).astype(np.uint8),
           "video_1080p_resampled": rng.randint(0, 256, (T, 1080, 1920, 3)).astype(np.uint8)}
    host_512 = src["video_512"]
    rows = []
    for name in ("none", "video_512", "video_1080p_resampled", "reference_style_STAND_IN"):
        frames = src.get(name)
        bg = VideoBackground.from_frames(frames, fps=30) if frames is not None else None
        scene = sc.Scene(cfg, avatar, background=bg, async_pair_count=True).to(dev).eval()
        stand_in = name == "reference_style_STAND_IN"

        def host_composite(out, i):
            rgb = np.ascontiguousarray(host_512[i % T][..., ::-1])                     # stand-in for cv2.cvtColor(BGR2RGB)
            bgt = (torch.from_numpy(rgb).float() / 255.0).to(out['image'])             # host division, pageable copy
            out['image_bg'], out['image_fg'] = bgt, out['image']
            out['image'] = out['image'] + bgt * (1 - out['alpha'])
            return out

        def eager(F):
            def run(n):
                with torch.inference_mode():
                    for s in range(0, n, F):
                        ps = [poses[(s + f) % T] for f in range(F)]
                        idx = [(s + f) % T for f in range(F)]
                        out = scene.forward_frames(data, ps, frame_indices=idx if bg is not None else None)
                        if stand_in:
                            for f in range(F):
                                host_composite({k: v[f:f + 1] for k, v in out.items()}, s + f)
            return run
        row = {"case": name, "render": RES, "gaussians": a.gaussians}
        for F in (1, 4):
            row["eager_F%d_fps" % F] = round(_fps(eager(F), a.frames, a.repeats), 1)
        pl = player.GraphedAnimation(scene, data, poses[0], warmup_poses=poses[:3], frame_index=0 if bg is not None else None)

        def replay(n):
            for i in range(n):
                out = pl.replay(poses[i % T], frame_index=(i % T) if bg is not None else None)
                if stand_in:
                    host_composite(dict(out), i)
        row["graph_replay_fps"] = round(_fps(replay, a.frames, a.repeats), 1)
        pl.close()
        rows.append(row)
        print("%-24s eager F=1 %8.1f  eager F=4 %8.1f  graph replay %8.1f  frames/s" % (name, row["eager_F1_fps"], row["eager_F4_fps"],
                                                                                     row["graph_replay_fps"]), flush=True)
        del scene, bg
    base = rows[0]
    for r in rows[1:]:
        r["vs_none"] = {k: round(r[k] / base[k], 3) for k in ("eager_F1_fps", "eager_F4_fps", "graph_replay_fps")}
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
