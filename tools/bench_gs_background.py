"""Times playback of one avatar inside a static 3D-Gaussian scene (boundary B24, csrc/scene_gaussians.hip) on one GPU: a 300 k-Gaussian
synthetic avatar at 1024^2 in synthetic scenes of 10^5, 10^6 and 3 10^6 random Gaussians in a room-sized box.

    python tools/bench_gs_background.py [--gaussians 300000] [--scenes 100000,1000000,3000000] [--frames 48] [--repeats 3] [--res 1024]

Per scene size:
  activation_ms            dwg_scene_gaussians_activate, once per parameter change
  merge_ms                 dwg_scene_merge per frame at sh_levels = 1: avatar rows + scene rows, 112 B moved per Gaussian; merge_GBps from
                           those bytes, merge_share_of_hbm_spec against the 8 TB/s specification
                           Both are DEVICE times: 20 calls captured into one graph, the replay timed by device events (median of
                           --repeats) -- the Python wrapper alone costs about as much as the launch at the small sizes; *_call_ms is
                           the same call issued eagerly, host included
  merge_sh4_ms             the same launch at sh_levels = 4 (192 B more read per scene row, the colour evaluated in the launch)
  TORCH_REFERENCE_composition_ms   a LABELLED restatement of the reference's per-frame composition on torch, timed in the same run in
                           alternation with the merge: GaussianModel.forward() (sigmoid, exp, F.normalize, the 48-float cat of the SH tensor),
                           compute_colors(sh_levels=1) and merge_gaussians' torch.cat per attribute (scene.py:123-132)
  eager_F1_fps, eager_F4_fps       Scene.forward_frames with 1 and 4 frames per launch chain
  TORCH_REFERENCE_eager_F1_fps     the torch composition in front of the same rasterizer (renderer.render_frames of one frame)
  graph_replay_fps         player.GraphedAnimation replays
  pairs / overflow         what the rasterizer chain reports for one frame: block pairs after culling, the reference's tile-pair count, and
                           whether the frame overflowed its pair buffers (the chain was tuned for <= 3 10^5 Gaussians)
With --cull (boundary B25, csrc/scene_cull.hip: the scene culled once per camera) the columns above stay as they are and these are added:
  kept_gaussians, kept_share       the scene Gaussians GaussianBackground.culled keeps for the benchmark's camera
  cull_ms                  device time of flags + compaction + gather (the three C entries on preallocated buffers, 20 calls in one
                           graph, event-timed, median of 3): what a cache miss costs on the device; a miss also reads the count back once
  merge_culled_ms          dwg_scene_merge per frame over the culled block (as merge_ms)
  cull_rounds              eager F = 1 and eager F = 4 in frames/s with culling off and on, ALTERNATED in this process, three rounds:
                           {column: [round 1, 2, 3]}; *_fps_cull_off / *_fps_cull_on are the medians and *_spread the largest max - min
                           of the two (GraphedAnimation does not cull: graph_replay_fps above is the only replay figure)
The last line is the whole table as JSON.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import camera, configs, player, scene as sc, sds_step, synth  # noqa: E402
from dreamwaltz_g_amd.avatar import GaussianOutput, merge_gaussians  # noqa: E402
from dreamwaltz_g_amd.background import GaussianBackground, scene_merge  # noqa: E402

HBM_SPEC_BYTES_PER_S = 8.0e12
BYTES_PER_GAUSSIAN = 112          # 28 floats read and 28 written


def room(n, seed, device):
    """n random Gaussians in an 8 x 3 x 8 m box around the avatar: 1-3 cm across, mostly opaque."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)           # noqa: E731
    pos = (u(n, 3) * 2 - 1) * torch.tensor([4.0, 1.5, 4.0])
    arrays = dict(positions=pos, sh_features_dc=u(n, 1, 3) * 3 - 1.5, sh_features_rest=(u(n, 15, 3) - 0.5) * 0.4, opacities=u(n, 1) * 6 - 1,
                  scales=u(n, 3) * 1.1 - 5.0, quaternions=torch.randn(n, 4, generator=g))
    return {k: v.to(device) for k, v in arrays.items()}


def events_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def graph_ms(fn, iters=20):
    """Device time per call: `iters` calls captured into one graph, one replay timed by events (no host work between the launches)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(iters):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    ms = events_ms(g.replay, 1) / iters
    del g
    return ms


def fps(run, frames, repeats):
    run(min(frames, 8))
    torch.cuda.synchronize()
    best = 0.0
    for _ in range(repeats):
        t0 = time.perf_counter()
        run(frames)
        torch.cuda.synchronize()
        best = max(best, frames / (time.perf_counter() - t0))
    return best


def torch_reference_composition(avatar_out, bg, data, renderer):
    """scene.py:123-132 on torch: what the reference runs per frame for its Gaussian background."""
    scene = GaussianOutput(positions=bg._positions, sh_features=torch.cat((bg._sh_features_dc, bg._sh_features_rest), dim=1),
                           opacities=torch.sigmoid(bg._opacities.view(-1, 1)), quaternions=torch.nn.functional.normalize(bg._quaternions),
                           scales=torch.exp(bg._scales))
    scene.colors = renderer.compute_colors(sh_features=scene.sh_features, positions=scene.positions, camera_positions=data['c2w'][:, :3, 3],
                                           sh_levels=1)
    scene.sh_features = None
    return merge_gaussians(avatar_out, scene)


def cull_columns(scene, bg, data, poses, part, a, dev):
    """The --cull columns of one scene size (see the module docstring)."""
    from dreamwaltz_g_amd import _lib
    from dreamwaltz_g_amd.background import CULL_CAMERA_FLOATS, CULL_MAX_ROWS, CullRowsC, _cull_camera_blocks
    row, n, T, L = {}, bg.n_points, len(poses), _lib.lib()
    with torch.inference_mode():
        culled = bg.culled(data, a.res, a.res)
        kept = culled.n_points
        row["kept_gaussians"], row["kept_share"] = kept, round(kept / max(n, 1), 4)
        block, cams = bg.activated(), _cull_camera_blocks(data, dev)
        flags, index = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        work = torch.empty(max(int(L.dwg_scene_cull_workspace_bytes(n)), 4), dtype=torch.uint8, device=dev)
        src = [bg._positions, block['opacities'], block['scales'], block['quaternions'], block['colors']]
        dst = [torch.empty((kept,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for t in src]
        tables = (CullRowsC * CULL_MAX_ROWS)()
        for r, s, d in zip(tables, src, dst):
            r.src, r.dst, r.width = s.data_ptr(), d.data_ptr(), s[0].numel()
        st = _lib.stream

        def cull_kernels():
            _lib.check(L.dwg_scene_cull_flags(n, _lib.ptr(bg._positions), _lib.ptr(block['scales']), 1, _lib.ptr(cams), CULL_CAMERA_FLOATS, a.res,
                                              a.res, _lib.ptr(flags), st(dev)), "dwg_scene_cull_flags")
            _lib.check(L.dwg_scene_cull_compact(n, _lib.ptr(flags), _lib.ptr(index), _lib.ptr(count), _lib.ptr(work), st(dev)), "dwg_scene_cull_compact")
            _lib.check(L.dwg_scene_cull_gather(kept, _lib.ptr(index), n, len(src), tables, st(dev)), "dwg_scene_cull_gather")
        cull_kernels()
        assert int(count.item()) == kept and torch.equal(dst[0], culled._positions) and torch.equal(dst[4], culled.activated()['colors'])
        row["cull_ms"] = round(statistics.median(graph_ms(cull_kernels) for _ in range(3)), 4)
        out = tuple(torch.empty((int(part.positions.shape[0]) + kept, w), dtype=torch.float32, device=dev) for w in (3, 1, 3, 3, 4))
        cam = data['c2w'][:, :3, 3]
        merge = lambda: scene_merge([part], culled, cam, out=out)                                  # noqa: E731
        merge()
        row["merge_culled_ms"] = round(statistics.median(graph_ms(merge) for _ in range(3)), 4)
        del out, dst, flags, index, work

    def eager(F, cull):
        def run(k):
            with torch.inference_mode():
                for s in range(0, k, F):
                    scene.forward_frames(data, [poses[(s + f) % T] for f in range(F)], cull_scene=cull)
        return run
    rounds = {}
    for _ in range(3):                                                                              # off and on alternate on the same box
        for cull, tag in ((False, "off"), (True, "on")):
            for F in (1, 4):
                rounds.setdefault("eager_F%d_fps_cull_%s" % (F, tag), []).append(round(fps(eager(F, cull), a.frames, a.repeats), 1))
    row["cull_rounds"] = rounds
    for k, v in rounds.items():
        row[k] = statistics.median(v)
    for what in ("eager_F1_fps", "eager_F4_fps"):
        row[what + "_cull_spread"] = round(max(max(rounds[what + "_cull_" + t]) - min(rounds[what + "_cull_" + t]) for t in ("off", "on")), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=300000)
    ap.add_argument("--scenes", default="100000,1000000,3000000")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--cull", action="store_true", help="add the columns of the per-camera scene cull (B25): culling off and on, alternated")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = configs.TrainConfig(); cfg.device = str(dev); cfg.render.bg_color = (0.5, 0.5, 0.5)
    avatar, _, _ = sds_step.build_synthetic_avatar(a.gaussians, dev, seed=0)
    data = camera.make_camera(radius=2.4, azimuth=20.0, elevation=80.0, fovy=55.0, height=a.res, width=a.res, device=dev)
    T = 16
    poses = [synth.random_smpl_inputs(seed=i, device=dev) for i in range(T)]
    rows = []
    for n in [int(s) for s in a.scenes.split(",")]:
        arrays = room(n, seed=n, device=dev)
        bg = GaussianBackground.from_tensors(**arrays)
        bg4 = GaussianBackground.from_tensors(**arrays, sh_levels=4)
        scene = sc.Scene(cfg, avatar, background=bg, async_pair_count=True).to(dev).eval()
        row = {"scene_gaussians": n, "avatar_gaussians": a.gaussians, "render": a.res}
        with torch.inference_mode():
            part = scene.avatar_forward(smpl_observed_inputs=poses[0])
            total = int(part.positions.shape[0]) + n
            cam = data['c2w'][:, :3, 3]

            def activate():
                bg.invalidate_caches()
                bg.activated()
            activate(); bg4.activated()
            out = tuple(torch.empty((total, w), dtype=torch.float32, device=dev) for w in (3, 1, 3, 3, 4))
            native = lambda: scene_merge([part], bg, cam, out=out)                          # noqa: E731
            native4 = lambda: scene_merge([part], bg4, cam, out=out)                        # noqa: E731
            reference = lambda: torch_reference_composition(part, bg, data, scene.renderer)  # noqa: E731
            for f in (native, native4, reference):
                f()
            torch.cuda.synchronize()
            row["activation_ms"] = round(statistics.median(graph_ms(activate, 5) for _ in range(max(a.repeats, 3))), 4)
            t_nat, t_ref, t_nat4, c_nat, c_ref = [], [], [], [], []
            for _ in range(max(a.repeats, 3)):                                              # alternating runs on the same box
                t_nat.append(graph_ms(native)); t_ref.append(graph_ms(reference)); t_nat4.append(graph_ms(native4))
                c_nat.append(events_ms(native, 20)); c_ref.append(events_ms(reference, 20))
            row["merge_ms"], row["merge_sh4_ms"] = round(statistics.median(t_nat), 4), round(statistics.median(t_nat4), 4)
            row["TORCH_REFERENCE_composition_ms"] = round(statistics.median(t_ref), 4)
            row["merge_call_ms"], row["TORCH_REFERENCE_composition_call_ms"] = round(statistics.median(c_nat), 4), round(statistics.median(c_ref), 4)
            row["merge_GBps"] = round(BYTES_PER_GAUSSIAN * total / (row["merge_ms"] * 1e-3) / 1e9, 1)
            row["merge_share_of_hbm_spec"] = round(BYTES_PER_GAUSSIAN * total / (row["merge_ms"] * 1e-3) / HBM_SPEC_BYTES_PER_S, 3)
            row["merge_sh4_GBps"] = round((BYTES_PER_GAUSSIAN * total + 192 * n) / (row["merge_sh4_ms"] * 1e-3) / 1e9, 1)
            del out

        def eager(F):
            def run(k):
                with torch.inference_mode():
                    for s in range(0, k, F):
                        scene.forward_frames(data, [poses[(s + f) % T] for f in range(F)])
            return run

        def torch_eager(k):
            with torch.inference_mode():
                for s in range(k):
                    g = torch_reference_composition(scene.avatar_forward(smpl_observed_inputs=poses[s % T]), bg, data, scene.renderer)
                    scene.renderer.render_frames(data=data, frames=[g])
        for F in (1, 4):
            row["eager_F%d_fps" % F] = round(fps(eager(F), a.frames, a.repeats), 1)
        with torch.inference_mode():
            scene.forward_frames(data, [poses[0]])
            h = scene.renderer.last_frames_headers[0].tolist()                 # block pairs, overflow, reference tile pairs, segments
        row["block_pairs"], row["overflow"], row["reference_tile_pairs"], row["segments"] = int(h[0]), int(h[1]), int(h[2]), int(h[3])
        row["TORCH_REFERENCE_eager_F1_fps"] = round(fps(torch_eager, a.frames, a.repeats), 1)
        pl = player.GraphedAnimation(scene, data, poses[0], warmup_poses=poses[:3])
        row["graph_replay_fps"] = round(fps(lambda k: [pl.replay(poses[i % T]) for i in range(k)], a.frames, a.repeats), 1)
        row["graph_replay_complete"] = bool(pl.check())
        pl.close()
        if a.cull:
            row.update(cull_columns(scene, bg, data, poses, part, a, dev))
        rows.append(row)
        print("scene %8d  activation %7.3f ms  merge %7.3f ms (%6.1f GB/s, %4.1f %% of 8 TB/s)  sh4 merge %7.3f ms  TORCH REFERENCE composition "
              "%7.3f ms" % (n, row["activation_ms"], row["merge_ms"], row["merge_GBps"], 100 * row["merge_share_of_hbm_spec"], row["merge_sh4_ms"],
                            row["TORCH_REFERENCE_composition_ms"]), flush=True)
        print("               eager calls, host included: merge %7.3f ms, TORCH REFERENCE composition %7.3f ms"
              % (row["merge_call_ms"], row["TORCH_REFERENCE_composition_call_ms"]), flush=True)
        print("               eager F=1 %7.1f  F=4 %7.1f  graph replay %7.1f (complete: %s)  TORCH REFERENCE composition + same rasterizer F=1 "
              "%7.1f frames/s" % (row["eager_F1_fps"], row["eager_F4_fps"], row["graph_replay_fps"], row["graph_replay_complete"],
                                  row["TORCH_REFERENCE_eager_F1_fps"]), flush=True)
        print("               rasterizer, one frame: block pairs %d, reference tile pairs %d, segments %d, overflow flag %d"
              % (row["block_pairs"], row["reference_tile_pairs"], row["segments"], row["overflow"]), flush=True)
        if a.cull:
            print("               cull: kept %d (%.1f %%)  flags + compaction + gather %7.3f ms  merge over the culled block %7.3f ms"
                  % (row["kept_gaussians"], 100 * row["kept_share"], row["cull_ms"], row["merge_culled_ms"]), flush=True)
            for what in ("eager_F1_fps", "eager_F4_fps"):
                print("               %-16s cull off %s  on %s frames/s (three alternating rounds; spread %.1f)"
                      % (what, row["cull_rounds"][what + "_cull_off"], row["cull_rounds"][what + "_cull_on"], row[what + "_cull_spread"]), flush=True)
        del scene, bg, bg4, arrays
        torch.cuda.empty_cache()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
