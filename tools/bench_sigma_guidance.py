"""Times the NeRF stage's SMPL-X sigma guidance (boundary B8) at the recipe's point counts: the device geometry alone (part preparation,
sample, point-to-mesh distance, keep mask) and the whole calc_sigma_loss with the B7-bound field's forward and backward, for
N in {5 000, 20 908} against a part of ~2 k faces and a full-body-sized part of 20 480 faces (icosphere level 5).

    python tools/bench_sigma_guidance.py [--reps 20] [--cpu-reps 1]

As a LABELLED STAND-IN for the reference's trimesh + igl (not installed here, so their own time cannot be measured), the float64
restatement of tests/sigma_guidance_cases.py is timed on the CPU for the same geometry (brute-force numpy-style distance in torch
float64; N = 5 000 only).  Per case: median ms of CUDA events over --reps calls (each call synchronised on its own), and per-kernel times of one call
from the library's own launch profiler.  The last line is the whole table as JSON.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import _lib  # noqa: E402
from dreamwaltz_g_amd import sigma_guidance as sg  # noqa: E402
from dreamwaltz_g_amd.nerf import bind_nerf_network  # noqa: E402
from tests import nerf_field_cases as nc  # noqa: E402
from tests import sigma_guidance_cases as sc  # noqa: E402


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
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


class _SMPL:
    def __init__(self, faces, part, wrist):
        self.model = types.SimpleNamespace(faces=faces)
        self.part, self.wrist = part, wrist

    def get_semantic_indices(self, select_parts):
        return None, list(self.wrist) if list(select_parts) == ['wrists'] else list(self.part)


def _cpu_restatement(V, F, draws, thick):
    t0 = time.perf_counter()
    pts, fid, pn, noisy = sc.sample(V, F, draws, 0.05)
    D = sc.all_face_distances(noisy, V, F, chunk=64)
    dmin, imin = D.min(dim=1)
    keep = sc.keep_mask(dmin ** 2, imin, thick)
    return (time.perf_counter() - t0) * 1e3, int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    V, F = sc.make_icosphere(5)
    cz = V[F].mean(axis=1)[:, 2]
    parts = {"part_2k": np.nonzero(cz > 0.8)[0], "body_20480": np.arange(len(F))}
    wrist = np.nonzero((cz > 0.8) & (cz < 0.83))[0]
    Vt = torch.from_numpy(V).cuda()
    net = nc.make_network(seed=0).cuda()
    assert bind_nerf_network(net) is None
    rows = []
    print("# MI355X, B8 sigma guidance; times in ms (median, [p10, p90]) of %d calls" % args.reps)
    for pname, pf in parts.items():
        for n in (5000, 20908):
            part = sg.PartMesh(F[pf], len(V), "cuda", wrist=np.isin(pf, wrist))
            g = torch.Generator(device="cuda").manual_seed(0)

            def geometry():
                draws = torch.rand((n, 4), dtype=torch.float64, device="cuda", generator=g)
                return sg.guidance_points(Vt, part, draws, 0.05, 0.005)
            geo = _time(geometry, args.reps)
            rec, _, _ = sg._prepare(Vt, part)
            noisy = geometry()['noisy']
            dist = _time(lambda: sg._distance(noisy, rec, closest_point=False), args.reps)
            cfg = types.SimpleNamespace(sigma_loss_type='margin', sigma_noise_range=0.05, sigma_num_points=n, sigma_surface_thickness=0.005,
                                        sigma_guidance_peak=15.0, sigma_guidance_delta=0.2, lambda_sigma_sigma=1.0, lambda_sigma_albedo=0.0,
                                        lambda_sigma_normal=0.0)
            tr = types.SimpleNamespace(cfg=cfg, smpl_model=_SMPL(F, pf, wrist), model=net, losses={}, time_to_snapshot=False)
            data = {'smpl_outputs': types.SimpleNamespace(vertices=Vt[None])}
            sd = torch.zeros(1, device="cuda")

            def whole():
                with torch.autocast("cuda", dtype=torch.float16):
                    losses = sg.calc_sigma_loss(tr, data, {}, sd, ['part'], generator=g)
                losses['sigma_loss'].backward()
            full = _time(whole, args.reps)
            _lib.prof_enable(True)
            geometry()
            torch.cuda.synchronize()
            kern = {k: round(v[1], 4) for k, v in _lib.prof_table().items() if k.startswith("sigma_")}
            _lib.prof_enable(False)
            tests = n * len(pf)
            row = {"part": pname, "faces": int(len(pf)), "N": n, "geometry_ms": geo, "distance_ms": dist, "calc_sigma_loss_fwd_bwd_f16_ms": full,
                   "kernels_ms": kern, "point_triangle_tests": tests, "tests_per_ns": round(tests / (dist[0] * 1e6), 1)}
            if not args.no_cpu and n == 5000:
                draws = torch.rand((n, 4), dtype=torch.float64)
                cpu = [_cpu_restatement(torch.from_numpy(V).double(), torch.from_numpy(F[pf]), draws, 0.005)[0] for _ in range(args.cpu_reps)]
                row["cpu_float64_restatement_ms_STAND_IN"] = float(np.median(cpu))
            rows.append(row)
            print("%-10s F=%5d N=%5d  geometry %.3f [%.3f, %.3f]  distance %.3f  calc_sigma_loss f16 fwd+bwd %.3f  %s%s" % (
                pname, len(pf), n, geo[0], geo[1], geo[2], dist[0], full[0], kern,
                "" if "cpu_float64_restatement_ms_STAND_IN" not in row else "  | CPU float64 restatement (stand-in for trimesh + igl) %.0f" % row["cpu_float64_restatement_ms_STAND_IN"]),
                flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
