"""Times the avatar constructor's geometry (boundary B11) on a synthetic shell cloud around a synthetic body-sized mesh: nearest triangles,
the K + 1 nearest neighbours within the cloud, and the LBS-weight smoothing sweeps, at N = 100 000 and 300 000 points, K = 30, J = 55.

    python tools/bench_avatar_init.py [--sizes 100000,300000] [--sweeps 200] [--reps 3] [--out profiles/b11_bench_avatar_init.txt]

Beside each native stage the reference's torch statements are timed on the same device in the same process, BEFORE and AFTER the native
side (two figures, so that clock drift shows):
  sweeps   the loop body of LBSUtils.initialize_lbs_weights as it reads (einsum over the gathered [N, K, J] neighbours, then the blend)
  KNN      a LABELLED STAND-IN: the reference calls pytorch3d's knn_points, which is not installed here; torch.cdist over query chunks +
           topk is what a torch user would write without it
  nearest triangles   no torch side: the reference calls libigl on the host (not installed here)
The mesh is a latitude-longitude sphere of radius 0.5 with 10 608 vertices and 21 008 faces (SMPL-X has 10 475 and 20 908); the cloud lies
0.002 .. 0.05 on either side of it, so with the reference's 1 cm threshold a part of the rows is frozen (update weight 0) -- its share
is printed.  The sweeps are also timed with every row active, the worst case.  Times are CUDA-event milliseconds; the KNN and nearest
triangle figures are medians of --reps calls, the sweeps one call of --sweeps sweeps after a warm-up.  The last line is the table as JSON.
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
from dreamwaltz_g_amd import avatar_init as ai  # noqa: E402
from tests import avatar_init_cases as ac  # noqa: E402

K, J = 30, 55


def _ms(fn, reps=1, warm=True):
    if warm:
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


def torch_knn(points, k, chunk=2048):
    """Stand-in for pytorch3d.ops.knn_points(points[None], points[None], K=k): squared distances and indices, ascending."""
    idx, d2 = [], []
    for s in range(0, points.shape[0], chunk):
        d = torch.cdist(points[s:s + chunk], points).square_()
        v, i = torch.topk(d, k, dim=1, largest=False)
        idx.append(i); d2.append(v)
    return torch.cat(idx), torch.cat(d2)


def torch_sweeps(lbs_weights, knn_weights, knn_indices, update_weights, n):
    """avatar.py:904-909 as it reads."""
    for _ in range(n):
        new_lbs_weights = torch.einsum('nk,nkj->nj', knn_weights, lbs_weights[knn_indices])
        lbs_weights = (1.0 - update_weights) * lbs_weights + update_weights * new_lbs_weights
    return lbs_weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,300000")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "b11_bench_avatar_init.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    V, F = ac.make_sphere(rings=102, segments=104, radius=0.5)
    Vt, Ft = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    table = torch.from_numpy(ac.sparse_table(len(V), J, seed=1)).to(dev)
    lines = ["# MI355X, B11 avatar construction; mesh %d vertices / %d faces, K = %d, J = %d; CUDA-event ms; torch side timed before / after the "
             "native side" % (len(V), len(F), K, J)]
    print(lines[0], flush=True)
    rows = []
    for n in [int(s) for s in args.sizes.split(",")]:
        P = torch.from_numpy(ac.shell_points(n, seed=n)).to(dev)
        row = {"N": n}
        # nearest triangles (the reference: libigl on the host, no torch statements to time)
        row["nearest_triangles_ms"] = _ms(lambda: ai.find_nearest_triangles(P, Vt, Ft), args.reps)
        ntb = ai.find_nearest_triangles(P, Vt, Ft)
        w0 = ai.lbs_interp(table, ntb['vertex_indices'].to(dev, torch.int32), ntb['barycentric_coords'])
        # K + 1 nearest neighbours
        t_first = _ms(lambda: torch_knn(P, K + 1), 1)
        row["knn_ms"] = _ms(lambda: ai.knn(P, P, K + 1), args.reps)
        t_last = _ms(lambda: torch_knn(P, K + 1), 1, warm=False)
        row["knn_torch_stand_in_ms"] = [t_first, t_last]
        idx, d2 = ai.knn(P, P, K + 1)
        ti, td = torch_knn(P, K + 1)
        row["knn_rows_equal_to_stand_in"] = float((ti == idx.long()).all(1).float().mean())
        row["knn_d2_max_rel_diff"] = float(((td - d2).abs() / d2.clamp_min(1e-12))[:, 1:].max())
        idx, d2 = idx[:, 1:].contiguous(), d2[:, 1:].contiguous()
        kw, u = ai.knn_weights(idx, d2, ntb['squared_distances'], use_sqrt=True, low=0.01)
        row["frozen_rows_share"] = float((u == 0).float().mean())
        for tag, uu in (("", u), ("_all_active", torch.ones_like(u))):
            idx64, u1 = idx.long(), uu[:, None]
            t_first = _ms(lambda: torch_sweeps(w0, kw, idx64, u1, args.sweeps), 1)
            native = _ms(lambda: ai.smooth_sweeps(w0, idx, kw, uu, args.sweeps), 1)
            t_last = _ms(lambda: torch_sweeps(w0, kw, idx64, u1, args.sweeps), 1, warm=False)
            row["sweep%s_us" % tag] = native / args.sweeps * 1e3
            row["sweep%s_torch_us" % tag] = [t_first / args.sweeps * 1e3, t_last / args.sweeps * 1e3]
            row["sweeps%s_5000_s" % tag] = native / args.sweeps * 5.0
            row["sweeps%s_5000_torch_s" % tag] = [t_first / args.sweeps * 5.0, t_last / args.sweeps * 5.0]
            row["sweeps%s_max_abs_diff" % tag] = float((ai.smooth_sweeps(w0, idx, kw, uu, args.sweeps)
                                                        - torch_sweeps(w0, kw, idx64, u1, args.sweeps)).abs().max())
        rows.append(row)
        line = ("N=%6d  nearest triangles %8.2f ms | KNN(K+1=%d) %8.2f ms  torch stand-in %9.1f / %9.1f ms  (%.4f of rows equal) | "
                "sweep %7.1f us  torch %7.1f / %7.1f us -> x5000: %6.2f s  torch %6.2f / %6.2f s  (frozen rows %.3f, max diff %.1e) | "
                "all rows active: sweep %7.1f us  torch %7.1f / %7.1f us -> x5000: %6.2f s  torch %6.2f / %6.2f s  (max diff %.1e)" % (
                    n, row["nearest_triangles_ms"], K + 1, row["knn_ms"], *row["knn_torch_stand_in_ms"], row["knn_rows_equal_to_stand_in"],
                    row["sweep_us"], *row["sweep_torch_us"], row["sweeps_5000_s"], *row["sweeps_5000_torch_s"], row["frozen_rows_share"],
                    row["sweeps_max_abs_diff"], row["sweep_all_active_us"], *row["sweep_all_active_torch_us"], row["sweeps_all_active_5000_s"],
                    *row["sweeps_all_active_5000_torch_s"], row["sweeps_all_active_max_abs_diff"]))
        lines.append(line)
        print(line, flush=True)
        del P, idx, d2, kw, u, w0, ti, td
        torch.cuda.empty_cache()
    lines.append(json.dumps(rows))
    print(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
