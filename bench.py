"""bench.py -- benchmark of the SDS render-and-distill hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W      the driver contract.  N > 1 with no launcher (WORLD_SIZE unset): this script starts
                                                        its own N ranks through torch.distributed.run (one process per GPU, RCCL); under
                                                        torchrun (WORLD_SIZE set) it is one of the ranks.
    python bench.py --config c1|c2|c4|c5                 one of the other BASELINE.json configurations as its own line
    python bench.py --dtype f32x | f32 | f16 | bf16      storage / arithmetic of the denoiser + VAE plans.  DEFAULT f32x: the reference's own
                                                         precision for this stage (fp32, configs/__init__.py:236,241) as split-precision
                                                         hi + lo fp16 planes on the 16-bit MFMA pipe (eps 3e-6 / SDS gradient 1e-5 vs the fp32 CPU
                                                         oracle); f32 = exact-f32 MFMA; f16 = its --guide.dtype fp16; bf16 = reduced precision
    python bench.py --gpus 2 --share-gpu                 functional run of the multi-rank path on a 1-GPU box (all ranks on cuda:0, gloo)

Prints ONE JSON line (rank 0): metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling / vs_baseline /
dtype / data / config + the roofline's headline numbers as flat scalars.  A "step" is one pass of the hot path over one batch of synthetic
input; inputs are resident in HBM before the timed region (the per-step host input is the 165-float pose).  --steps K is the number of
timed steps: the default c3 run times those K steps and nothing else, and ms_per_step is one of them (c4 times 3 x K and reports the
median; c5 times its side measurements after its K frames).

  c3 (default, the headline)  full SDS step, 100k Gaussians, 512^2, SD-1.5 + ControlNet, one view per GPU       -> SDS steps/s
  c4   multi-view SDS: V = 8 views per step, view v on GPU v mod N, ONE all-reduce of the flat gradient buffer  -> steps/s and views/s
  c2   50k Gaussians + LBS / encoder / MLPs, 512^2 raster fwd+bwd, no guidance                                  -> steps/s, raster GB/s
  c5   300k Gaussians, 1024^2, per-frame animate + raster forward (inference)                                   -> frames/s
  c1   10k Gaussians, canonical pose, 256^2 raster forward only (the plumbing case; BASELINE.md's primary CPU number) -> frames/s

--headline-only keeps the per-kernel blocks ("roofline", "kernel_ms_per_step") in the line.  --all-configs (single GPU) adds the full
report: the CPU baseline, and for c3 the runs of c1 / c2 / c4 (8 views on the one GPU) / c5 attached under "configs" and the same step at
the other plan precisions under "by_dtype" (each with its own roofline peak; their steps/s also sit right behind "dtype" as
"steps_per_s_by_dtype") -- a line of some 20 KB, and timed steps beyond the K asked for.
--dump-outputs DIR writes what the last timed step computed (dump_outputs).
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import _lib  # noqa: E402
from dreamwaltz_g_amd import sds_step  # noqa: E402

HBM_PEAK_GBS = 8000.0                                  # MI355X_MICROARCH.md: 8 TB/s HBM3E
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3, "f32x": 2500.0}      # dense MFMA peaks per operand type (same guide); f32x runs on the
                                                                                       # f16 MFMA pipe, its ALGORITHMIC flops (one multiply-add per product, not the three MFMAs) are priced against that peak
N1_LINE_JSON = os.path.join(ROOT, "profiles", "r06_bench_line.json")           # the round's single-GPU line: N = 1 references of an N > 1 line
TRAFFIC_JSON = os.path.join(ROOT, "profiles", "r06_pmc_traffic.json")      # PMC passes over the f32x (headline) step: tools/profile_round.sh
HEADLINE_DTYPE = "f32x"       # the reference runs the guidance stage in fp32 (configs/__init__.py:236,241): the headline is a same-precision number
HEADLINE_METRIC = "SDS steps/sec @512^2, 100k Gaussians, SD1.5+ControlNet; raster Mpix/s vs HBM roofline"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="default: 20 (c3), 10 (c4: 8 views each), 200 (c1 / c2 / c5, whose steps take ~2 ms)")
    ap.add_argument("--warmup", type=int, default=None, help="default: 3 (c3), 3 (c4), 20 (c1 / c2 / c5)")
    ap.add_argument("--repeats", type=int, default=None, help="timed regions per run (the value is their MEDIAN, min / max reported); default 3 for c4, else 1")
    ap.add_argument("--config", choices=["c1", "c2", "c3", "c4", "c5"], default="c3")
    ap.add_argument("--views", type=int, default=None, help="views per step over ALL GPUs (default: one per GPU for c3, 8 for c4)")
    ap.add_argument("--dtype", choices=["bf16", "f32", "f16", "f32x"], default=HEADLINE_DTYPE, help="storage type of the denoiser / VAE plans")
    ap.add_argument("--gaussians", type=int, default=None)
    ap.add_argument("--res", type=int, default=None)
    ap.add_argument("--headline-only", action="store_true", help="keep the per-kernel roofline / kernel_ms_per_step blocks in the line")
    ap.add_argument("--all-configs", action="store_true", help="the full report: CPU baseline, and for c3 the attached configs / by_dtype legs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-guidance", action="store_true", help="raster+LBS sub-path only (not the headline workload)")
    ap.add_argument("--frames-per-launch", type=int, default=4, help="config c5: pose frames per launch chain of the `batched_frames` side measurement (the value is always frame by frame)")
    ap.add_argument("--frame-graph", action="store_true", help="config c5: replay each frame as one captured hipGraph (player.GraphedAnimation)")
    ap.add_argument("--step-graph", action="store_true", help="config c2 / single-GPU c3: the whole step (zero_grad, condition image, animate, raster, "
                                                              "VAE, ControlNet + UNet, backward, Adam) as ONE captured HIP graph replayed per pose "
                                                              "(step_graph.GraphedTrainStep)")
    ap.add_argument("--moving-camera", action="store_true", help="config c2 / single-view c3: a NEW camera every step (radius, azimuth, elevation, field of "
                    "view from a table of 64, as the reference's loader samples one per step) -- the captured step follows it through its "
                    "device-resident camera block (step_graph.GraphedTrainStep.step(pose, camera))")
    ap.add_argument("--eager", action="store_true", help="launch every kernel eagerly (no hipGraph replay of the denoiser/VAE plans)")
    ap.add_argument("--no-gpu-condition", action="store_true", help="fixed condition image instead of the per-step GPU OpenPose image of the posed body")
    ap.add_argument("--bound-loop", action="store_true", help="config c2 / c3: the step as the reference's own loop drives it through dropin/dwg_bind.py "
                    "(launch by launch, new camera per step, exact pair sizing per frame, loader-side condition image)")
    ap.add_argument("--sync-pairs", action="store_true", help="exact pair-buffer sizing through a 16-byte read-back per frame")
    ap.add_argument("--sequential-views", action="store_true", help="config c4: one guidance call per view (gradients accumulated) instead of one "
                                                                    "batched VAE / denoiser pass for all the views of a rank")
    ap.add_argument("--share-gpu", action="store_true", help="every rank on cuda:0 over gloo: a functional run of the N > 1 path on a 1-GPU box, "
                                                             "NOT a measurement")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the measured workload's LAST timed "
                    "step returned (and, for a training step, the parameter and gradient buffers it left) as DIR/<name>.npy, float32 or float64, "
                    "at most 64 MB in all: arrays of more than 2^20 elements as a fixed seeded sample of at most 2^20 (rank 0; see dump_outputs)")
    return ap.parse_args()


def defaults(config, steps, warmup):
    d = {"c3": (20, 3), "c4": (10, 3)}.get(config, (200, 20))
    return (d[0] if steps is None else steps), (d[1] if warmup is None else warmup)


# ------------------------------------------------------------------------------------------------------------------------------------
# launching N ranks without a launcher
# ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def spawn_ranks(args):
    """`python bench.py --gpus N` with WORLD_SIZE unset: re-execute this script under torch.distributed.run, one rank per GPU."""
    env = dict(os.environ)
    share = args.share_gpu or env.get("DWG_BENCH_SHARE_GPU") == "1"
    if torch.cuda.device_count() < args.gpus and not share:
        sys.stderr.write("bench.py: --gpus %d but %d GPU(s) visible (use --share-gpu for a functional run of the multi-rank path on "
                         "one GPU; its numbers are not a measurement)\n" % (args.gpus, torch.cuda.device_count()))
        return 2
    if share:
        env["DWG_BENCH_SHARE_GPU"] = "1"
        env.setdefault("DWG_BENCH_BACKEND", "gloo")     # RCCL refuses two ranks on one device
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(1, args.gpus))))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU baselines (the oracle timed on the host cores)
# ------------------------------------------------------------------------------------------------------------------------------------
def _cpu_workload(G, res, canonical=False):
    """The oracle's inputs for an `animate` + rasterizer pass at G Gaussians (90 % free with 4 non-zero skinning weights, 10 % mesh-bound)."""
    import numpy as np
    from oracle import animate as oa
    from tests import raster_cases as rc
    M = (G // 10) // 6 * 6
    N = G - M
    body = oa.SyntheticBody(seed=0)
    nets = oa.init_avatar_networks(seed=0)
    g = torch.Generator().manual_seed(1)
    logits = torch.full((N, 55), -1e9)
    logits.scatter_(1, torch.randint(0, 55, (N, 4), generator=g), torch.randn(N, 4, generator=g))
    params = dict(_positions=((torch.rand(N, 3, generator=g) * 2 - 1) * torch.tensor([0.4, 0.9, 0.2])).requires_grad_(True),
                  _scales=torch.log(torch.rand(N, 3, generator=g) * 0.018 + 0.002).requires_grad_(True),
                  _quaternions=torch.randn(N, 4, generator=g).requires_grad_(True), _lbs_weights=torch.softmax(logits, -1))
    nets["table"].requires_grad_(True)
    Vp, Fp = 1200, M // 6
    vi = torch.randperm(body.V, generator=g)[:Vp]
    tri = torch.stack([torch.randint(0, Vp, (Fp,), generator=g) for _ in range(3)], 1)
    tri[:, 1] = (tri[:, 0] + 1 + tri[:, 1] % (Vp // 2 - 1)) % Vp; tri[:, 2] = (tri[:, 0] + Vp // 2 + tri[:, 2] % (Vp // 2)) % Vp    # distinct corners
    base = torch.tensor([[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12],
                         [5 / 12, 1 / 6, 5 / 12], [5 / 12, 5 / 12, 1 / 6]])
    mesh = dict(vertex_indices=vi, triangles=tri, vertex_coords=body.v_template[vi], bary=base.expand(Fp, -1, -1).clone().requires_grad_(True),
                scales=torch.ones(Fp * 6, 3).requires_grad_(True)) if M > 0 else None
    cnl = dict(body_pose=torch.zeros(1, 63), global_orient=torch.zeros(1, 3), left_hand_pose=torch.zeros(1, 45),
               right_hand_pose=torch.zeros(1, 45), expression=torch.zeros(1, 100))
    obs = dict(cnl, transl=torch.zeros(1, 3)) if canonical else oa.random_smpl_inputs(seed=3)
    sc = rc.make_scene(G, res, res, seed=0)
    wc = np.random.RandomState(0).randn(3, res, res).astype(np.float32)
    return dict(oa=oa, rc=rc, params=params, nets=nets, body=body, obs=obs, cnl=cnl, mesh=mesh, sc=sc, wc=wc, N=N, M=M)


def _cpu_pass(w, backward):
    """One pass: oracle animate (+ autograd backward) and the multi-threaded C tile rasterizer forward (+ backward).  Seconds each."""
    import numpy as np
    oa, rc = w["oa"], w["rc"]
    for v in list(w["params"].values()) + [w["nets"]["table"]] + ([w["mesh"]["bary"], w["mesh"]["scales"]] if w["mesh"] else []):
        v.grad = None
    t0 = time.perf_counter()
    if backward:
        out = oa.animate(w["params"], w["nets"], w["body"], w["obs"], w["cnl"], mesh=w["mesh"])
        sum(v.sum() for v in out.values()).backward()
    else:
        with torch.no_grad():
            oa.animate(w["params"], w["nets"], w["body"], w["obs"], w["cnl"], mesh=w["mesh"])
    t1 = time.perf_counter()
    rc.oracle_forward(w["sc"], omp=True, near=None)
    if backward:
        rc.oracle_backward(w["sc"], w["wc"], None, None, dtype=np.float32, omp=True)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


CPU_BASELINE_THREADS = 32     # the SAME thread count on every box (torch intra-op pool and the OpenMP tile rasterizer alike)


def _cpu_worker(spec):
    """Body of the `--_cpu-worker` child process (see cpu_baseline): affinity and thread counts are set BEFORE torch / the OpenMP oracle create
    their pools, so every pool has `nthr` threads on `nthr` cores and nothing left over from the GPU legs spins beside them."""
    import numpy as np
    nthr = spec["threads"]
    pinned = False
    # Affinity: NOT pinned by default.  Measured on the pool's 2 x 64-core EPYC 9575F hosts (tools/cpu_probe.sh, same box, 100 k / 512^2,
    # s per pass min / median / max): unpinned 2.8 / 3.0 / 4.7, pinned to the first 32 CPUs 3.8 / 7.0 / 15.1, to every 8th CPU 8.0 / 12.5 /
    # 19.7 -- the hosts are shared, and a pinned process cannot move away from cores somebody else is using.  DWG_CPU_PIN=first|spread pins.
    mode = os.environ.get("DWG_CPU_PIN", "none")
    try:
        allowed = sorted(os.sched_getaffinity(0))
        if mode == "first":
            pick = allowed[:nthr]
        elif mode == "spread":                           # every (n / nthr)-th allowed CPU: one thread per physical core, all NUMA nodes
            st = max(1, len(allowed) // nthr)
            pick = allowed[::st][:nthr]
        else:
            pick = None
        if pick:
            os.sched_setaffinity(0, set(pick))
            pinned = mode
    except (AttributeError, OSError):
        pinned = False
    torch.set_num_threads(nthr)
    w = _cpu_workload(spec["G"], spec["res"], spec["canonical"])
    _cpu_pass(w, spec["backward"])                       # warm-up: library load, OpenMP pools, allocator
    ta, tr, spent = [], [], 0.0
    while len(ta) < 5 or (spent < spec["budget_s"] and len(ta) < 9):
        a, r = _cpu_pass(w, spec["backward"])
        ta.append(a); tr.append(r); spent += a + r
    print("CPU_WORKER_RESULT " + json.dumps({"ta": ta, "tr": tr, "spent": spent, "pinned": pinned, "N": w["N"], "M": w["M"]}), flush=True)


def cpu_baseline(G, res, backward=True, canonical=False, budget_s=10.0, unit="steps/s"):
    """The oracle (CPU restatement of the reference's PyTorch LBS / encoder / MLP path + the C tile rasterizer, OpenMP over tiles) timed on
    the host cores on the SAME kind of workload the GPU step renders.  Hygiene (round 4; the same leg measured 0.24 .. 0.91 steps/s on
    different boxes in round 3): the passes run in a FRESH child process with a FIXED 32 threads for the torch pool and the OpenMP rasterizer
    alike -- set before either library creates a pool, so no spinning left-over threads of the GPU legs compete (affinity pinning was
    measured and made the SHARED hosts of this pool slower and noisier: see _cpu_worker) (BASELINE.md
    section 4 prescribes all cores; on the 256-core GPU hosts the oracle's small-tensor ops are 30x slower that way: every op pays the
    wake-up of 256 OpenMP threads) -- one untimed warm-up pass, then at least 5 timed passes: min AND median reported, `value` = from the
    median.  The reference has no CPU diffusion path, so the diffusion half of a step has no CPU counterpart and is NOT in this number."""
    import numpy as np
    host = os.cpu_count() or 1
    nthr = min(CPU_BASELINE_THREADS, host)
    spec = {"G": int(G), "res": int(res), "backward": bool(backward), "canonical": bool(canonical), "budget_s": float(budget_s), "threads": nthr}
    env = dict(os.environ)
    env.update(OMP_NUM_THREADS=str(nthr), MKL_NUM_THREADS=str(nthr), OMP_PROC_BIND="false", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--_cpu-worker", json.dumps(spec)], env=env, capture_output=True, text=True,
                       timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CPU_WORKER_RESULT ")]
    if r.returncode != 0 or not line:
        return {"value": None, "unit": unit, "cores": nthr, "kind": "port", "error": (r.stderr or r.stdout)[-600:]}
    o = json.loads(line[-1][len("CPU_WORKER_RESULT "):])
    ta, tr = o["ta"], o["tr"]
    tot = np.array(ta) + np.array(tr)
    t_med, t_min = float(np.median(tot)), float(tot.min())
    t_an, t_ra = float(np.median(ta)), float(np.median(tr))
    what = "fwd+bwd" if backward else "forward"
    return {"value": 1.0 / t_med, "value_best": 1.0 / t_min, "unit": "%s (animate + rasterizer %s, no diffusion)" % (unit, what), "cores": nthr,
            "kind": "port", "host_cores": host, "pinned": o["pinned"], "passes": len(ta),
            "s_per_pass": {"min": round(t_min, 4), "median": round(t_med, 4), "max": round(float(tot.max()), 4)},
            "sample": "%d timed passes after 1 warm-up (%.0f s of CPU work) in a fresh process, value = 1 / median: oracle animate %s %.3f s (%d free "
                      "Gaussians with 4 non-zero skinning weights + %d mesh-bound) + C tile rasterizer %s %.3f s (OpenMP over tiles; %d Gaussians "
                      "@%dx%d); %d threads for both on the %d-CPU host (affinity: %s)"
                      % (len(ta), o["spent"], what, t_an, o["N"], o["M"], what, t_ra, G, res, res, nthr, host, o["pinned"] or "not pinned")}


# ------------------------------------------------------------------------------------------------------------------------------------
# roofline reports
# ------------------------------------------------------------------------------------------------------------------------------------
def sources_sha():
    """Hash of the kernel sources: stamps the PMC traffic profile (tools/pmc_traffic.py) so that a profile taken on OTHER kernels is marked."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "dreamwaltz-g_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def _traffic():
    if not os.path.exists(TRAFFIC_JSON):
        return None, None
    t = json.load(open(TRAFFIC_JSON))
    stale = t.get("sources_sha") != sources_sha()
    return t, stale


def raster_report(prof, G, Kref, K, P, steps, pmc=False):
    """Rasterizer against the HBM roofline with SURVEY 8d's byte formula (K = reference tile-pair count; sort traffic not counted)."""
    rf = sum(v[1] for k, v in prof.items() if k.startswith("raster_") and not k.endswith("_bwd")) / steps
    rb = sum(v[1] for k, v in prof.items() if k.startswith("raster_") and k.endswith("_bwd")) / steps
    out = {}
    if rf > 0:
        b = 56 * G + 44 * Kref + 20 * P
        out["raster_forward"] = {"bytes": b, "pairs_reference": Kref, "pairs_after_exact_culling": K, "ms": rf, "mpix_per_s": P / (rf * 1e-3) / 1e6,
                                 "achieved_GBps": b / (rf * 1e-3) / 1e9, "frac_of_hbm_peak": b / (rf * 1e-3) / 1e9 / HBM_PEAK_GBS}
    if rb > 0:
        b = 80 * Kref + 20 * P + 152 * G
        out["raster_backward"] = {"bytes": b, "ms": rb, "achieved_GBps": b / (rb * 1e-3) / 1e9,
                                  "frac_of_hbm_peak": b / (rb * 1e-3) / 1e9 / HBM_PEAK_GBS}
    tj, stale = _traffic() if pmc else (None, None)
    if tj is not None:       # HBM bytes per frame from the PMC passes (taken on the default c3 workload only)
        tk = tj["kernels"]
        fwd = ("k_preprocess", "k_scan_super", "k_scatter_super", "k_chunk_sort", "k_rank_merge", "k_split", "k_render_fwd", "k_camera_setup", "k_camera_block")
        bwd = ("k_render_bwd", "k_gather_partials", "k_preprocess_bwd")
        for key, names in (("raster_forward", fwd), ("raster_backward", bwd)):
            if key in out:
                # ONE number: FETCH_SIZE x 2 for the kernels that stream, x 1 for the ones that gather (tools/pmc_traffic.py, calibrated on known
                # byte counts: profiles/r06_fetch_calibration.json), + WRITE_SIZE
                t = sum(v["hbm_bytes_per_launch"] * v.get("launches_per_step", 1) for k, v in tk.items() if k.split("<")[0] in names)
                out[key]["traffic"] = t
                out[key]["traffic_over_algorithmic"] = t / out[key]["bytes"]
                out[key]["traffic_stale"] = bool(stale)
    return out


def roofline(prof, prof_sym, prof_steps, G, Kref, K, P, dtype="bf16"):
    """Roofline entry for the dominant kernel = the kernel SYMBOL (as rocprofv3 --kernel-trace names it) with the largest total time
    in the profiled region; achieved = algorithmic work per launch / average launch duration (HIP events on the launch stream)."""
    out = {}
    peak = MFMA_PEAK_TFLOPS[dtype]
    if prof_sym:
        # largest total time; symbols within 8 % of the largest are ranked by their algorithmic work instead: an event bracket over-reads a
        # ~18 us launch by ~3 us (dispatch + release, which rocprofv3's kernel trace does not count: csrc/prof.hip), enough to reorder a
        # near-tie between 170 launches of 20 us and 17 of 215 us per step against the order the committed rocprofv3 summary shows
        top_ms = max(v[1] for v in prof_sym.values())
        name, (count, total_ms, work) = max(((k, v) for k, v in prof_sym.items() if v[1] >= 0.92 * top_ms), key=lambda kv: (kv[1][2], kv[1][1]))
        avg_ms = total_ms / max(1, count)
        if work > 0:
            ach = work / count / (avg_ms * 1e-3) / 1e12
            out = {"kernel": name, "bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
                   "traffic": None, "avg_launch_ms": avg_ms, "launches": count, "flops_per_launch": work / count}
        else:
            out = {"kernel": name, "bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None,
                   "avg_launch_ms": avg_ms, "launches": count}
        out["mfma_kernels"] = {k: {"launches": c, "avg_launch_ms": ms / c, "tflops": w / (ms * 1e-3) / 1e12, "frac": w / (ms * 1e-3) / 1e12 / peak}
                               for k, (c, ms, w) in sorted(prof_sym.items(), key=lambda kv: -kv[1][1]) if w > 0 and ms > 0}
        tw = sum(w for (_, _, w) in prof_sym.values()); tms = sum(ms for (_, ms, w) in prof_sym.values() if w > 0)
        if tms > 0:
            out["mfma_all"] = {"tflops": tw / (tms * 1e-3) / 1e12, "frac": tw / (tms * 1e-3) / 1e12 / peak, "flops_per_step": tw / prof_steps,
                               "ms_per_step": tms / prof_steps, "includes": "GEMM / conv / attention launches"}
        tj, stale = _traffic()
        if tj is not None and out.get("kernel") and dtype == tj.get("plan_dtype", "bf16"):
            tk = tj["kernels"].get(out["kernel"].replace(" ", ""))
            if tk:
                out["traffic"] = tk["hbm_bytes_per_launch"]
                out["traffic_source"] = "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, gfx950 corrections)" % os.path.basename(TRAFFIC_JSON)
                out["traffic_stale"] = bool(stale)       # True: the profile was taken on other kernel sources than the ones running now
    out.update(raster_report(prof, G, Kref, K, P, prof_steps, pmc=(G == 100000 and P == 512 * 512)))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the workloads
# ------------------------------------------------------------------------------------------------------------------------------------
class Ctx:
    """rank / world / device / process group of this process (+ objects shared between the legs of the default invocation)."""

    def __init__(self, args):
        self.args = args
        self.rank = int(os.environ.get("RANK", "0")); self.world = int(os.environ.get("WORLD_SIZE", "1"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        # Functional run of the N > 1 flow on a 1-GPU box: every rank on cuda:0 over gloo (RCCL refuses two ranks on one device).
        self.shared_gpu = os.environ.get("DWG_BENCH_SHARE_GPU") == "1" or args.share_gpu
        if self.shared_gpu:
            local = 0
        torch.cuda.set_device(local)
        self.dev = torch.device("cuda", local)
        self.dist = None
        if self.world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = os.environ.get("DWG_BENCH_BACKEND", "gloo" if self.shared_gpu else "nccl")
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=self.dev)
            else:
                dist.init_process_group(backend)
            self.dist, self.backend = dist, backend
        torch.cuda.set_stream(torch.cuda.Stream(device=self.dev))   # one real (non-default) HIP stream for the whole step: graph-safe
        self.guidance = {}          # dtype -> ControlNetScoreDistillation (plans are shared between the c3 and c4 legs)
        self.state_dicts = None

    def guidance_for(self, dtype, views=1):
        """One guidance object per (plan dtype, views per call); the seeded random-init state dicts (1.22 G + 34 M parameters, generated on
        the host) are made once, and the kernel-layout weights in HBM are shared between the objects of one dtype."""
        key = dtype if views == 1 else (dtype, views)
        if key not in self.guidance:
            if views > 1:
                from dreamwaltz_g_amd import guidance as gd
                base = self.guidance_for(dtype, 1)
                self.guidance[key] = gd.ControlNetScoreDistillation(self.dev, image_hw=512, seed=0, dtype=dtype, views=views, share_weights_with=base)
                return self.guidance[key]
            from dreamwaltz_g_amd import guidance as gd, sd15
            if self.state_dicts is None:
                u, v = sd15.UNetConfig(), sd15.VAEConfig()
                self.state_dicts = (sd15.random_state_dict(sd15.unet_param_shapes(u), seed=0),
                                    sd15.random_state_dict(sd15.controlnet_param_shapes(u), seed=1),
                                    sd15.random_state_dict(sd15.vae_encoder_param_shapes(v), seed=2))
            usd, csd, vsd = self.state_dicts
            g = gd.ControlNetScoreDistillation(self.dev, image_hw=512, seed=0, unet_sd=usd, controlnet_sd=csd, vae_sd=vsd, dtype=dtype)
            self.guidance[dtype] = g
            import gc
            gc.collect(); gc.freeze()           # the plans are ~1e5 long-lived Python objects: out of the cyclic collector's way
        return self.guidance[key]


def _timed(ctx, fn, steps, warmup, keep=None):
    """W untimed + EXACTLY K timed calls bracketed by barrier + synchronize on both sides; MAX over ranks.  `keep` (a list): receives what
    the LAST timed call returned (no other call's result is held on to)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    if ctx.dist is not None:
        ctx.dist.barrier()
    torch.cuda.synchronize()
    last = steps > 0 and keep is not None
    t0 = time.perf_counter()
    for _ in range(steps - 1 if last else steps):
        fn()
    if last:
        keep[:] = [fn()]
    torch.cuda.synchronize()
    if ctx.dist is not None:
        ctx.dist.barrier()
    dt = time.perf_counter() - t0
    if ctx.dist is not None:
        t = torch.tensor([dt], device=ctx.dev if ctx.backend == "nccl" else "cpu", dtype=torch.float64)
        ctx.dist.all_reduce(t, op=ctx.dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


DUMP_LIMIT_BYTES = 64 << 20         # --dump-outputs: all files together
DUMP_SAMPLE = 1 << 20               # an array of more elements is dumped as (at most) this many of them, at fixed seeded positions


def snapshot_outputs(named):
    """{name: host array} of every tensor inside `named` ({name: tensor / dict / list / tuple}, nested; other values are skipped), copied
    off the device at once -- the next step or a graph replay overwrites them.  Floating tensors stay float32 (float64 if they are),
    integer and boolean ones become float64 (exact)."""
    import numpy as np
    out = {}

    def walk(name, v):
        if isinstance(v, torch.Tensor):
            t = v.detach()
            out[name] = t.cpu().numpy().astype(np.float64 if t.dtype == torch.float64 or not t.is_floating_point() else np.float32)
        elif isinstance(v, dict):
            for k, x in v.items():
                walk("%s.%s" % (name, k), x)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk("%s.%d" % (name, i), x)
    for k, v in named.items():
        walk(k, v)
    return out


def dump_outputs(arrays, path):
    """Writes the snapshot as path/<name>.npy, DUMP_LIMIT_BYTES at most.  An array of more than `cap` elements is written flattened, as the
    elements at np.sort(RandomState(0).choice(size, cap, replace=False)); `cap` starts at DUMP_SAMPLE and is halved until everything fits.
    The positions depend only on the shapes, so that two builds are compared element for element.  Returns a summary for the result line."""
    import numpy as np
    cap = DUMP_SAMPLE
    while sum(a.itemsize * min(a.size, cap) for a in arrays.values()) > DUMP_LIMIT_BYTES:
        cap //= 2
    os.makedirs(path, exist_ok=True)
    total, sampled = 0, []
    for name, a in sorted(arrays.items()):
        if a.size > cap:
            a = a.reshape(-1)[np.sort(np.random.RandomState(0).choice(a.size, cap, replace=False))]
            sampled.append(name)
        np.save(os.path.join(path, name + ".npy"), a)
        total += a.nbytes
    return {"dir": path, "arrays": len(arrays), "bytes": total, "sampled": sampled, "sample_elements": cap}


def run_sds(ctx, config, dtype=HEADLINE_DTYPE, views=None, steps=None, warmup=None, profile=True, batch_views=None, repeats=None, step_graph=None,
            moving_camera=False, bound_loop=None, dump=None):
    """c2 / c3 / c4: SDSStep-based workloads.  Returns the JSON line as a dict (rank 0) or None.
    `dump` (a directory): what the last timed step returned -- loss, render outputs, guidance outputs -- and the flat parameter / gradient
    buffers it left, written there (dump_outputs).
    `bound_loop`: the step as the reference's OWN loop drives it through the binding (dropin/dwg_bind.py; /root/reference/core/trainer.py:840-896):
    zero_grad -> update_learning_rate -> render -> guidance -> backward -> every optimizer's step, launch by launch from Python (no captured
    step), a NEW camera every step, the pair workspace sized by the 16-byte read-back per frame (the binding builds its Scene with
    async_pair_count=False: the reference's loop body knows nothing about re-rendering a truncated frame) and the condition image handed
    over by the loader (the reference draws it on the CPU in its dataloader workers, outside the seams) -- the denoiser / VAE plans replay
    as the hipGraphs bind_guidance captures.  This is the rate a `main.py` user gets."""
    args = ctx.args
    bound = bool(getattr(args, "bound_loop", False)) if bound_loop is None else bool(bound_loop)
    if bound:
        moving_camera, step_graph = True, False
    steps, warmup = defaults(config, steps, warmup)
    guidance = config in ("c3", "c4") and not args.no_guidance
    G = args.gaussians or (50000 if config == "c2" else 100000)
    res = args.res or 512
    if views is None:
        views = 8 if config == "c4" else ctx.world
    if views < ctx.world:
        raise SystemExit("bench.py: %d views cannot be spread over %d GPUs (at least one view per rank)" % (views, ctx.world))
    per_rank = len(range(ctx.rank, views, ctx.world))
    if batch_views is None:         # c4: one guidance call per step for all the views of a rank, unless --sequential-views
        batch_views = config == "c4" and not args.sequential_views
    batch_views = bool(batch_views and guidance and per_rank > 1 and views % ctx.world == 0)
    step = sds_step.SDSStep(n_gaussians=G, res=res, device=ctx.dev, rank=ctx.rank, world=ctx.world, guidance=guidance, dist=ctx.dist,
                            async_pair_count=not (args.sync_pairs or bound), gpu_condition=not (args.no_gpu_condition or bound), views=views, dtype=dtype,
                            guidance_obj=ctx.guidance_for(dtype, per_rank if batch_views else 1) if guidance else None)
    moving = bool(getattr(args, "moving_camera", False) or moving_camera) and views == 1 and ctx.world == 1
    if moving:
        # the reference samples a camera per step (data/camera/__init__.py:124-165); its loader builds the matrices in dataloader workers,
        # so the table is made ahead of the timed region here as well
        from dreamwaltz_g_amd import camera as _cam
        table = [_cam.make_camera(radius=1.8 + 0.05 * (i % 7), azimuth=(360.0 / 64) * i, elevation=70.0 + 2.5 * (i % 5), fovy=48.0 + 1.5 * (i % 6),
                                  height=res, width=res, device="cpu") for i in range(64)]
        step.camera_fn = lambda i: table[i % 64]
    if not args.eager:
        step.capture_graphs()       # denoiser / VAE plans replay as hipGraphs (identical kernels, one launch each)
    else:
        step.set_use_graphs(False)
    if args.eager:
        for _ in range(warmup):
            step.run()
        warmup = 0
        _lib.prof_enable(True)
    if repeats is None:
        repeats = args.repeats or (3 if config == "c4" else 1)
    run = step.run
    whole_graph = (bool(getattr(args, "step_graph", False)) if step_graph is None else bool(step_graph)) and not args.eager and ctx.world == 1 \
        and ((config == "c2" and not guidance) or (config == "c3" and guidance and views == 1))
    if whole_graph:
        runner = step.graphed()
        run = runner.step
    keep = [] if dump is not None and ctx.rank == 0 else None
    dts = [_timed(ctx, run, steps, warmup if r == 0 else 0, keep) for r in range(max(1, repeats))]       # each: barrier + sync on both sides, max over ranks
    recaptures = 0
    while whole_graph and runner.graph.check():
        # a replay needed more (Gaussian, block) pairs than the capacity frozen into the graph and was truncated by the kernels: the timed
        # region is void -- capture again with twice the capacity and time again (what a training loop does on check())
        recaptures += 1
        if recaptures > 3:
            raise SystemExit("bench.py: captured steps kept being truncated by the frozen pair capacity")
        runner.graph.recapture()
        dts = [_timed(ctx, run, steps, 2, keep) for r in range(max(1, repeats))]
    dt = sorted(dts)[len(dts) // 2]
    dumped = None
    if keep:
        # before the eager profiling steps below move the parameters on: the step's (loss, render outputs[, guidance outputs]) and the
        # flat parameter / gradient buffers it left
        bufs = step.optimizers.buffers
        dumped = dump_outputs(snapshot_outputs(dict(zip(("loss", "render", "guidance"), keep[0]), params=bufs.flat, grads=bufs.grad)), dump)
        keep.clear()
    prof_steps, prof, prof_sym = steps, {}, {}
    if profile and not args.eager:
        # Per-kernel durations (HIP events on the launch stream) cannot be bracketed inside a graph replay: the same steps
        # are replayed eagerly right after the timed region with the event timers on (same kernels, same inputs).
        step.set_use_graphs(False)
        prof_steps = min(steps, 3)
        _lib.prof_enable(True)
        for _ in range(prof_steps):
            step.run()
        torch.cuda.synchronize()
    if profile or args.eager:
        prof, prof_sym = _lib.prof_table(), _lib.prof_symbols()
        _lib.prof_enable(False)
    step.set_use_graphs(not args.eager)
    if ctx.rank != 0:
        return None
    info = step.describe()
    K, Kref = step.num_pairs
    headline = config == "c3" and guidance
    vps = len(step.my_views)
    if config == "c4":
        metric = "Multi-view SDS (config c4): steps/s, %d views per step sharded over the GPUs, one flat-gradient all-reduce, 100k Gaussians 512^2" % views
        value, unit, scaling = steps / dt, "steps/s (one step = %d views; whole job)" % views, "strong"
    elif headline:
        metric, value, unit, scaling = HEADLINE_METRIC, views * steps / dt, "SDS steps/s (one view each; whole job)", "weak"
    else:
        metric = "config %s sub-path (NOT the headline): animate + raster fwd+bwd + Adam steps/s, %dk Gaussians @%d^2, no guidance" % (config, G // 1000, res)
        value, unit, scaling = views * steps / dt, "steps/s", "weak"
    out = {"metric": metric, "value": value, "unit": unit, "n_gpus": ctx.world}
    if ctx.world > 1:
        # what a reader of an N > 1 line needs inside its first 2 KB: that N ranks really ran, over which backend, what the exchange step
        # costs, and how the rate compares with the two N = 1 forms of the same work (profiles/: measured on ONE GPU by the default run)
        out["dist"] = {"world_size": ctx.dist.get_world_size(), "backend": ctx.dist.get_backend(), "views_per_step": views,
                       "views_per_s": views * steps / dt, "allreduce_ms_per_step": step.trainer.allreduce_ms,
                       "allreduce": "one asynchronous all-reduce per named optimizer's slice of the flat fp32 gradient buffer (%.1f MB in all), "
                                    "smallest first, each optimizer stepping behind its slice; the time is issue .. last optimizer launched"
                                    % (step.optimizers.buffers.grad.numel() * 4 / 1e6)}
        ref = n1_reference(config, guidance)
        if ref:
            out["dist"].update(ref)
            for k in ("n1_batched_views_per_s", "n1_sequential_views_per_s", "n1_views_per_s"):
                if ref.get(k):
                    out["dist"]["scaling_vs_" + k[:-len("_views_per_s")]] = (views * steps / dt) / ref[k]
    out.update({"steps": steps, "warmup": warmup if not args.eager else 0,
                "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": info["dtype"],
                "data": "synthetic", "config": info["config"]})
    out["views_per_s"] = views * steps / dt
    if len(dts) > 1:
        out["repeats"] = {"n": len(dts), "value_is": "median", "ms_per_step_min": min(dts) / steps * 1e3, "ms_per_step_median": dt / steps * 1e3,
                          "ms_per_step_max": max(dts) / steps * 1e3}
    out["views_per_step"], out["views_per_step_per_gpu"] = views, vps
    if ctx.shared_gpu and ctx.world > 1:
        out["shared_gpu"] = "all %d ranks on ONE GPU over %s: a functional run of the multi-rank path, NOT a measurement" % (ctx.world, ctx.backend)
    if prof_sym or prof:
        out["roofline"] = roofline(prof, prof_sym, prof_steps * vps, step.G, Kref, K, res * res, dtype=info["dtype"] if guidance else "f32")
        rf = out["roofline"].get("raster_forward")
        out["raster_mpix_per_s"] = rf["mpix_per_s"] if rf else None      # the rasterizer's own forward rate (pixels / forward-chain time)
        out["kernel_ms_per_step"] = {k: round(v[1] / prof_steps, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:40]}
    out["redone_frames"] = step.trainer.redone_frames
    out["camera"] = "a new camera every step (64-entry table: radius, azimuth, elevation, field of view all move)" if moving else "fixed"
    if whole_graph:
        out["graph_recaptures"] = recaptures
    if bound:
        out["bound_loop"] = ("driven as /root/reference/core/trainer.py:840-896 drives it through dropin/dwg_bind.py: launch by launch, new camera per step, "
                             "16-byte pair-count read-back per frame, loader-side condition image")
    out["launch_mode"] = ("eager" if args.eager else "the WHOLE step (zero_grad, animate, raster fwd + bwd, Adam) replayed as one captured HIP graph per pose"
                          if whole_graph else "hipGraph replay of denoiser/VAE plans; kernel timers from an eager replay after the timed region")
    if dumped:
        out["dumped_outputs"] = dumped
    return out


def n1_reference(config, guidance):
    """The N = 1 rates an N > 1 line is compared with, read from the round's committed single-GPU line (profiles/, labelled with its file):
    for c4 both ways one GPU can do the step's 8 views -- ONE batched guidance call, or one call per view -- and for c3 the single-view rate.
    The driver computes scaling efficiency itself from its own per-N runs; these ratios only make a lone N = 8 line readable."""
    if not guidance or not os.path.exists(N1_LINE_JSON):
        return None
    try:
        d = json.load(open(N1_LINE_JSON))
        src = "profiles/" + os.path.basename(N1_LINE_JSON)
        if config == "c4":
            c = d.get("configs", {})
            return {"n1_batched_views_per_s": c["c4_n1"]["views_per_s"], "n1_sequential_views_per_s": c["c4_n1_sequential_views"]["views_per_s"],
                    "n1_source": src}
        return {"n1_views_per_s": d["value"], "n1_source": src}
    except Exception:       # an older line without these legs: no reference, no ratios
        return None


def _scene(ctx, G):
    from dreamwaltz_g_amd import configs, scene as sc
    cfg = configs.TrainConfig(); cfg.device = str(ctx.dev); cfg.render.bg_color = (0.5, 0.5, 0.5)
    avatar, N, M = sds_step.build_synthetic_avatar(G, ctx.dev, seed=0)
    return sc.Scene(cfg, avatar, async_pair_count=not ctx.args.sync_pairs).to(ctx.dev).eval(), N, M


def run_c5(ctx, steps=None, warmup=None, dump=None):
    """Config c5: 300k-Gaussian avatar, per-frame animate (LBS + encoder + MLPs + mesh binding) + raster forward at 1024^2, inference.
    `dump` (a directory): the last timed frame's outputs written there (dump_outputs)."""
    args = ctx.args
    steps, warmup = defaults("c5", steps, warmup)
    G, res = args.gaussians or 300000, args.res or 1024
    from dreamwaltz_g_amd import camera, synth
    scene, N, M = _scene(ctx, G)
    data = camera.make_camera(radius=2.0, azimuth=0.0, elevation=80.0, fovy=55.0, height=res, width=res, device=ctx.dev)
    poses = [synth.random_smpl_inputs(seed=i, device=ctx.dev) for i in range(240)]        # 240 pose frames
    player = None
    if args.frame_graph:        # the frame as ONE captured graph replayed per pose (player.GraphedAnimation); measured: no gain, the frame is GPU-bound
        from dreamwaltz_g_amd import player as pl
        player = pl.GraphedAnimation(scene, data, poses[0], warmup_poses=poses[:24])
    idx = [0]
    F = 1 if player is not None else max(1, int(args.frames_per_launch))

    def frame():
        i = idx[0]; idx[0] += 1
        if player is not None:
            return player.replay(poses[i % 240])
        with torch.inference_mode():
            return scene.forward(data, smpl_observed_inputs=poses[i % 240], use_densifier=False, bg_mode=None)

    frozen = [False]

    def batch():                # F pose frames animated one by one, rasterized by ONE launch chain (Scene.forward_frames)
        i = idx[0]; idx[0] += F
        with torch.inference_mode():
            return scene.forward_frames(data, [poses[(i + f) % 240] for f in range(F)], bg_mode=None, frozen_avatar=frozen[0])
    # `value` is the reference's loop: ONE frame per call (/root/reference/core/trainer.py:1019-1150).  The batched form (F pose frames per
    # rasterizer launch chain, bit-identical images) and the frozen-avatar form are measured right after it and reported in side fields.
    keep = [] if dump is not None else None
    dt = _timed(ctx, frame, steps, warmup, keep)
    dumped = dump_outputs(snapshot_outputs({"render": keep[0]}), dump) if keep else None
    dt_batched = dt_frozen = None
    bsteps = (steps + F - 1) // F * F
    if F > 1:
        bwarm = (warmup + F - 1) // F * F
        dt_batched = _timed(ctx, batch, bsteps // F, bwarm // F)
        frozen[0] = True
        dt_frozen = _timed(ctx, batch, bsteps // F, bwarm // F)
        frozen[0] = False
    graphed = player is not None
    if graphed:                 # per-kernel timers need eager launches: same kernels, same inputs, after the timed region
        assert player.check(), "a replayed frame was truncated by the frozen pair capacity"
        player.close(); player = None
    _lib.prof_enable(True)
    ps = min(steps, 5)
    for _ in range(ps):
        frame()
    torch.cuda.synchronize()
    prof = _lib.prof_table(); _lib.prof_enable(False)
    K, Kref = scene.renderer.last_rasterizer.last_num_pairs
    batched = None
    if F > 1:
        _lib.prof_enable(True)
        for _ in range(2):
            batch()
        torch.cuda.synchronize()
        profb = _lib.prof_table(); _lib.prof_enable(False)
        hdr = scene.renderer.last_frames_headers.cpu()
        Kb, Krefb = int(hdr[:, 0].float().mean()), int(hdr[:, 2].float().mean())
        batched = {"frames_per_launch": F, "value": bsteps / dt_batched, "unit": "frames/s", "ms_per_frame": dt_batched / bsteps * 1e3,
                   "what": "the same frames, F pose frames per rasterizer launch chain (Scene.forward_frames: animate per frame, one binning + "
                           "compositing chain for the batch); every image bit-identical to the frame-by-frame one",
                   "roofline": raster_report(profb, G, Krefb, Kb, res * res, 2 * F),
                   "kernel_ms_per_frame": {k: round(v[1] / (2 * F), 4) for k, v in sorted(profb.items(), key=lambda kv: -kv[1][1])[:12]}}
    return {"metric": "AIST++-style animation inference (config c5): frames/s, %dk-Gaussian avatar, per-frame LBS+raster at %d^2" % (G // 1000, res),
            "value": steps / dt, "unit": "frames/s", "n_gpus": 1, "steps": steps, "warmup": warmup, "ms_per_step": dt / steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "c5: animate (LBS x2, grid encoder, MLPs, %d free + %d mesh-bound Gaussians) + raster forward %dx%d, "
                                   "inference_mode, 240 seeded random pose frames" % (N, M, res, res), "gaussians": G, "resolution": res},
            "roofline": raster_report(prof, G, Kref, K, res * res, ps),
            "launch_mode": "one hipGraph per frame (player.GraphedAnimation); kernel timers from eager frames after the timed region" if graphed
                           else "eager, frame by frame (the reference's evaluation loop); `batched_frames`: F pose frames per launch chain",
            "frames_per_launch": 1,
            "batched_frames": batched,
            "frozen_avatar_playback": None if dt_frozen is None else {
                "value": bsteps / dt_frozen, "unit": "frames/s", "ms_per_step": dt_frozen / bsteps * 1e3,
                "what": "the batched frames with Scene.forward_frames(frozen_avatar=True): canonical positions, grid encoding and the colour / opacity "
                        "network computed once and kept while no parameter changes (bit-identical images); NOT the c5 value -- there every frame "
                        "recomputes them, as the reference's evaluation loop does"},
            "kernel_ms_per_step": {k: round(v[1] / ps, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:20]}} | ({"dumped_outputs": dumped} if dumped else {})


def run_c1(ctx, steps=None, warmup=None, dump=None):
    """Config c1 (the plumbing case; BASELINE.md's primary CPU number): 10k Gaussians, canonical neutral pose, 256^2, raster forward only
    -- Scene.forward without observed pose (avatar.forward(): canonical LBS + encoder + MLPs) under inference mode.  `dump` (a directory):
    the last timed frame's outputs written there (dump_outputs)."""
    args = ctx.args
    steps, warmup = defaults("c1", steps, warmup)
    G, res = args.gaussians or 10000, args.res or 256
    from dreamwaltz_g_amd import camera
    scene, N, M = _scene(ctx, G)
    data = camera.make_camera(radius=2.0, azimuth=30.0, elevation=80.0, fovy=55.0, height=res, width=res, device=ctx.dev)

    def frame():
        with torch.inference_mode():
            return scene.forward(data, smpl_observed_inputs=None, use_densifier=False, bg_mode=None)
    player = None
    if not args.eager:          # the frame as ONE captured graph (player.GraphedAnimation, canonical pose: no per-frame input)
        from dreamwaltz_g_amd import player as pl
        player = pl.GraphedAnimation(scene, data, None)
    keep = [] if dump is not None else None
    dt = _timed(ctx, player.replay if player is not None else frame, steps, warmup, keep)
    dumped = dump_outputs(snapshot_outputs({"render": keep[0]}), dump) if keep else None
    if player is not None:
        assert player.check(), "a replayed frame was truncated by the frozen pair capacity"
        player.close()
    _lib.prof_enable(True)
    ps = min(steps, 5)
    for _ in range(ps):
        frame()
    torch.cuda.synchronize()
    prof = _lib.prof_table(); _lib.prof_enable(False)
    K, Kref = scene.renderer.last_rasterizer.last_num_pairs
    return {"metric": "config c1 (plumbing): frames/s, %dk random Gaussians, canonical pose, %d^2 raster forward only" % (G // 1000, res),
            "value": steps / dt, "unit": "frames/s", "n_gpus": 1, "steps": steps, "warmup": warmup, "ms_per_step": dt / steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "c1: canonical-pose forward (%d free + %d mesh-bound Gaussians through the encoder / MLPs) + raster forward %dx%d, "
                                   "inference_mode" % (N, M, res, res), "gaussians": G, "resolution": res},
            "roofline": raster_report(prof, G, Kref, K, res * res, ps),
            "launch_mode": "eager" if args.eager else "one hipGraph per frame (player.GraphedAnimation); kernel timers from eager frames after the timed region",
            "kernel_ms_per_step": {k: round(v[1] / ps, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])[:12]}} | ({"dumped_outputs": dumped} if dumped else {})


def _brief(line, keys=("value", "unit", "ms_per_step", "steps", "warmup", "repeats", "launch_mode", "camera", "dtype", "views_per_s", "views_per_step", "config",
                       "roofline", "raster_mpix_per_s", "cpu_baseline", "metric", "redone_frames", "frames_per_launch", "batched_frames", "frozen_avatar_playback")):
    return {k: line[k] for k in keys if k in line}


def flat_scalars(out, cfgs, by):
    """The sub-metrics of BASELINE.json's metric ("...; raster Mpix/s vs HBM roofline") and the other configurations' rates as FLAT top-level
    scalars: a record that keeps only scalar keys of the line still carries them (the nested blocks stay for readers)."""
    def g(d, *path):
        for k in path:
            if not isinstance(d, dict) or d.get(k) is None:
                return None
            d = d[k]
        return d
    rl = out.get("roofline", {})
    c5b = g(cfgs, "c5", "batched_frames")
    flat = {
        "mfma_all_frac": g(rl, "mfma_all", "frac"), "mfma_all_tflops": g(rl, "mfma_all", "tflops"),
        "raster_fwd_ms": g(rl, "raster_forward", "ms"), "raster_fwd_frac": g(rl, "raster_forward", "frac_of_hbm_peak"),
        "raster_fwd_GBps": g(rl, "raster_forward", "achieved_GBps"), "raster_fwd_traffic_ratio": g(rl, "raster_forward", "traffic_over_algorithmic"),
        "raster_bwd_ms": g(rl, "raster_backward", "ms"), "raster_bwd_frac": g(rl, "raster_backward", "frac_of_hbm_peak"),
        "raster_bwd_GBps": g(rl, "raster_backward", "achieved_GBps"), "raster_bwd_traffic_ratio": g(rl, "raster_backward", "traffic_over_algorithmic"),
        "c1_frames_per_s": g(cfgs, "c1", "value"), "c1_raster_fwd_frac": g(cfgs, "c1", "roofline", "raster_forward", "frac_of_hbm_peak"),
        "c2_steps_per_s": g(cfgs, "c2", "value"), "c2_steps_per_s_moving": g(cfgs, "c2_moving_camera", "value"),
        "c2_steps_per_s_eager_launches": g(cfgs, "c2_eager_launches", "value"),
        "c2_steps_per_s_bound_loop": g(cfgs, "c2_bound_loop", "value"),
        "c2_raster_fwd_frac": g(cfgs, "c2", "roofline", "raster_forward", "frac_of_hbm_peak"),
        "c2_raster_bwd_frac": g(cfgs, "c2", "roofline", "raster_backward", "frac_of_hbm_peak"),
        "c3_steps_per_s_bound_loop": g(cfgs, "c3_bound_loop", "value"),
        "c4_n1_views_per_s": g(cfgs, "c4_n1", "views_per_s"), "c4_n1_sequential_views_per_s": g(cfgs, "c4_n1_sequential_views", "views_per_s"),
        "c4_n1_raster_fwd_frac_per_view": g(cfgs, "c4_n1", "roofline", "raster_forward", "frac_of_hbm_peak"),
        "c4_n1_raster_bwd_frac_per_view": g(cfgs, "c4_n1", "roofline", "raster_backward", "frac_of_hbm_peak"),
        "c5_frames_per_s_frame_by_frame": g(cfgs, "c5", "value"), "c5_raster_frac_frame_by_frame": g(cfgs, "c5", "roofline", "raster_forward", "frac_of_hbm_peak"),
        "c5_frames_per_s": g(c5b, "value"), "c5_frames_per_launch": g(c5b, "frames_per_launch"),
        "c5_raster_frac": g(c5b, "roofline", "raster_forward", "frac_of_hbm_peak"), "c5_raster_ms_per_frame": g(c5b, "roofline", "raster_forward", "ms"),
        "c5_frames_per_s_frozen_avatar": g(cfgs, "c5", "frozen_avatar_playback", "value"),
    }
    for d in ("f32", "f16", "bf16"):
        flat["steps_per_s_" + d] = g(by, d, "value")
    return {k: v for k, v in flat.items() if v is not None}


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    assert torch.cuda.is_available(), "bench.py needs a GPU (HIP kernels, no CPU fallback)"
    ctx = Ctx(args)
    if ctx.world != args.gpus and ctx.rank == 0:
        sys.stderr.write("bench.py: --gpus %d but the launcher started %d rank(s); reporting n_gpus=%d\n" % (args.gpus, ctx.world, ctx.world))
    cpu_ok = args.all_configs and not args.no_cpu_baseline and not args.headline_only and ctx.world == 1
    if args.config == "c5":
        out = run_c5(ctx, args.steps, args.warmup, dump=args.dump_outputs)
        if cpu_ok:
            out["cpu_baseline"] = cpu_baseline(out["config"]["gaussians"], out["config"]["resolution"], backward=False, budget_s=6.0, unit="frames/s")
    elif args.config == "c1":
        out = run_c1(ctx, args.steps, args.warmup, dump=args.dump_outputs)
        if cpu_ok:
            out["cpu_baseline"] = cpu_baseline(out["config"]["gaussians"], out["config"]["resolution"], backward=False, canonical=True, budget_s=4.0,
                                               unit="frames/s")
    else:
        full = (args.all_configs and args.config == "c3" and ctx.world == 1 and not args.headline_only and not args.no_guidance and args.dtype == HEADLINE_DTYPE
                and args.gaussians is None and args.res is None and not args.eager)
        pre_cfgs = {}
        if full:
            # the three host-fed configurations (2-ms steps: their rate is the host's enqueue rate) run FIRST, in the state a process of
            # their own would have -- after the denoiser / VAE plans exist, the interpreter's heap holds ~1e5 more objects and the same
            # loops measured 25 % slower (c2: 364 vs 516 steps/s)
            c2 = run_sds(ctx, "c2", steps=200, warmup=20, step_graph=True)        # the whole step replayed as one captured graph per pose
            pre_cfgs["c2"] = _brief(c2)
            c2e = run_sds(ctx, "c2", steps=200, warmup=20, step_graph=False, profile=False)
            pre_cfgs["c2_eager_launches"] = _brief(c2e, ("value", "unit", "ms_per_step", "steps", "warmup", "launch_mode"))
            c2m = run_sds(ctx, "c2", steps=200, warmup=20, step_graph=True, profile=False, moving_camera=True)     # ... with the reference's per-step camera
            pre_cfgs["c2_moving_camera"] = _brief(c2m, ("value", "unit", "ms_per_step", "steps", "warmup", "launch_mode", "camera", "graph_recaptures"))
            c2b = run_sds(ctx, "c2", steps=200, warmup=20, profile=False, bound_loop=True)      # ... driven as the reference's loop drives it through the binding
            pre_cfgs["c2_bound_loop"] = _brief(c2b, ("value", "unit", "ms_per_step", "steps", "warmup", "launch_mode", "camera"))
            c5 = run_c5(ctx, 200, 20)
            c1 = run_c1(ctx, 200, 20)
            if cpu_ok:
                c1["cpu_baseline"] = cpu_baseline(10000, 256, backward=False, canonical=True, budget_s=3.0, unit="frames/s")
                c5["cpu_baseline"] = cpu_baseline(300000, 1024, backward=False, budget_s=5.0, unit="frames/s")
            pre_cfgs["c5"], pre_cfgs["c1"] = _brief(c5), _brief(c1)
            torch.cuda.empty_cache()
        out = run_sds(ctx, args.config, dtype=args.dtype, views=args.views, steps=args.steps, warmup=args.warmup, dump=args.dump_outputs)
        if full:
            # everything the other BASELINE.json configurations and the precision trade need, inside the one line the driver records
            rk = ("kernel", "achieved", "peak", "frac", "mfma_all")
            by = {HEADLINE_DTYPE: _brief(out, ("value", "unit", "ms_per_step", "dtype")) | {"roofline": {k: out["roofline"].get(k) for k in rk}}}
            cfgs = dict(pre_cfgs)
            c3b = run_sds(ctx, "c3", steps=20, warmup=5, profile=False, bound_loop=True)     # the headline workload as a `main.py` user's loop runs it
            cfgs["c3_bound_loop"] = _brief(c3b, ("value", "unit", "ms_per_step", "steps", "warmup", "launch_mode", "camera"))
            c4 = run_sds(ctx, "c4", profile=False)                       # 8 views through ONE VAE / denoiser pass per step; median of 3 x 10 steps
            cfgs["c4_n1"] = _brief(c4)
            ctx.guidance.pop((HEADLINE_DTYPE, 8), None); torch.cuda.empty_cache()
            c4s = run_sds(ctx, "c4", profile=False, batch_views=False, steps=5, repeats=3)   # the same 8 views one guidance call at a time
            cfgs["c4_n1_sequential_views"] = _brief(c4s, ("value", "unit", "ms_per_step", "steps", "warmup", "views_per_s", "repeats"))
            ctx.guidance.pop(HEADLINE_DTYPE, None); torch.cuda.empty_cache()
            f32 = run_sds(ctx, "c3", dtype="f32", steps=5, warmup=2)
            by["f32"] = _brief(f32, ("value", "unit", "ms_per_step", "steps", "warmup", "dtype")) | {"roofline": {k: f32["roofline"].get(k) for k in rk},
                                                                                                     "config": f32["config"]}
            ctx.guidance.pop("f32", None)                         # free the fp32 plans (weights 5 GB, activations) before the other legs
            torch.cuda.empty_cache()
            for dtn in ("f16", "bf16"):
                o = run_sds(ctx, "c3", dtype=dtn, steps=20, warmup=5)
                by[dtn] = _brief(o, ("value", "unit", "ms_per_step", "steps", "warmup", "dtype")) | {"roofline": {k: o["roofline"].get(k) for k in rk},
                                                                                                     "config": o["config"]}
                ctx.guidance.pop(dtn, None)
                torch.cuda.empty_cache()
            by["note"] = ("same workload, same kernels outside the denoiser / VAE.  f32x (the headline) = the reference's precision for this stage "
                          "(fp32: configs/__init__.py:236,241) as split-precision hi + lo fp16 planes, three f16 MFMAs per product, flops counted "
                          "ONCE against the 2.5 PFLOP/s peak; f32 = exact-f32 MFMA (peak 157 TFLOP/s); f16 = its --guide.dtype fp16 storage type; "
                          "bf16 = reduced precision (eps 1.5 %, SDS gradient 4 % off).  Parity against the fp32 CPU oracle: "
                          "tests/test_sd15_f32x_gpu.py, test_sd15_fp32_gpu.py, test_sd15_fp16_gpu.py, test_sd15_full_width_gpu.py")
            out["by_dtype"] = by
            out["configs"] = cfgs
            out.update(flat_scalars(out, cfgs, by))
            # the per-precision rates right behind "dtype", so that they are inside the head of the line whatever its length
            head = {}
            for k, v in out.items():
                head[k] = v
                if k == "dtype":
                    head["steps_per_s_by_dtype"] = {d: round(by[d]["value"], 2) for d in (HEADLINE_DTYPE, "f32", "f16", "bf16")}
            out = head
        if cpu_ok and ctx.rank == 0 and args.config in ("c2", "c3"):
            out["cpu_baseline"] = cpu_baseline(out["config"]["gaussians"], out["config"]["resolution"])
    if ctx.rank == 0:
        if not (args.headline_only or args.all_configs):
            # the default line stays short (about 2 KB): the per-kernel blocks give way to their headline numbers
            out = {k: v for k, v in out.items() if k not in ("roofline", "kernel_ms_per_step")} | flat_scalars(out, {}, {})
        print(json.dumps(out), flush=True)
    if ctx.dist is not None:
        ctx.dist.destroy_process_group()


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--_cpu-worker":
        _cpu_worker(json.loads(sys.argv[2]))
    else:
        main()
