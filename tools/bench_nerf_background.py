"""Times the learned background of stage I (boundary B22) at 64^2, 256^2 and 512^2 rays, rgb (C = 3, sigmoid) and latent (C = 4,
identity), fp32 and fp16:

  native     nerf_background.learned_background: one launch forward, two backward, nothing kept but rays_d and the parameters
  torch      the composition it replaces: the frequency encoding restated in torch (sin / cos of 2^f x, concatenated), bg_net
             (Linear + ReLU, the last layer without), the sigmoid; under fp16 the same statements inside torch.autocast

    python tools/bench_nerf_background.py [--sizes 64,256,512] [--repeats 50] [--warmup 5] [--timeout 240]

Per row the torch form runs FIRST and LAST with the native form between them, so the output carries the torch form's own run-to-run
spread; every figure is min / median / max of host-clock times around a device synchronise, after warm-up calls of the same shape.
"fwd" is the forward under no_grad; "f+b" the forward with gradients on and the backward of a fixed cotangent.  The ratio is
native / torch on the medians: nothing asserts it.  Each size runs in a child process of its own under --timeout seconds, and a child
that fails or runs out of time ends the run: nothing more is started on the GPU after it.  Needs a GPU."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"


def torch_freq_encode(x, degree):
    import torch
    cols = [x]
    for f in range(degree):
        v = x * (2.0 ** f)
        cols += [torch.sin(v), torch.cos(v)]
    return torch.cat(cols, -1)


def timed(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def fmt(ts):
    return "%8.3f /%8.3f /%8.3f" % (min(ts), statistics.median(ts), max(ts))


def rows(res, repeats, warmup):
    """The rows of one size, in this process."""
    import numpy as np
    import torch
    import dwg_import  # noqa: F401
    from dreamwaltz_g_amd import nerf_background, nerf_model
    if not torch.cuda.is_available():
        raise SystemExit("bench_nerf_background needs a GPU: a CPU run says nothing about the kernels' time")
    N = res * res
    r = np.random.RandomState(res).randn(N, 3)
    rays_d = torch.from_numpy((r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)).to(DEV)
    enc = nerf_background.FreqEncoder(3, 6)
    for C, sigmoid, name in ((3, True, "rgb"), (4, False, "latent")):
        torch.manual_seed(C)
        bg_net = nerf_model.MLP(enc.output_dim, C, 64, 2, bias=True).to(DEV)
        cot = torch.randn(N, C, device=DEV)
        for precision, pname in ((0, "fp32"), (1, "fp16")):
            def composition():
                h = bg_net(torch_freq_encode(rays_d, enc.degree))
                return torch.sigmoid(h) if sigmoid else h

            def torch_form():
                if precision:
                    with torch.autocast('cuda', dtype=torch.float16):
                        return composition()
                return composition()

            def native_form():
                return nerf_background.learned_background(rays_d, enc, bg_net, sigmoid=sigmoid, precision=precision)

            def fwd(form):
                def run():
                    with torch.no_grad():
                        form()
                return run

            def fb(form):
                def run():
                    for p in bg_net.parameters():
                        p.grad = None
                    out = form()
                    out.backward(cot.to(out.dtype))
                return run
            for what, wrap in (("fwd", fwd), ("f+b", fb)):
                first = timed(wrap(torch_form), warmup, repeats)
                nat = timed(wrap(native_form), warmup, repeats)
                last = timed(wrap(torch_form), warmup, repeats)
                tmed = statistics.median(first + last)
                print("%4d^2 %-6s %s %s  torch (first) %s | native %s | torch (last) %s | native / torch %.3f; torch first-to-last spread %.3f ms" % (
                    res, name, pname, what, fmt(first), fmt(nat), fmt(last), statistics.median(nat) / tmed,
                    abs(statistics.median(first) - statistics.median(last))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,512")
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for one size's child process")
    ap.add_argument("--size", type=int, default=None, help="(internal) run the rows of this size in this process")
    args = ap.parse_args()
    if args.size is not None:
        return rows(args.size, args.repeats, args.warmup)
    print("== python tools/bench_nerf_background.py " + " ".join(sys.argv[1:]))
    print("bg_net 39 -> 64 -> C (2 layers), degree 6; times in ms, min / median / max of %d calls after %d warm-up calls" % (args.repeats, args.warmup),
          flush=True)
    for res in [int(s) for s in args.sizes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(res), "--repeats", str(args.repeats), "--warmup", str(args.warmup)]
        try:
            r = subprocess.run(cmd, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit("size %d ran out of its %d s: nothing more is started" % (res, args.timeout))
        if r.returncode != 0:
            raise SystemExit("size %d ended with status %d: nothing more is started" % (res, r.returncode))


if __name__ == "__main__":
    main()
