"""Times the native VAE decoder (boundary B26: sd15.VAEDecoderPlan.decode, what `decode_latents` runs) at SD-1.5's full width, latent
64 x 64 -> image 512 x 512, batch 1, in the four plan precisions.

    python tools/bench_vae_decoder.py [--reps 20] [--rounds 3] [--latent 64] [--out profiles/b26_bench_vae_decoder.txt]

Each precision is timed as its user runs it: the captured plan replayed on a side stream, boundary conversions included (for f32x the two
one-launch converters, for the others the torch statements `decode` makes).  Times are HIP-event milliseconds per decode over --reps
back-to-back decodes, the median of --rounds rounds after one warm-up round.

Beside it, on the same card in the same process, the same graph written with torch-ROCm operators in fp32: a LABELLED TORCH RESTATEMENT
(tests/vae_decoder_cases.decode_oracle on device tensors: F.conv2d / F.group_norm / F.silu / F.scaled_dot_product_attention /
F.interpolate, then x / 2 + 0.5 and the clamp).  diffusers is not a dependency of this project, so its own modules are not what is timed;
the restatement makes the operator calls AutoencoderKL.decode makes for this configuration, eagerly, which is what `decode_latents` costs a
user of the reference's path today.  It is timed before AND after the native runs (two figures, so that clock drift shows).  Weights are
seeded random ones: no checkpoint is read, and the arithmetic does not depend on the values.  No bar is set on either figure.  The last
line is the table as JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import sd15  # noqa: E402
from tests import vae_decoder_cases as vc  # noqa: E402


def _event_ms(fn, reps, rounds, stream):
    """Median over `rounds` of (event time of `reps` back-to-back calls) / reps, on `stream`, after one warm-up round."""
    out = []
    with torch.cuda.stream(stream):
        for r in range(rounds + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(reps):
                fn()
            b.record(stream)
            b.synchronize()
            if r > 0:
                out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), [round(v, 4) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--dtypes", default="f32x,f32,f16,bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vae_decoder.py needs a GPU"
    dev = torch.device("cuda")
    cfg = sd15.VAEConfig()
    sd = sd15.random_state_dict(sd15.vae_decoder_param_shapes(cfg), seed=3)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, cfg.latent_channels, args.latent, args.latent, generator=g).to(dev)
    stream = torch.cuda.Stream()
    lines, table = [], {"latent_hw": args.latent, "image_hw": args.latent * 2 ** (len(cfg.block_out_channels) - 1), "batch": 1,
                        "reps": args.reps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "native_ms": {}, "torch_fp32_ms": {}}

    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    torch.cuda.synchronize()

    def torch_decode():
        with torch.no_grad():
            return vc.postprocess(vc.decode_oracle(cfg, sd_dev, lat))

    def time_torch(label):
        ms, rounds = _event_ms(torch_decode, args.reps, args.rounds, stream)
        table["torch_fp32_ms"][label] = ms
        lines.append("torch-ROCm fp32 restatement (eager, %s the native runs): %8.3f ms per decode   rounds %s" % (label, ms, rounds))

    time_torch("before")
    ref = torch_decode().double()
    for dt in args.dtypes.split(","):
        plan = sd15.VAEDecoderPlan(cfg, sd, dev, latent_hw=args.latent, dtype=dt, batch=1)
        plan.capture()
        ms, rounds = _event_ms(lambda: plan.decode(lat), args.reps, args.rounds, stream)
        with torch.cuda.stream(stream):
            img = plan.decode(lat)
        stream.synchronize()
        err = float((img.double() - ref).abs().max())
        launches = sum(1 for op in plan.plan.ops if op[0] != "fork")
        table["native_ms"][dt] = ms
        lines.append("native %-4s (graph replay, %3d launches + converters): %8.3f ms per decode   rounds %s   max |image - torch fp32| %.2e"
                     % (dt, launches, ms, rounds, err))
        del plan
        torch.cuda.empty_cache()
    time_torch("after")
    t = 0.5 * (table["torch_fp32_ms"]["before"] + table["torch_fp32_ms"]["after"])
    for dt, ms in table["native_ms"].items():
        lines.append("torch fp32 / native %-4s: %.2fx" % (dt, t / ms))
    head = ["VAE decoder, SD-1.5 width %s, latent %d -> %d x %d, batch 1, %s" % (cfg.block_out_channels, args.latent, table["image_hw"],
                                                                                table["image_hw"], table["device"]),
            "HIP-event time per decode, %d decodes per round, median of %d rounds after one warm-up round" % (args.reps, args.rounds)]
    text = "\n".join(head + lines + [json.dumps(table)])
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
