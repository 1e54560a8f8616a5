"""Times of the stage-II learned MLP background (boundary B23) on the GPU: python tools/bench_mlp_background.py [--steps 50] [--warmup 5]

  1. the background's forward and forward + backward at 64^2, 256^2, 512^2: background.MLPBackground (directions kernel + the fused
     encoding / network / sigmoid kernels) against the same statements composed in torch on the device;
  2. the Adan step at the background's 499 parameters and at 1 M and 16 M elements: optim.FlatAdan (three launches, no host read)
     against the optimizer's statements composed in torch, INCLUDING the reference's host read of the clipping factor (.item());
  3. the stage-II step through SDSTrainer with a stub guidance (loss = sum(image * W)), with and without the background.

Every form is called --warmup times, then --steps times with a device synchronisation before and after each call (wall clock, ms):
min / median / max.  Before the first timed case of a section both of its forms run 200 untimed calls (clocks, allocator and code loading
settle before anything is timed).  The comparison form runs first and last around the native one; the first-to-last spread of its medians is printed
as the drift of the machine during the measurement.  Nothing here is a pass / fail check."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import background as bgm  # noqa: E402
from dreamwaltz_g_amd import camera, configs, optim, scene as sc, sds_step, synth, trainer as tr  # noqa: E402

DEV = torch.device("cuda:0")
SETTLE = 200          # untimed calls of both forms before a section's first timed case


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out), float(np.median(out)), max(out)


def fmt(t):
    return "%8.3f / %8.3f / %8.3f" % t


def sandwich(label, first_name, other, native, steps, warmup):
    a = timed(other, steps, warmup)
    n = timed(native, steps, warmup)
    b = timed(other, steps, warmup)
    base = 0.5 * (a[1] + b[1])
    print("%s %s (first) %s | native %s | %s (last) %s | native / %s %.3f; first-to-last spread %.3f ms"
          % (label, first_name, fmt(a), fmt(n), first_name, fmt(b), first_name, n[1] / base, abs(a[1] - b[1])))


def torch_dirs(c2w, K, H, W):
    j, i = torch.meshgrid(torch.arange(H, device=DEV, dtype=torch.float32), torch.arange(W, device=DEV, dtype=torch.float32), indexing='ij')
    i, j = i.reshape(1, -1) + 0.5, j.reshape(1, -1) + 0.5
    d = torch.stack([(i - K[:, 0, 2:3]) / K[:, 0, 0:1], (j - K[:, 1, 2:3]) / K[:, 1, 1:2], torch.ones_like(i)], -1)
    d = d / torch.sqrt(torch.clamp((d * d).sum(-1, keepdim=True), min=1e-20))
    d = d @ c2w[:, :3, :3].transpose(-1, -2)
    return (d / torch.norm(d, dim=-1, keepdim=True)).reshape(-1, 3)


def torch_image(bg, data):
    d = torch_dirs(data['c2w'], data['intrinsics'], data['image_height'], data['image_width'])
    cols = [d]
    for f in range(4):
        cols += [torch.sin(d * 2.0 ** f), torch.cos(d * 2.0 ** f)]
    h = torch.relu(torch.nn.functional.linear(torch.cat(cols, -1), bg.bg_net.net[0].weight, bg.bg_net.net[0].bias))
    return torch.sigmoid(torch.nn.functional.linear(h, bg.bg_net.net[1].weight, bg.bg_net.net[1].bias))


def cam(res):
    data = dict(camera.make_camera(radius=2.0, azimuth=20.0, elevation=80.0, fovy=55.0, height=res, width=res, device=DEV))
    fl = 0.5 * res / float(data["tanfov"][0])
    data["intrinsics"] = torch.tensor([[[fl, 0.0, 0.5 * res], [0.0, fl, 0.5 * res], [0.0, 0.0, 1.0]]], device=DEV)
    return data


def bench_background(steps, warmup):
    warm = False
    print("MLPBackground: degree-4 encoding, 27 -> 16 -> 3, sigmoid; times in ms, min / median / max of %d calls after %d warm-up calls" % (steps, warmup))
    bg = bgm.MLPBackground().to(DEV)
    for res in (64, 64, 256, 512):                     # the first pass at 64^2 is the section's untimed warm-up
        data = cam(res)
        cot = torch.randn(res * res, 3, device=DEV)

        def fb(fn):
            for p in bg.parameters():
                p.grad = None
            fn().reshape(-1, 3).backward(cot)
        if not warm:
            for _ in range(SETTLE):
                fb(lambda: torch_image(bg, data))
                fb(lambda: bg(data))
            torch.cuda.synchronize()
            warm = True
            continue
        with torch.no_grad():
            sandwich("%4d^2 fwd " % res, "torch", lambda: torch_image(bg, data), lambda: bg(data), steps, warmup)
        sandwich("%4d^2 f+b " % res, "torch", lambda: fb(lambda: torch_image(bg, data)), lambda: fb(lambda: bg(data)), steps, warmup)


class TorchAdan:
    """The optimizer's statements composed in torch on one flat tensor, with the reference's host read of the clipping factor."""

    def __init__(self, p, lr=1e-3, betas=(0.98, 0.92, 0.99), eps=1e-8, wd=2e-5, mgn=5.0):
        self.p, self.g = p, torch.zeros_like(p)
        self.m, self.n, self.v, self.q = (torch.zeros_like(p) for _ in range(4))
        self.lr, self.betas, self.eps, self.wd, self.mgn, self.t = lr, betas, eps, wd, mgn, 0

    @torch.no_grad()
    def step(self):
        b1, b2, b3 = self.betas
        norm = torch.sqrt(self.g.pow(2).sum())
        clip = torch.clamp(torch.tensor(self.mgn, device=DEV) / (norm + self.eps), max=1.0).item()
        self.t += 1
        t = self.t
        g = self.g.mul_(clip)
        if t == 1:
            self.q = g.clone().mul_(-1.0)
        q = self.q
        q.add_(g)
        self.m.mul_(b1).add_(g, alpha=1 - b1)
        self.v.mul_(b2).add_(q, alpha=1 - b2)
        q.mul_(b2).add_(g)
        self.n.mul_(b3).addcmul_(q, q, value=1 - b3)
        den = (self.n.sqrt() / (1 - b3 ** t) ** 0.5).add_(self.eps)
        self.p.addcdiv_(self.m, den, value=-self.lr / (1 - b1 ** t))
        self.p.addcdiv_(self.v, den, value=-self.lr * b2 / (1 - b2 ** t))
        self.p.div_(1 + self.lr * self.wd)
        q.zero_().add_(g, alpha=-1.0)


def bench_adan(steps, warmup):
    print("Adan step (lr 1e-3, weight_decay 2e-5, max_grad_norm 5): torch = the statements composed in torch with the host read of the clipping factor")
    for n, label in ((499, "   499 (the background)"), (1 << 20, "    1 M"), (1 << 24, "   16 M")):
        g = torch.randn(n, device=DEV) * 0.01
        ta = TorchAdan(torch.randn(n, device=DEV))
        p = torch.nn.Parameter(torch.randn(n, device=DEV))
        fa = optim.FlatAdan(optim.AdanSpec([{'params': [p]}], lr=1e-3, eps=1e-8, weight_decay=2e-5, max_grad_norm=5.0), DEV)

        def torch_step():
            ta.g.copy_(g)
            ta.step()

        def native_step():
            p.grad.copy_(g)
            fa.step()
        if n == 499:
            for _ in range(SETTLE):
                torch_step()
                native_step()
            torch.cuda.synchronize()
        sandwich("%-24s" % label, "torch", torch_step, native_step, steps, warmup)
        del ta, fa, p, g
        torch.cuda.empty_cache()


def bench_step(steps, warmup, G=100000, res=512):
    print("stage-II step through SDSTrainer, stub guidance (loss = sum(image * W)), %d Gaussians at %d^2" % (G, res))

    def build(with_bg):
        cfg = configs.TrainConfig(); cfg.device = str(DEV); cfg.render.bg_color = (0.5, 0.5, 0.5)
        cfg.prompt.text_augmentation = False
        avatar, _, _ = sds_step.build_synthetic_avatar(G, DEV, seed=0)
        opts = avatar.get_optimizer(cfg)
        bg = bgm.MLPBackground().to(DEV) if with_bg else None
        scene = sc.Scene(cfg, avatar, background=bg, async_pair_count=True).to(DEV).train()
        if with_bg:
            opts['background'] = bg.get_optimizer(cfg)
        wimg = torch.randn(1, res, res, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
        t = tr.SDSTrainer(cfg, scene, sds_step._ImageLoss(wimg), opts, {}, use_controlnet=False, max_step=10000)
        data = cam(res)
        data['smpl_inputs'] = synth.random_smpl_inputs(seed=1, device=DEV)
        return lambda: t.train_step(data)
    plain, with_bg = build(False), build(True)
    for _ in range(SETTLE):
        plain()
        with_bg()
    torch.cuda.synchronize()
    a = timed(plain, steps, warmup)
    n = timed(with_bg, steps, warmup)
    b = timed(plain, steps, warmup)
    base = 0.5 * (a[1] + b[1])
    print("  without (first) %s | with the background %s | without (last) %s | with - without %+.3f ms (medians); first-to-last spread %.3f ms"
          % (fmt(a), fmt(n), fmt(b), n[1] - base, abs(a[1] - b[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    print("== python tools/bench_mlp_background.py --steps %d --warmup %d" % (args.steps, args.warmup))
    bench_background(args.steps, args.warmup)
    bench_adan(args.steps, args.warmup)
    bench_step(args.steps, args.warmup)


if __name__ == "__main__":
    main()
