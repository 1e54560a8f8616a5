"""Times the stage-I (NeRF) training step (boundary B20) with a stub guidance -- a fixed seeded image gradient, so the number isolates
the NeRF side -- at 64^2, 128^2, 256^2 and 512^2:

  native     nerf_trainer.NeRFSDSTrainer.train_step: view_rays -> render_rays_train -> view_compose (mix + planar image + sparsity loss)
             -> backward -> the flat fused Adam
  composed   the same step from the parent commit's public pieces: a torch restatement of get_rays, raymarch.near_far_from_aabb,
             render_rays_train, a torch mix + permute + SparsityLoss, torch.optim.Adam
  view       the two view kernels alone against their torch compositions (rays + near/far; compose forward + backward)

    python tools/bench_nerf_step.py [--sizes 64,128,256,512] [--repeats 20] [--warmup 3] [--guidance] [--profile] [--fp16] [--bg-mode nerf]

Per size the composed form runs FIRST and LAST with the native form between them, so the output carries the composed form's own
run-to-run spread; every figure is min / median / max of host-clock times around a device synchronise, after warm-up steps of the same
shape.  Both forms render the same network, grid and camera with the same perturbation; the occupancy update is kept out of the timed
steps (it is B13's, and the same in both forms).  --profile adds torch launches per step for both forms (torch.profiler, a pass of its
own).  --guidance adds, at 512^2, the native step with the real guidance object (full-width random weights).

--fp16 (boundary B21) times instead, per size, the step under cfg.optim.fp16 in two forms that share every kernel but the scaler's:
  native fp16     NeRFSDSTrainer.train_step with grad_scaler.FlatGradScaler: scan, decision, unscale, step counts and scale on the device
  torch scaler    the same forward under autocast with torch.amp.GradScaler('cuda') driving the same kind of FlatOptimizer (unscale_ over
                  its .grad views, the found_inf read on the host, then FlatOptimizer.step()): the composition the device scaler replaces
Each form steps a network and optimizer of its own from the same state; "torch scaler" runs first and last.

--bg-mode nerf (boundary B22) times the same forms with the learned background: the native step on nerf_model.BackgroundNeRFNetwork
(nerf_background.learned_background, the 'bg_net' group in the flat Adam), the composed step with the frequency encoding restated in
torch, bg_net, the sigmoid and a fourth torch.optim.Adam group.  Needs a GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import configs, nerf_model, nerf_render, nerf_trainer, nerf_view, raymarch  # noqa: E402

DEV = "cuda"
LAMBDAS = (5e-3, 1e-3, 0.5)


def make_cfg(bg_mode='gray'):
    cfg = configs.TrainConfig()
    cfg.stage, cfg.device = 'nerf', DEV
    cfg.nerf = configs.NeRFConfig(bound=2.0, grid_size=128, density_prior='gaussian', lambda_opacity=LAMBDAS[0], lambda_entropy=LAMBDAS[1],
                                  lambda_emptiness=LAMBDAS[2], update_extra_interval=1 << 30, bg_mode=bg_mode)
    cfg.prompt.text_augmentation = False
    cfg.optim.iters = 10000
    return cfg


def make_network(cfg, seed=0):
    net = nerf_model.build_nerf_network(cfg.nerf)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        net.encoder.embeddings.copy_((torch.rand(net.encoder.embeddings.shape, generator=g) * 2 - 1) * 0.1)
        for lin in list(net.sigma_net.net) + (list(net.bg_net.net) if net.bg_net is not None else []):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * (1.0 / lin.in_features) ** 0.5)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return net.to(DEV).train()


def camera(res, bound):
    """A camera 3.2 bounds from the origin looking at it, 50 degrees across."""
    a, b = 0.3, -0.6
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    R = Ry @ Rx
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = R, -R[:, 2] * 3.2 * bound
    f = 0.5 * res / np.tan(np.radians(25.0))
    K = np.array([[f, 0, 0.5 * res], [0, f, 0.5 * res], [0, 0, 1]])
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)[None]    # noqa: E731
    return {'c2w': t(c2w), 'intrinsics': t(K), 'image_height': res, 'image_width': res, 'body_part': 'full'}


def torch_get_rays(c2w, intrinsics, H, W):
    """get_rays with N = -1 (core/nerf/nerf_utils.py:72-137), the reference's torch statements."""
    device = c2w.device
    B = c2w.shape[0]
    fx, fy = intrinsics[:, 0, 0], intrinsics[:, 1, 1]
    cx, cy = intrinsics[:, 0, 2], intrinsics[:, 1, 2]
    i, j = torch.meshgrid(torch.linspace(0, W - 1, W, device=device), torch.linspace(0, H - 1, H, device=device), indexing='ij')
    i = i.t().reshape([1, H * W]).expand([B, H * W]) + 0.5
    j = j.t().reshape([1, H * W]).expand([B, H * W]) + 0.5
    zs = torch.ones_like(i)
    xs = (i - cx) / fx * zs
    ys = (j - cy) / fy * zs
    directions = torch.stack((xs, ys, zs), dim=-1)
    directions = directions / torch.sqrt(torch.clamp(torch.sum(directions * directions, -1, keepdim=True), min=1e-20))
    rays_d = directions @ c2w[:, :3, :3].transpose(-1, -2)
    rays_o = c2w[..., :3, 3]
    rays_o = rays_o[..., None, :].expand_as(rays_d)
    return rays_o, rays_d


def torch_freq_encode(x, degree):
    """The frequency encoding (FreqEncoder's layout) in torch: x, then per frequency the sines and the cosines of 2^f x."""
    cols = [x]
    for f in range(degree):
        v = x * (2.0 ** f)
        cols += [torch.sin(v), torch.cos(v)]
    return torch.cat(cols, -1)


def torch_sparsity(ws):
    lo, le, lm = LAMBDAS
    al = ws.clamp(1e-6, 1 - 1e-6)
    loss = 0.0
    loss += lo * torch.sqrt((ws ** 2 + 0.01).mean())
    loss += le * (- al * torch.log2(al) - (1 - al) * torch.log2(1 - al)).mean()
    loss += lm * (10000 * torch.log(1 + 10 * ws).mean())
    return loss


class Stub:
    def __init__(self, res):
        self.G = torch.randn(1, 3, res, res, generator=torch.Generator().manual_seed(res)).to(DEV)

    def __call__(self, inputs, **kwargs):
        return {"diffusion_loss": (inputs * self.G).sum().reshape(1)}


class Composed:
    """The step from the parent commit's public pieces, on a network of its own with the native one's parameters and grid."""

    def __init__(self, cfg, src, stub):
        self.net = make_network(cfg)
        self.net.load_state_dict(src.state_dict())
        n = self.net
        groups = [{'params': n.encoder.parameters(), 'lr': cfg.nerf.lr * 10}, {'params': n.sigma_net.parameters(), 'lr': cfg.nerf.lr},
                  {'params': n.sigma_scale, 'lr': cfg.nerf.lr}]
        if n.bg_net is not None:
            groups.append({'params': n.bg_net.parameters(), 'lr': cfg.nerf.bg_lr})
        self.opt = torch.optim.Adam(groups, betas=(0.9, 0.99), eps=1e-15)
        self.stub, self.bg = stub, torch.tensor([0.5, 0.5, 0.5])

    def step(self, data, noises):
        n = self.net
        H, W = data['image_height'], data['image_width']
        rays_o, rays_d = torch_get_rays(data['c2w'], data['intrinsics'], H, W)
        rays_o, rays_d = rays_o.contiguous().view(-1, 3), rays_d.contiguous().view(-1, 3)
        nears, fars = raymarch.near_far_from_aabb(rays_o, rays_d, n.aabb_train)
        counter = n.step_counter[n.local_step % 16]
        counter.zero_()
        n.local_step += 1
        ws, depth, image = nerf_render.render_rays_train(
            rays_o, rays_d, nears, fars, n.density_bitfield, n.cascade, n.grid_size, n.encoder, n.sigma_net, n.sigma_scale, n.bound,
            density_activation=n.opt.density_activation, density_prior=n.density_prior_type, albedo_sigmoid=True, perturb=True, noises=noises,
            counter=counter)
        image_fg, ws4 = image.reshape(1, H, W, -1), ws.reshape(1, H, W, 1)
        if n.bg_mode == 'nerf':
            image_bg = torch.sigmoid(n.bg_net(torch_freq_encode(rays_d, n.encoder_bg.degree))).reshape_as(image_fg)
        else:
            image_bg = self.bg.to(image_fg).expand_as(image_fg)
        image = image_fg + (1 - ws4) * image_bg
        sd_inputs = image.permute(0, 3, 1, 2).contiguous()
        loss = self.stub(sd_inputs)['diffusion_loss'] * 1.0 + torch_sparsity(ws4)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss


class TorchScalerStep:
    """The fp16 step with torch.amp.GradScaler('cuda') around the flat optimizers instead of grad_scaler.FlatGradScaler."""

    def __init__(self, tr):
        self.tr, self.ts = tr, torch.amp.GradScaler('cuda')

    def step(self, data, noises):
        tr = self.tr
        with torch.autocast('cuda', dtype=torch.float16):
            tr.train_step_index += 1
            out = tr.train_forward(data, render_kwargs=dict(noises=noises))
        for optimizer in tr.optimizers.values():
            optimizer.zero_grad()
        self.ts.scale(out[0]).backward()
        for optimizer in tr.optimizers.values():
            self.ts.step(optimizer)
        self.ts.update()
        return out


def fp16_rows(args, cfg, net):
    """The --fp16 table: both forms on networks of their own that start from `net`'s parameters and occupancy grid."""
    cfg.optim.fp16 = True
    text = {'pos': torch.zeros(1, 77, 8, device=DEV)}
    print("size   form                 step ms min / median / max      scale after the run (2^16 at its start; halved by every skipped step)")
    for res in [int(s) for s in args.sizes.split(",")]:
        data = camera(res, net.bound)
        noises = torch.rand(res * res, generator=torch.Generator().manual_seed(res)).to(DEV)
        stub = Stub(res)
        forms = []
        for _ in range(2):
            n = make_network(cfg)
            n.load_state_dict(net.state_dict())
            o, _s = n.get_optimizer(cfg.nerf)
            tr = nerf_trainer.NeRFSDSTrainer(cfg, n, stub, o, text_embeds_dict=dict(text), use_controlnet=False)
            tr.train_step_index = 1                            # the occupancy update ran before; none inside the timed steps
            forms.append(tr)
        nat, comp = forms[0], TorchScalerStep(forms[1])

        def native_step():
            return nat.train_step(data, render_kwargs=dict(noises=noises))

        def torch_scaler_step():
            return comp.step(data, noises)
        first = timed(torch_scaler_step, args.warmup, args.repeats)
        mid = timed(native_step, args.warmup, args.repeats)
        last = timed(torch_scaler_step, args.warmup, args.repeats)
        for name, ts, sc in (("torch scaler (first)", first, None), ("native fp16", mid, nat.scaler.get_scale()),
                             ("torch scaler (last)", last, comp.ts.get_scale())):
            print("%4d^2 %-20s %s   %s" % (res, name, fmt(ts), "" if sc is None else "%g" % sc))
        spread = abs(statistics.median(first) - statistics.median(last))
        cmed = statistics.median(first + last)
        print("       native fp16 / torch scaler %.3f (medians; torch scaler = both runs); torch scaler first-to-last spread %.3f ms; "
              "native - torch scaler %+.3f ms" % (statistics.median(mid) / cmed, spread, statistics.median(mid) - cmed))
        if args.profile:
            nk, no = launches(native_step)
            ck, co = launches(torch_scaler_step)
            print("       launches per step: native fp16 %d device kernels (%d top-level aten ops), torch scaler %d (%d)" % (nk, no, ck, co))


def timed(fn, warmup, repeats):
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


def launches(fn):
    """Device kernels of one call (HIP-library launches included) and the top-level aten ops among them."""
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    nk, ops = 0, 0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            nk += 1
        elif e.name.startswith("aten::") and (e.cpu_parent is None or not e.cpu_parent.name.startswith("aten::")):
            ops += 1
    return nk, ops


def view_alone(data, net, warmup, repeats):
    """The two view kernels against their torch compositions, on this size's rays and a seeded render-shaped input."""
    H, W = data['image_height'], data['image_width']
    N = H * W
    g = torch.Generator().manual_seed(N)
    fg = torch.rand(1, H, W, 3, generator=g).to(DEV)
    ws = torch.rand(1, H, W, 1, generator=g).to(DEV)
    G = torch.randn(1, 3, H, W, generator=g).to(DEV)
    bg = torch.tensor([0.5, 0.5, 0.5], device=DEV)
    sp = LAMBDAS + (1.0,)

    def rays_native():
        nerf_view.view_rays(data['c2w'], data['intrinsics'], H, W, net.aabb_train)

    def rays_torch():
        o, d = torch_get_rays(data['c2w'], data['intrinsics'], H, W)
        raymarch.near_far_from_aabb(o.contiguous().view(-1, 3), d.contiguous().view(-1, 3), net.aabb_train)

    def compose_native():
        a, b = fg.clone().requires_grad_(True), ws.clone().requires_grad_(True)
        image, loss = nerf_view.view_compose(a, b, bg, H, W, sparsity=sp)
        ((image * G).sum() + loss).backward()

    def compose_torch():
        a, b = fg.clone().requires_grad_(True), ws.clone().requires_grad_(True)
        image = (a + (1 - b) * bg.expand_as(a)).permute(0, 3, 1, 2).contiguous()
        ((image * G).sum() + torch_sparsity(b)).backward()
    return {k: timed(f, warmup, repeats) for k, f in (("rays native", rays_native), ("rays torch", rays_torch),
                                                      ("compose f+b native", compose_native), ("compose f+b torch", compose_torch))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256,512")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--guidance", action="store_true", help="at 512^2, also the native step with the real guidance object")
    ap.add_argument("--profile", action="store_true", help="torch launches per step for both forms (a pass of its own)")
    ap.add_argument("--fp16", action="store_true", help="the step under optim.fp16: the device-resident scaler against torch.amp.GradScaler")
    ap.add_argument("--bg-mode", default="gray", choices=["gray", "nerf"], help="'nerf': the learned background in both forms")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nerf_step needs a GPU: a CPU run says nothing about the step's time")
    print("== python tools/bench_nerf_step.py " + " ".join(sys.argv[1:]))
    torch.manual_seed(0)
    cfg = make_cfg(args.bg_mode)
    net = make_network(cfg)
    net.update_extra_state()
    opts, _ = net.get_optimizer(cfg.nerf)
    print("network: bound %g, grid %d^3 x %d cascades, %d table rows; occupied cells %d; lambdas %s; background %r; stub guidance" % (
        net.bound, net.grid_size, net.cascade, net.encoder.embeddings.shape[0],
        int(torch.tensor([bin(v).count("1") for v in range(256)], device=DEV)[net.density_bitfield.long()].sum()), LAMBDAS, net.bg_mode))
    if args.fp16:
        return fp16_rows(args, cfg, net)
    print("size   form                 step ms min / median / max      M samples (each form's own count, last step of the run)")
    for res in [int(s) for s in args.sizes.split(",")]:
        data = camera(res, net.bound)
        noises = torch.rand(res * res, generator=torch.Generator().manual_seed(res)).to(DEV)
        stub = Stub(res)
        tr = nerf_trainer.NeRFSDSTrainer(cfg, net, stub, opts, text_embeds_dict={'pos': torch.zeros(1, 77, 8, device=DEV)}, use_controlnet=False)
        tr.train_step_index = 1                                # the occupancy update ran above; none inside the timed steps
        comp = Composed(cfg, net, stub)

        def native_step():
            return tr.train_step(data, render_kwargs=dict(noises=noises))

        def composed_step():
            return comp.step(data, noises)
        def samples(n):
            """What the last march of network n added to its own step counter: the samples M of that run's last step."""
            return int(n.step_counter[(n.local_step - 1) % 16, 0])
        first = timed(composed_step, args.warmup, args.repeats)
        m_first = samples(comp.net)
        nat = timed(native_step, args.warmup, args.repeats)
        m_nat = samples(net)
        last = timed(composed_step, args.warmup, args.repeats)
        m_last = samples(comp.net)
        for name, ts, M in (("composed (first)", first, m_first), ("native", nat, m_nat), ("composed (last)", last, m_last)):
            print("%4d^2 %-18s %s   %10d" % (res, name, fmt(ts), M))
        spread = abs(statistics.median(first) - statistics.median(last))
        cmed = statistics.median(first + last)
        print("       native / composed %.3f (medians; composed = both runs); composed first-to-last spread %.3f ms; native - composed %+.3f ms" % (
            statistics.median(nat) / cmed, spread, statistics.median(nat) - cmed))
        va = view_alone(data, net, args.warmup, args.repeats)
        for k, ts in va.items():
            print("       view  %-18s %s" % (k, fmt(ts)))
        if args.profile:
            nk, no = launches(native_step)
            ck, co = launches(composed_step)
            print("       launches per step: native %d device kernels (%d top-level aten ops), composed %d (%d)" % (nk, no, ck, co))
        if args.guidance and res == 512:
            from dreamwaltz_g_amd import guidance
            gd = guidance.ControlNetScoreDistillation(torch.device(DEV), image_hw=512, seed=0, cfg=cfg.guide)
            tg = torch.Generator().manual_seed(5)
            cd = gd.unet_cfg.cross_dim
            text = {k: torch.randn(1, 77, cd, generator=tg).to(DEV) for k in ("neg", "pos", "text")}
            trg = nerf_trainer.NeRFSDSTrainer(cfg, net, gd, opts, text_embeds_dict=text, use_controlnet=True)
            trg.train_step_index = 1
            gdata = dict(data, cond_images=(torch.randint(0, 256, (1, 3, 512, 512), generator=tg).float() / 255.0).to(DEV))
            ts = timed(lambda: trg.train_step(gdata, render_kwargs=dict(noises=noises)), 2, 5)
            print(" 512^2 native + real guidance %s" % fmt(ts))


if __name__ == "__main__":
    main()
