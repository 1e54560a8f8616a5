"""Restatements for the tests of the one-launch inference render (boundary B14, dreamwaltz_g_amd.nerf_render).  Imports nothing of the
reference.

  _NeRFNetwork        tests/occupancy_cases' stand-in network plus what _NeRFRenderer.run_cuda reads (raymarching, aabb_train / aabb_infer,
                      img_dims) and run_cuda itself: the reference's statements core/nerf/nerf_renderer.py:311-402 over
                      dreamwaltz_g_amd.raymarch -- THE COMPOSITION a bound network ran before the native render.  With `record` set to a
                      list, the evaluation loop appends, per iteration, rays_alive, n_step, ts, sigmas and rgbs.
  trace(...)          float32 numpy restatement of the per-ray inference composite over those records: each ray's sample count, how it
                      ended, the distance of every transmittance test from T_thresh, and weights_sum
  composite_first(...)  the same composite over the first K samples of ray-major (training-march) samples
  make_scene(...)     rays of raymarch_cases.make_cameras, the 'body' bitfield of raymarch_cases.make_grid and a network with the
                      gaussian density prior (centre density e^5: central rays end by T_thresh, outer rays run to far)
  host_counts(...)    the CPU check of a scene: raymarch_cases' numpy march, nerf_field_cases.restate as the field, trace() on them
  compare(...)        the comparison rule of the issue between the native render and the composition
"""
import numpy as np
import torch

from tests import nerf_field_cases as nc
from tests import occupancy_cases as occ
from tests import raymarch_cases as rmc

f32 = np.float32
MAX_STEPS = 256
T_THRESH = 1e-4
BORDER = 1e-6           # a ray is borderline when a transmittance test lies this close to T_thresh (8 ulps of a weights_sum near 1)
BORDER_SHARE = 0.005
ULP = 2.0 ** -23


class _NeRFNetwork(occ._NeRFNetwork):
    """The stand-in carries the reference's class name: nerf.unbound_reason binds the shared-MLP structure by it."""

    def __init__(self, encoder, **kw):
        super().__init__(encoder, **kw)
        from dreamwaltz_g_amd import raymarch
        self.raymarching = raymarch
        b = float(self.bound)
        aabb_train = torch.FloatTensor([-b, -b, -b, b, b, b])
        self.register_buffer('aabb_train', aabb_train)
        self.register_buffer('aabb_infer', aabb_train.clone())
        self.img_dims = 4 if self.latent_mode else 3
        self.record = None          # a list: the evaluation loop appends one dict per iteration
        self.run_calls = []         # (training, shading, perturb) of every call that reached this class method

    def forward(self, x, d, l=None, ratio=1, shading='albedo'):
        # the stand-in has no normals: every shading returns the albedo (the binding test only counts which method a call reaches)
        return self.common_forward(x)

    def run_cuda(self, rays_o, rays_d, light_d=None, ambient_ratio=1.0, shading='albedo', perturb=False, dt_gamma=0, max_steps=1024,
                 T_thresh=1e-4, **kwargs):
        self.run_calls.append((self.training, shading, perturb))
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3)
        rays_d = rays_d.contiguous().view(-1, 3)
        N = rays_o.shape[0]
        device = rays_o.device
        nears, fars = self.raymarching.near_far_from_aabb(rays_o, rays_d, self.aabb_train if self.training else self.aabb_infer)
        if light_d is None:
            light_d = (rays_o[0] + torch.randn(3, device=device, dtype=torch.float))
            light_d = light_d / torch.sqrt(torch.clamp(torch.sum(light_d * light_d, -1, keepdim=True), min=1e-20))
        results = {}
        xyzs, sigmas = None, None
        if self.training:
            counter = self.step_counter[self.local_step % 16]
            counter.zero_()
            self.local_step += 1
            xyzs, dirs, ts, rays = self.raymarching.march_rays_train(rays_o, rays_d, self.bound, self.density_bitfield, self.cascade,
                                                                     self.grid_size, nears, fars, perturb, dt_gamma, max_steps)
            sigmas, rgbs = self(xyzs, dirs, light_d, ratio=ambient_ratio, shading=shading)
            weights, weights_sum, depth, image = self.raymarching.composite_rays_train(sigmas, rgbs, ts, rays, T_thresh)
            results['weights'] = weights
        else:
            dtype = torch.float32
            weights_sum = torch.zeros(N, dtype=dtype, device=device)
            depth = torch.zeros(N, dtype=dtype, device=device)
            image = torch.zeros(N, self.img_dims, dtype=dtype, device=device)
            n_alive = N
            rays_alive = torch.arange(n_alive, dtype=torch.int32, device=device)
            rays_t = nears.clone()
            step = 0
            rgbs = None
            while step < max_steps:
                n_alive = rays_alive.shape[0]
                if n_alive <= 0:
                    break
                n_step = max(min(N // n_alive, 8), 1)
                xyzs, dirs, ts = self.raymarching.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound,
                                                             self.density_bitfield, self.cascade, self.grid_size, nears, fars,
                                                             perturb if step == 0 else False, dt_gamma, max_steps)
                sigmas, rgbs = self(xyzs, dirs, light_d, ratio=ambient_ratio, shading=shading)
                if self.record is not None:
                    self.record.append({"rays_alive": rays_alive.cpu().numpy().copy(), "n_step": n_step, "ts": ts.cpu().numpy().copy(),
                                        "sigmas": sigmas.float().cpu().numpy().copy(), "rgbs": rgbs.float().cpu().numpy().copy()})
                self.raymarching.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, T_thresh)
                rays_alive = rays_alive[rays_alive >= 0]
                step += n_step
        results['image'] = image.reshape(*prefix, self.img_dims)
        results['depth'] = depth.reshape(*prefix)
        results['weights_sum'] = weights_sum.reshape(*prefix)
        results['mask'] = (nears < fars).reshape(*prefix)
        results['xyzs'] = xyzs
        results['sigmas'] = sigmas
        results['rgbs'] = rgbs
        return results


def make_render_network(grid_size, bound, density_prior='gaussian', latent=False, seed=3, gridtype='tiled', interp='linear',
                        density_activation='exp'):
    """A _NeRFNetwork (CPU) with the parameters of nerf_field_cases.make_network; latent: four albedo channels and no sigmoid."""
    kw = dict(density_activation=density_activation, density_prior=density_prior, latent_mode=latent, additional_dim_size=1 if latent else 0)
    src = nc.make_network(gridtype=gridtype, interp=interp, seed=seed, **kw)
    net = _NeRFNetwork(src.encoder, grid_size=grid_size, bound=bound, **kw)
    net.sigma_net.load_state_dict(src.sigma_net.state_dict())
    with torch.no_grad():
        net.sigma_scale.copy_(src.sigma_scale)
    return net


def make_rays(n_rays, seed):
    """n_rays of raymarch_cases.make_cameras' views (32 x 32 pixels each), drawn without replacement in a seeded order."""
    views = max(1, -(-n_rays // 1024))
    o, d = rmc.make_cameras(views, 32, 32, seed=seed)
    pick = np.random.RandomState(seed).permutation(len(o))[:n_rays]
    return np.ascontiguousarray(o[pick]), np.ascontiguousarray(d[pick])


def make_scene(C, H, n_rays, seed=0, kind="body"):
    """(rays_o, rays_d [n_rays, 3] fp32, bitfield [C H^3 / 8] uint8, bound) as numpy; bound = 2^(C - 1)."""
    bound = float(2 ** (C - 1))
    o, d = make_rays(n_rays, seed)
    _, bits = rmc.make_grid(C, H, bound, kind)
    return o, d, bits, bound


def trace(records, N, T_thresh=T_THRESH, binarize=False):
    """The per-ray inference composite (raymarching.cu:874-924) in float32 over the records of the composition's loop.  Returns a dict of
    [N] arrays: count (samples composited), by_thresh (the ray ended on T < T_thresh), margin (the least |T - T_thresh| over the ray's
    tests; inf without a sample) and weights_sum."""
    ws = np.zeros(N, f32)
    count = np.zeros(N, np.int64)
    margin = np.full(N, np.inf)
    by_thresh = np.zeros(N, bool)
    tt = f32(T_thresh)
    for rec in records:
        alive, n_step = rec["rays_alive"].astype(np.int64), rec["n_step"]
        ts = rec["ts"].reshape(len(alive), n_step, 2).astype(f32)
        sig = rec["sigmas"].reshape(len(alive), n_step).astype(f32)
        act = np.ones(len(alive), bool)
        for s in range(n_step):
            act &= ts[:, s, 0] != 0
            i = alive[act]
            a = f32(1) - np.exp(-(sig[act, s] * ts[act, s, 1]))
            if binarize:
                a = (a > f32(0.5)).astype(f32)
            T = f32(1) - ws[i]
            ws[i] = ws[i] + a * T
            count[i] += 1
            margin[i] = np.minimum(margin[i], np.abs(T.astype(np.float64) - float(tt)))
            stop = T < tt
            by_thresh[i[stop]] = True
            act[np.nonzero(act)[0][stop]] = False
    return {"count": count, "by_thresh": by_thresh, "margin": margin, "weights_sum": ws}


def composite_first(sigmas, ts, rays, K, T_thresh=T_THRESH):
    """float32 inference composite of the first K samples of every ray of ray-major samples (rays [N, 2]: offset, count) -> (weights_sum
    [N], used [N])."""
    N = len(rays)
    ws = np.zeros(N, f32)
    used = np.zeros(N, np.int64)
    sig, ts = np.asarray(sigmas, f32), np.asarray(ts, f32)
    for n in range(N):
        off, cnt = int(rays[n, 0]), int(rays[n, 1])
        for i in range(off, off + min(cnt, K)):
            a = f32(1) - np.exp(-(sig[i] * ts[i, 1]))
            T = f32(1) - ws[n]
            ws[n] = ws[n] + a * T
            used[n] += 1
            if T < f32(T_thresh):
                break
    return ws, used


def host_counts(net, o, d, bits, bound, C, H, max_steps=MAX_STEPS, T_thresh=T_THRESH, f16=False):
    """The CPU check of a scene: raymarch_cases' numpy march (no perturbation) for the samples, nerf_field_cases.restate (float64, with
    the fp16 rounding points when f16) rounded to fp32 for the density, trace() for the counts.  Needs no device."""
    b = f32(bound)
    near, far = rmc.near_far(o, d, [-b, -b, -b, b, b, b], 0.2)
    counts, xyzs, _, ts = rmc.march_train(o, d, bits, bound, False, 0.0, max_steps, C, H, near, far, np.zeros(len(o), f32))   # max_steps sets dt_min; a fair scene stays below it
    with torch.no_grad():
        sigma = nc.restate(net, xyzs, f16=f16)[0].numpy().astype(f32) if len(xyzs) else np.zeros(0, f32)
    # one record per sample rank: ray n's k-th sample in iteration k (n_step 1), as the loop's first iterations batch them
    off = np.concatenate([[0], np.cumsum(counts)[:-1]])
    recs, alive = [], np.nonzero(near < far)[0]
    k = 0
    ws = np.zeros(len(o), f32)
    while len(alive):
        has = counts[alive] > k
        t_k = np.zeros((len(alive), 2), f32)
        s_k = np.zeros(len(alive), f32)
        t_k[has] = ts[off[alive[has]] + k]
        s_k[has] = sigma[off[alive[has]] + k]
        recs.append({"rays_alive": alive.copy(), "n_step": 1, "ts": t_k, "sigmas": s_k})
        a = f32(1) - np.exp(-(s_k * t_k[:, 1]))
        T = f32(1) - ws[alive]
        ws[alive] = np.where(has, ws[alive] + a * T, ws[alive])
        alive = alive[has & ~(T < f32(T_thresh))]
        k += 1
    return trace(recs, len(o), T_thresh), counts


def fairness(tr, N, max_steps=MAX_STEPS):
    """The counts the issue asks a fair scene for, from a trace."""
    c = tr["count"]
    return {"by_thresh": int(tr["by_thresh"].sum()), "by_far": int(((c > 0) & ~tr["by_thresh"]).sum()), "no_sample": int((c == 0).sum()),
            "max_count": int(c.max()) if N else 0, "borderline": int((tr["margin"] <= BORDER).sum())}


def assert_fair(fair, N, max_steps=MAX_STEPS):
    assert fair["by_thresh"] >= 50 and fair["by_far"] >= 50 and fair["no_sample"] >= 10, fair
    assert fair["max_count"] < max_steps, fair
    assert fair["borderline"] <= BORDER_SHARE * N, fair


def compare(native, composed, tr, mask, fars, records, T_thresh=T_THRESH):
    """native: (weights_sum, depth, image, counts) of render_rays; composed: (weights_sum, depth, image) of the composition; all numpy.
    Non-borderline rays: counts equal the trace's, values within (S + 2) 2^-23 scale.  Borderline rays: counts within one sample, values
    within T_thresh scale, at most BORDER_SHARE of the rays.  Returns the figures (bit-equal rays among them)."""
    ws, dep, img, cnt = (np.asarray(a) for a in native)
    ws0, dep0, img0 = (np.asarray(a) for a in composed)
    N = len(ws)
    hit = np.asarray(mask, bool)
    s_depth = float(np.max(fars[hit])) if hit.any() else 1.0
    rgb_max = max([float(np.abs(r["rgbs"]).max()) for r in records if r["rgbs"].size] or [0.0])
    s_img = max(1.0, rgb_max)
    border = tr["margin"] <= BORDER
    S = tr["count"].astype(np.float64)
    err = {"weights_sum": np.abs(ws.astype(np.float64) - ws0) / 1.0, "depth": np.abs(dep.astype(np.float64) - dep0) / s_depth,
           "image": np.abs(img.astype(np.float64) - img0).max(-1) / s_img if N else np.zeros(0)}
    bit_equal = int(((ws == ws0) & (dep == dep0) & (img == img0).all(-1) & (cnt == tr["count"])).sum())
    fig = {"rays": N, "borderline": int(border.sum()), "bit_equal": bit_equal, "count_mismatch": int((cnt != tr["count"])[~border].sum()),
           "max_err_over_bound": {k: float((v[~border] / ((S[~border] + 2) * ULP)).max()) if (~border).any() else 0.0 for k, v in err.items()},
           "max_err_borderline": {k: float(v[border].max()) if border.any() else 0.0 for k, v in err.items()}}
    print("nerf_render parity:", fig)
    assert border.sum() <= BORDER_SHARE * N, fig
    assert (cnt[~border] == tr["count"][~border]).all(), fig
    assert (np.abs(cnt[border] - tr["count"][border]) <= 1).all(), fig
    for k, v in err.items():
        assert (v[~border] <= (S[~border] + 2) * ULP).all(), (k, fig)
        assert (v[border] <= T_thresh).all(), (k, fig)
    return fig
