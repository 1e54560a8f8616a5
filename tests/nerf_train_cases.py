"""Restatements for the tests of the training render (boundary B18, dreamwaltz_g_amd.nerf_render.render_rays_train).  Imports nothing of
the reference.

  SCENES                the three scenes of nerf_render_cases.make_scene / make_render_network the tests run: (cascade, grid, rays, seed)
  noises(n, seed)       the perturbation of a scene: RandomState(seed + 100).rand(n), the same on the host and on the device
  stops(...)            float64 training stop rule over ray-major samples: live (samples composited: up to and including the first one
                        after which T < T_thresh) and margin (least |T - T_thresh| over the ray's tests)
  host_figures(...)     the CPU check of a scene: raymarch_cases' numpy march, nerf_field_cases.restate for the density, stops()
  make_network(...)     the scene's network, also the 'scaling' and the opaque variants
  figures / assert_fair the counts a fair scene is asked for, from live and the per-ray sample counts
"""
import numpy as np
import torch

from tests import nerf_field_cases as nc
from tests import nerf_render_cases as rc
from tests import raymarch_cases as rmc

f32 = np.float32
MAX_STEPS = 1024
T_THRESH = 1e-4
BORDER = 1e-7                # a ray is borderline when a transmittance test lies this close to T_thresh
BORDER_SHARE = 0.005
F32_BWD = 1e-4               # relative L2 between two orders of the same fp32 sums (tests/test_nerf_field_gpu.py)
SCENES = [(1, 16, 5, 1), (2, 32, 1000, 9), (2, 64, 3000, 3)]


def noises(n, seed):
    return np.random.RandomState(seed + 100).rand(n).astype(f32)


def stops(sigmas, ts, counts, T_thresh=T_THRESH):
    """-> live [N], margin [N] (inf without a sample) of ray-major samples with per-ray `counts`; float64 on the given values."""
    sig, ts = np.asarray(sigmas, np.float64), np.asarray(ts, np.float64)
    N = len(counts)
    live = np.zeros(N, np.int64)
    margin = np.full(N, np.inf)
    off = 0
    for n in range(N):
        cnt = int(counts[n])
        if cnt:
            s = slice(off, off + cnt)
            T = np.cumprod(np.exp(-sig[s] * ts[s, 1]))          # 1 - alpha, alpha = 1 - exp(-sigma dt)
            below = np.nonzero(T < T_thresh)[0]
            k = below[0] + 1 if len(below) else cnt
            live[n] = k
            margin[n] = np.abs(T[:k] - T_thresh).min()
        off += cnt
    return live, margin


def figures(live, counts, margin=None):
    """The counts of the issue's table from live [N] and the per-ray sample counts [N]."""
    live, counts = np.asarray(live, np.int64), np.asarray(counts, np.int64)
    cut = live < counts
    whole = (live == counts) & (counts > 0)
    M, M_live = int(counts.sum()), int(live.sum())
    fig = {"M": M, "M_live": M_live, "culled": (M - M_live) / M if M else 0.0, "cut": int(cut.sum()), "whole": int(whole.sum()),
           "no_sample": int((counts == 0).sum()), "longest": int(counts.max()) if len(counts) else 0,
           "long_cut": int((cut & (counts > 64)).sum()), "long_whole": int((whole & (counts > 64)).sum()),
           "stop_in_a_later_chunk": int((cut & (live > 64)).sum())}
    if margin is not None:
        fig["borderline"] = int((np.asarray(margin) <= BORDER).sum())
    return fig


def assert_fair(fig, N):
    """>= 100 rays cut, >= 100 whole, >= 100 without a sample, culled share >= 0.03, rays longer than one 64-sample chunk on both sides
    of a cut and a stop inside a later chunk, borderline rays <= 0.5 % of N."""
    assert fig["cut"] >= 100 and fig["whole"] >= 100 and fig["no_sample"] >= 100, fig
    assert fig["culled"] >= 0.03, fig
    assert fig["long_cut"] >= 1 and fig["long_whole"] >= 1 and fig["stop_in_a_later_chunk"] >= 1, fig
    assert fig.get("borderline", 0) <= BORDER_SHARE * N, fig


def make_network(H, bound, latent=False, act='exp', opaque=False):
    """nerf_render_cases.make_render_network (CPU, gaussian density prior).  opaque (with act 'scaling'): sigma_scale 6 and the density
    bias raised by 10, so that every pre-activation is positive and scaled by e^6 -- sigma dt > 8 at the smallest step and a ray is spent
    within a few samples."""
    net = rc.make_render_network(H, bound, latent=latent, density_activation=act)
    if opaque:
        with torch.no_grad():
            net.sigma_scale.fill_(6.0)
            net.sigma_net.net[-1].bias[0] += 10.0
    return net


def host_figures(C, H, n, seed, f16=False, latent=False, act='exp', opaque=False):
    """The CPU check of a scene with the training stop rule; needs no device."""
    o, d, bits, bound = rc.make_scene(C, H, n, seed=seed)
    net = make_network(H, bound, latent, act, opaque)
    b = f32(bound)
    near, far = rmc.near_far(o, d, [-b, -b, -b, b, b, b], 0.2)
    counts, xyzs, _, ts = rmc.march_train(o, d, bits, bound, False, 0.0, MAX_STEPS, C, H, near, far, noises(n, seed))
    with torch.no_grad():
        sigma = nc.restate(net, xyzs, f16=f16)[0].numpy().astype(f32) if len(xyzs) else np.zeros(0, f32)
    live, margin = stops(sigma, ts, counts)
    fig = figures(live, counts, margin)
    fig["longest_live"] = int(live.max()) if n else 0
    fig["longer_than_3"] = int((counts > 3).sum())
    return fig
