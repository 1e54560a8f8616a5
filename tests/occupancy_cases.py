"""Restatements for the tests of the occupancy-grid update (boundary B13, dreamwaltz_g_amd.occupancy).  Imports nothing of the reference.

  restate_update(...)   the reference's statements core/nerf/nerf_renderer.py:106-147 (S = None) as torch code over a given `density`
                        callable, a given noise tensor in place of torch.rand_like, and given morton3D / packbits callables: the points,
                        the scattered densities, the EMA, the three statistics, the threshold and the bitfield, in the reference's dtypes
                        and on the device of the buffers.
  restate_ema(...)      its second half (:137-147) on its own, over given density_grid / tmp_grid
  update64(...)         float64 numpy EMA, statistics and threshold beside it
  morton3d_np, packbits_np     numpy stand-ins for raymarching.morton3D / packbits (the capture script and the host tests use them)
  bitfield_excuse(...)  the comparison rule of two bitfields packed with two nearby thresholds
  OccNetwork            the test-local network of tests/nerf_field_cases.py with the reference's render state (cuda_ray, grid_size,
                        cascade, density_grid, density_bitfield, step_counter, ...) and update_extra_state stated over the package's
                        morton3D / packbits: the composition a bound user ran before the native update
  load_fixture()        tests/golden/occupancy.npz (recorded from the reference's own update_extra_state by capture_golden_occupancy.py)
"""
import math
import os

import numpy as np
import torch

from tests import nerf_field_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))

REL_STATS = 2e-6        # torch's pairwise fp32 sum over <= 2^22 non-negative terms is within 22 * 2^-24 of the exact mean; ours is fp64 rounded once
ABS_LOG = 1e-5
EXCUSED_SHARE = 1e-4    # at most 1 cell in 10 000 may lie between the two thresholds


def morton3d_np(coords):
    """[N, 3] integer coordinates -> [N] int64 Morton indices (raymarching.cu:92-105)."""
    def expand(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        v = (v * 0x00000005) & 0x49249249
        return v
    c = np.asarray(coords).astype(np.int64)
    return expand(c[:, 0]) | (expand(c[:, 1]) << 1) | (expand(c[:, 2]) << 2)


def packbits_np(grid, thresh):
    """bit i of byte j = grid[8 j + i] > float32(thresh) (raymarching.cu:300-326: the kernel takes the threshold as a float)."""
    g = np.asarray(grid, np.float32).reshape(-1, 8)
    return ((g > np.float32(thresh)).astype(np.uint8) << np.arange(8, dtype=np.uint8)).sum(-1).astype(np.uint8)


def unpack_bits(bitfield):
    """[N] uint8 -> [8 N] bool in cell order."""
    b = np.asarray(bitfield, np.uint8)
    return ((b[:, None] >> np.arange(8, dtype=np.uint8)) & 1).astype(bool).reshape(-1)


@torch.no_grad()
def restate_update(density, noise, density_grid, density_bitfield, grid_size, bound, cascade, density_thresh, morton3D, packbits, decay=0.95,
                   random_sigmas=False):
    """nerf_renderer.py:106-147 with S = grid_size.  density(x) -> {'sigma': ...}; noise [cascade, H^3, 3] replaces the rand_like draws
    (one per cascade, in cascade order).  density_grid is updated in place; returns a dict with the points handed to `density`
    ([cascade, H^3, 3]), tmp_grid, the bitfield and mean_density / min_density / max_density / density_thresh as Python floats."""
    tmp_grid = - torch.ones_like(density_grid)
    dev = density_bitfield.device
    xs = torch.arange(grid_size, dtype=torch.int32, device=dev)
    xx, yy, zz = torch.meshgrid(xs, xs, xs, indexing='ij')
    coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
    indices = morton3D(coords).long()
    xyzs = 2 * coords.float() / (grid_size - 1) - 1
    points = []
    for cas in range(cascade):
        b = min(2 ** cas, bound)
        half_grid_size = b / grid_size
        cas_xyzs = xyzs * (b - half_grid_size)
        cas_xyzs += (noise[cas] * 2 - 1) * half_grid_size
        points.append(cas_xyzs.clone())
        sigmas = density(cas_xyzs)['sigma'].reshape(-1).detach()
        if random_sigmas:
            sigmas += 1.0 * torch.exp(-(cas_xyzs ** 2).sum(-1) / (2 * 0.2 ** 2))
        tmp_grid[cas, indices] = sigmas.float()
    out = restate_ema(density_grid, tmp_grid, density_bitfield, density_thresh, packbits, decay)
    out.update(points=torch.stack(points), tmp_grid=tmp_grid)
    return out


@torch.no_grad()
def restate_ema(density_grid, tmp_grid, density_bitfield, density_thresh, packbits, decay=0.95):
    """nerf_renderer.py:137-147: the EMA in place on density_grid, the three statistics with their read-backs, the threshold, packbits."""
    valid_mask = density_grid >= 0
    density_grid[valid_mask] = torch.maximum(density_grid[valid_mask] * decay, tmp_grid[valid_mask])
    mean_density = torch.mean(density_grid[valid_mask]).item()
    min_density = torch.log(torch.min(density_grid[valid_mask])).clamp(-15., 15.).item()
    max_density = torch.log(torch.max(density_grid[valid_mask])).clamp(-15., 15.).item()
    thresh = min(mean_density, density_thresh)
    bitfield = packbits(density_grid, thresh, density_bitfield)
    return {"bitfield": bitfield, "mean_density": mean_density, "min_density": min_density, "max_density": max_density,
            "density_thresh": thresh}


def update64(grid_before, tmp_grid, decay, density_thresh):
    """float64 numpy: (grid after [fp32 values], mean, min, max, thresh) of the EMA over the valid cells; the decayed product and the
    maximum are taken in fp32 (they are exact statements of fp32 values), the statistics in float64."""
    g = np.array(grid_before, np.float32)
    t = np.asarray(tmp_grid, np.float32)
    valid = g >= 0
    with np.errstate(invalid="ignore"):
        a = g[valid] * np.float32(decay)
        new = np.where(np.isnan(a) | np.isnan(t[valid]), np.float32(np.nan), np.maximum(a, t[valid]))
    g[valid] = new
    v = new.astype(np.float64)
    if v.size == 0:
        return g, float("nan"), float("inf"), float("-inf"), float("nan")
    mean = float(v.sum() / v.size)
    lo, hi = (float("nan"),) * 2 if np.isnan(v).any() else (float(v.min()), float(v.max()))
    return g, mean, lo, hi, min(mean, density_thresh)


def bitfield_excuse(bits_a, bits_b, grid, thresh_a, thresh_b):
    """Number of cells whose bits differ; AssertionError if one of them has a density outside [min, max] of the two thresholds (only a
    cell between the two thresholds may differ) or if more than EXCUSED_SHARE of the cells differ."""
    a, b = unpack_bits(bits_a), unpack_bits(bits_b)
    g = np.asarray(grid, np.float32).reshape(-1)
    diff = np.nonzero(a != b)[0]
    lo, hi = min(thresh_a, thresh_b), max(thresh_a, thresh_b)
    assert all(lo <= float(g[i]) <= hi for i in diff), "a cell outside the two thresholds differs"
    assert len(diff) <= EXCUSED_SHARE * g.size, "%d of %d cells differ" % (len(diff), g.size)
    return len(diff)


def check_stats(got, want, tag=""):
    """got / want: dicts with mean_density, min_density, max_density (the reference's attributes) within the bounds of the issue."""
    m, w = got["mean_density"], want["mean_density"]
    assert abs(m - w) <= REL_STATS * abs(w), (tag, "mean", m, w)
    for k in ("min_density", "max_density"):
        assert abs(got[k] - want[k]) <= ABS_LOG, (tag, k, got[k], want[k])


class _NeRFNetwork(nc._NeRFNetwork):
    """nerf_field_cases._NeRFNetwork + the render state of _NeRFRenderer.__init__ (nerf_renderer.py:24-28, 64-77) and its
    update_extra_state over the package's morton3D and packbits."""

    def __init__(self, encoder, grid_size=16, bound=nc.BOUND, density_thresh=10.0, **kw):
        super().__init__(encoder, bound=bound, **kw)
        self.cascade = 1 + math.ceil(math.log2(bound))
        self.grid_size = grid_size
        self.cuda_ray = True
        self.density_thresh = density_thresh
        self.register_buffer('density_grid', torch.zeros([self.cascade, grid_size ** 3]))
        self.register_buffer('density_bitfield', torch.zeros(self.cascade * grid_size ** 3 // 8, dtype=torch.uint8))
        self.mean_density = 0
        self.iter_density = 0
        self.min_density = None
        self.max_density = None
        self.register_buffer('step_counter', torch.zeros(16, 2, dtype=torch.int32))
        self.mean_count = 0
        self.local_step = 0
        self.calls = []          # (decay, S, random_sigmas) of every call that reached this class method

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=None, random_sigmas=False):
        from dreamwaltz_g_amd import raymarch
        self.calls.append((decay, S, random_sigmas))
        if not self.cuda_ray:
            return
        H3 = self.grid_size ** 3
        noise = torch.stack([torch.rand_like(torch.empty((H3, 3), device=self.density_bitfield.device)) for _ in range(self.cascade)])
        out = restate_update(self.density, noise, self.density_grid, self.density_bitfield, self.grid_size, self.bound, self.cascade,
                             self.density_thresh, raymarch.morton3D, raymarch.packbits, decay=decay, random_sigmas=random_sigmas)
        self.mean_density, self.min_density, self.max_density = out["mean_density"], out["min_density"], out["max_density"]
        self.iter_density += 1
        self.density_bitfield = out["bitfield"]
        total_step = min(16, self.local_step)
        if total_step > 0:
            self.mean_count = int(self.step_counter[:total_step, 0].sum().item() / total_step)
        self.local_step = 0


OccNetwork = _NeRFNetwork       # the class carries the reference's name: nerf.unbound_reason binds the shared-MLP structure by it


def make_occ_network(grid_size, bound=nc.BOUND, gridtype='tiled', interp='linear', density_activation='exp', density_prior='none', seed=3,
                     density_thresh=10.0):
    """An OccNetwork on the package's GridEncoder (CPU) with the parameters of nerf_field_cases.make_network."""
    src = nc.make_network(gridtype=gridtype, interp=interp, density_activation=density_activation, density_prior=density_prior, seed=seed,
                          log2_hashmap_size=15 if gridtype == 'hash' else 19)
    net = OccNetwork(src.encoder, grid_size=grid_size, bound=bound, density_thresh=density_thresh, density_activation=density_activation,
                     density_prior=density_prior)
    net.sigma_net.load_state_dict(src.sigma_net.state_dict())
    with torch.no_grad():
        net.sigma_scale.copy_(src.sigma_scale)
    return net


def load_fixture():
    return np.load(os.path.join(HERE, "golden", "occupancy.npz"))
