"""Golden fixture of the reference's occupancy-grid update (/root/reference/core/nerf/nerf_renderer.py:95-153): the reference's OWN
_NeRFRenderer.update_extra_state run on the CPU, on an object made with object.__new__ that carries only what the method touches
-> tests/golden/occupancy.npz (recorded inputs and outputs only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_golden_occupancy.py       (build container only: needs /root/reference)

Inert stand-ins satisfy the imports (tests/golden/_ref_stubs.py); the statements that run are the reference's.  STUB-DEPENDENT: the CUDA
backend's raymarching.morton3D and raymarching.packbits are replaced by the numpy stand-ins of tests/occupancy_cases.py (they restate
raymarching.cu:92-105 and :300-326), so the fixture pins the reference's Python statements, not that backend.  `density` is a stand-in that
records the points it is handed and returns an analytic, log-normal-like density of them; torch.rand_like is patched to record its draws.

Calls (H = 8, bound = 2: two cascades of 512 cells):
  first, second   two consecutive calls on one object (density_thresh 10): the second decays the first's grid, under a density that is
                  lower in half of space so that both operands of the maximum win somewhere
  above           one call whose mean exceeds density_thresh (0.05)
  blob            one call with random_sigmas=True
Per call: noise [C, H^3, 3] (the draws), points [C, H^3, 3] (handed to density), sigma [C, H^3] (what density returned, meshgrid order),
tmp [C, H^3] (the values scattered into tmp_grid, Morton order), grid_before / grid_after [C, H^3], bitfield, stats = (mean_density,
min_density, max_density, threshold) as float64, and args = (H, bound, density_thresh, decay, random_sigmas)."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, "/root/reference")
from oracle import animate as oa  # noqa: E402
import _ref_stubs  # noqa: E402
from tests import occupancy_cases as occ  # noqa: E402

H, BOUND = 8, 2


class Raymarching:
    @staticmethod
    def morton3D(coords):
        return torch.from_numpy(occ.morton3d_np(coords.numpy()).astype(np.int32))

    @staticmethod
    def packbits(grid, thresh, bitfield):
        return torch.from_numpy(occ.packbits_np(grid.numpy(), thresh))


def analytic(x, low):
    d = torch.exp(1.2 * torch.sin(3 * x[:, 0] + 1) * torch.cos(2 * x[:, 1]) + 0.8 * x[:, 2] - 1.0)
    return torch.where(x[:, 0] > 0, d * 0.25, d) if low else d


def make(renderer_cls, density_thresh):
    obj = object.__new__(renderer_cls)
    d = obj.__dict__
    d.update(cuda_ray=True, grid_size=H, bound=BOUND, cascade=2, density_thresh=density_thresh, raymarching=Raymarching, mean_density=0,
             iter_density=0, min_density=None, max_density=None, mean_count=0, local_step=0, training=False,
             density_grid=torch.zeros([2, H ** 3]), density_bitfield=torch.zeros(2 * H ** 3 // 8, dtype=torch.uint8),
             step_counter=torch.zeros(16, 2, dtype=torch.int32))
    return obj


def call(obj, out, name, gen, decay=0.95, random_sigmas=False, low=False):
    seen, returned, draws = [], [], []

    def density(x):
        seen.append(x.clone())
        returned.append(analytic(x, low))
        return {'sigma': returned[-1]}

    def rand_like(t, **kw):
        draws.append(torch.rand(t.shape, generator=gen, dtype=t.dtype))
        return draws[-1].clone()
    obj.__dict__["density"] = density
    before = obj.density_grid.clone()
    orig = torch.rand_like
    torch.rand_like = rand_like
    try:
        obj.update_extra_state(decay=decay, random_sigmas=random_sigmas)
    finally:
        torch.rand_like = orig
    assert len(seen) == len(draws) == 2
    coords = np.stack(np.meshgrid(*(np.arange(H),) * 3, indexing='ij'), -1).reshape(-1, 3)
    m = occ.morton3d_np(coords)
    assert sorted(m.tolist()) == list(range(H ** 3))
    sigma = torch.stack([analytic(p, low) for p in seen]).numpy()
    tmp = np.empty((2, H ** 3), np.float32)
    for c in range(2):
        tmp[c, m] = returned[c].numpy()         # the tensor `sigmas += blob` wrote into
    after = obj.density_grid.numpy().copy()
    thresh = min(obj.mean_density, obj.density_thresh)
    # the reference alone needs no excuse: no cell lies between its fp32 mean and the float64 mean
    _, mean64, lo64, hi64, thresh64 = occ.update64(before.numpy(), tmp, decay, obj.density_thresh)
    between = (after > min(thresh, thresh64)) & (after <= max(thresh, thresh64))
    assert not between.any(), name
    g64, *_ = occ.update64(before.numpy(), tmp, decay, obj.density_thresh)
    assert np.array_equal(g64, after), name
    out[name + ".noise"] = torch.stack(draws).numpy()
    out[name + ".points"] = torch.stack(seen).numpy()
    out[name + ".sigma"] = sigma
    out[name + ".tmp"] = tmp
    out[name + ".grid_before"] = before.numpy()
    out[name + ".grid_after"] = after
    out[name + ".bitfield"] = obj.density_bitfield.numpy().copy()
    out[name + ".stats"] = np.array([obj.mean_density, obj.min_density, obj.max_density, thresh], np.float64)
    out[name + ".args"] = np.array([H, BOUND, obj.density_thresh, decay, float(random_sigmas)], np.float64)
    print("%-7s mean %.9g (float64 %.17g, rel %.2e)  log-min %.6f  log-max %.6f  thresh %.9g  bits set %d of %d  iter %d" % (
        name, obj.mean_density, mean64, abs(obj.mean_density - mean64) / mean64, obj.min_density, obj.max_density, thresh,
        int(occ.unpack_bits(out[name + ".bitfield"]).sum()), 2 * H ** 3, obj.iter_density))


def main():
    _ref_stubs.install(oa)
    from core.nerf.nerf_renderer import _NeRFRenderer
    out = {}
    gen = torch.Generator().manual_seed(13)
    obj = make(_NeRFRenderer, 10.0)
    call(obj, out, "first", gen)
    call(obj, out, "second", gen, low=True)
    assert (out["second.grid_after"] == out["second.tmp"]).any() and (out["second.grid_after"] != out["second.tmp"]).any()
    call(make(_NeRFRenderer, 0.05), out, "above", gen)
    assert out["above.stats"][3] == 0.05
    call(make(_NeRFRenderer, 10.0), out, "blob", gen, random_sigmas=True)
    assert (out["blob.tmp"].sum() > out["blob.sigma"].sum())
    np.savez_compressed(os.path.join(HERE, "occupancy.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
