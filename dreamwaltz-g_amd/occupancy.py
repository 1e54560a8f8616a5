"""MI355X-native occupancy-grid update of the NeRF stage (boundary B13): what the reference's _NeRFRenderer.update_extra_state
(core/nerf/nerf_renderer.py:95-153) does between the density field and the grid that march_rays_train / march_rays read, on
csrc/nerf_field.hip (k_nf_occupancy) + csrc/occupancy.hip instead of a meshgrid, a dozen element-wise torch statements and a scatter per
cascade, three masked gathers and four host read-backs.

  OccupancyGrid(grid_size, bound, density_thresh, device)     owns density_grid [C, H^3], density_bitfield [C H^3 / 8], iter_density, the
                                                               statistics and the workspace; or adopts existing buffers
      .update(encoder, sigma_net, sigma_scale, ...)            one update: the density pass and dwg_occ_update; no host synchronisation
      .stats()                                                 the one read-back (32 bytes): mean_density, min_density, max_density, ...
      .reset()                                                 reset_extra_state
  lattice_sigma, lattice_points, update_grid, packbits_dev     one C entry point each (include/dwg_occupancy.h, dwg_raymarch.h), for
                                                               callers with their own buffers
  axis_table, cascade_tables, cell_order                       the tables the entry points read, and the host mirror of the cell order

The tables are prepared here, not in the kernels: axis = 2 * arange(H).float() / (H - 1) - 1 evaluated by torch ON THE DEVICE (where the
reference evaluates it; torch on the CPU rounds the division differently at some entries), scale[c] = bound_c - bound_c / H and
half[c] = bound_c / H as Python doubles rounded to fp32 (how torch rounds a Python scalar operand), bound_c = min(2 ** c, bound).
Precision follows autocast like nerf.nerf_field.  No CPU fallback; every buffer is checked (CUDA, dtype, shape, contiguity, alignment)
and a violation raises RuntimeError before any launch.  Nothing here records autograd state."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import pointcloud

MIN_H, MAX_H, MAX_C = 4, 1024, 8
STATS = ("mean", "min", "max", "log_min", "log_max", "thresh", "count_lo", "count_hi")
_axis_cache = {}


def cascades(bound):
    """1 + ceil(log2(bound)), as the reference computes it (nerf_renderer.py:24)."""
    return 1 + math.ceil(math.log2(bound))


def check_limits(C, H):
    """RuntimeError unless (C, H) is within include/dwg_occupancy.h's limits."""
    if int(C) != C or int(H) != H:
        raise RuntimeError("cascades and grid_size must be integers, got %r and %r" % (C, H))
    C, H = int(C), int(H)
    if not (MIN_H <= H <= MAX_H) or H & (H - 1):
        raise RuntimeError("grid_size must be a power of two in [%d, %d], got %d" % (MIN_H, MAX_H, H))
    if not 1 <= C <= MAX_C:
        raise RuntimeError("the occupancy update takes 1..%d cascades, got %d" % (MAX_C, C))
    if C * H ** 3 >= 1 << 32:
        raise RuntimeError("an occupancy grid of %d x %d^3 cells does not fit the 32-bit indices" % (C, H))
    return C, H


def within_limits(C, H):
    try:
        check_limits(C, H)
    except RuntimeError:
        return False
    return True


def axis_table(H, device):
    """2 * arange(H).float() / (H - 1) - 1 evaluated by torch on `device` (nerf_renderer.py:119), cached per (H, device)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(H), str(device))
    if key not in _axis_cache:
        _axis_cache[key] = (2 * torch.arange(H, dtype=torch.int32, device=device).float() / (H - 1) - 1).contiguous()
    return _axis_cache[key]


def cascade_values(bound, C, H):
    """(scale, half) as lists of Python floats: bound_c - bound_c / H and bound_c / H for bound_c = min(2 ** c, bound) (:123-126)."""
    scale, half = [], []
    for cas in range(C):
        b = min(2 ** cas, bound)
        h = b / H
        scale.append(b - h)
        half.append(h)
    return scale, half


def cascade_tables(bound, C, H, device):
    """(scale [C], half [C]) fp32 on the device."""
    scale, half = cascade_values(bound, C, H)
    return (torch.tensor(np.array(scale, np.float64).astype(np.float32), device=device),
            torch.tensor(np.array(half, np.float64).astype(np.float32), device=device))


def cell_order(H):
    """(coords [H^3, 3] int64 in meshgrid order, morton [H^3] int64): the host mirror of csrc/occupancy_common.h + csrc/morton.h."""
    r = np.arange(H, dtype=np.int64)
    coords = np.stack(np.meshgrid(r, r, r, indexing='ij'), -1).reshape(-1, 3)

    def expand(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        v = (v * 0x00000005) & 0x49249249
        return v
    c = coords & 0xFFFFFFFF
    return coords, expand(c[:, 0]) | ((expand(c[:, 1]) << 1) & 0xFFFFFFFF) | ((expand(c[:, 2]) << 2) & 0xFFFFFFFF)


def _aligned(name, t):
    if t.data_ptr() % 16:
        raise RuntimeError("%s must be 16-byte aligned" % name)


def _table_args(axis, noise, scale, half):
    _lib.check_tensor("axis", axis, torch.float32, (None,))
    H = axis.numel()
    _lib.check_tensor("scale", scale, torch.float32, (None,))
    C = scale.numel()
    check_limits(C, H)
    _lib.check_tensor("half", half, torch.float32, (C,))
    _lib.check_tensor("noise", noise, torch.float32, (C, H ** 3, 3))
    return C, H


def lattice_points(axis, noise, scale, half):
    """[C, H^3, 3] fp32: the jittered cell points in meshgrid order (dwg_occ_lattice_points)."""
    C, H = _table_args(axis, noise, scale, half)
    out = torch.empty((C, H ** 3, 3), dtype=torch.float32, device=axis.device)
    _lib.check(_lib.lib().dwg_occ_lattice_points(_lib.ptr(axis), _lib.ptr(noise), _lib.ptr(scale), _lib.ptr(half), C, H, _lib.ptr(out), _lib.stream(axis)),
               "dwg_occ_lattice_points")
    return out


def lattice_sigma(spec, embeddings, sigma_scale, wb, axis, noise, scale, half, random_sigmas=False, out=None):
    """tmp_grid [C, H^3] fp32: the density of the field (pointcloud.field_spec's tuple) at every cell point, at the cell's Morton index
    (dwg_occ_lattice_sigma).  random_sigmas adds the reference's blob.  out: a buffer to write into."""
    C, H = _table_args(axis, noise, scale, half)
    if spec.raw:
        raise RuntimeError("the occupancy update takes the activated density (raw must be False)")
    spec.check(torch.empty((0, 3), dtype=torch.float32, device=embeddings.device), embeddings, sigma_scale, wb)
    if out is None:
        out = torch.empty((C, H ** 3), dtype=torch.float32, device=axis.device)
    else:
        _lib.check_tensor("out", out, torch.float32, (C, H ** 3))
    d = spec.desc(embeddings, sigma_scale, wb)
    _lib.check(_lib.lib().dwg_occ_lattice_sigma(ctypes.byref(d), _lib.ptr(axis), _lib.ptr(noise), _lib.ptr(scale), _lib.ptr(half), C, H,
                                                int(bool(random_sigmas)), _lib.ptr(out), _lib.stream(axis)), "dwg_occ_lattice_sigma")
    return out


def workspace_bytes(C, H):
    C, H = check_limits(C, H)
    return int(_lib.lib().dwg_occ_update_workspace_bytes(C, H))


def update_grid(density_grid, tmp_grid, grid_size, decay, density_thresh, bitfield, stats=None, workspace=None):
    """dwg_occ_update in place on density_grid [C, H^3] and bitfield [C H^3 / 8]: the decayed maximum with tmp_grid on the valid cells,
    the statistics, min(mean, density_thresh) and the bitfield.  Returns stats [8] fp32 on the device (STATS names the entries; the last
    two hold the valid count's uint32 words as bit patterns)."""
    _lib.check_tensor("density_grid", density_grid, torch.float32, (None, None))
    C, H = check_limits(density_grid.shape[0], grid_size)
    _lib.check_tensor("density_grid", density_grid, torch.float32, (C, H ** 3))
    _lib.check_tensor("tmp_grid", tmp_grid, torch.float32, (C, H ** 3))
    _lib.check_tensor("bitfield", bitfield, torch.uint8, (C * H ** 3 // 8,))
    _aligned("density_grid", density_grid); _aligned("tmp_grid", tmp_grid)
    dev = density_grid.device
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=dev)
    else:
        _lib.check_tensor("stats", stats, torch.float32, (8,))
    L = _lib.lib()
    nbytes = int(L.dwg_occ_update_workspace_bytes(C, H))
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        _lib.check_tensor("workspace", workspace, torch.uint8, (None,))
        _aligned("workspace", workspace)
        if workspace.numel() < nbytes:
            raise RuntimeError("workspace has %d bytes, the update needs %d" % (workspace.numel(), nbytes))
    _lib.check(L.dwg_occ_update(_lib.ptr(density_grid), _lib.ptr(tmp_grid), C, H, ctypes.c_float(decay), ctypes.c_float(density_thresh),
                                _lib.ptr(bitfield), _lib.ptr(stats), _lib.ptr(workspace), workspace.numel(), _lib.stream(density_grid)), "dwg_occ_update")
    return stats


def packbits_dev(grid, thresh, bitfield):
    """bitfield [N] <- bit i of byte j = grid[8 j + i] > thresh[0], the threshold a device tensor (dwg_raymarch_packbits_dev)."""
    _lib.check_tensor("bitfield", bitfield, torch.uint8, (None,))
    N = bitfield.numel()
    if not isinstance(grid, torch.Tensor) or grid.numel() != 8 * N:
        raise RuntimeError("grid must be a tensor of %d elements (8 per bitfield byte)" % (8 * N))
    _lib.check_tensor("grid", grid, torch.float32, tuple(grid.shape))
    _lib.check_tensor("thresh", thresh, torch.float32, (1,))
    _aligned("grid", grid)
    if N >= 1 << 32:
        raise RuntimeError("packbits_dev takes fewer than 2^32 bytes")
    _lib.check(_lib.lib().dwg_raymarch_packbits_dev(_lib.ptr(grid), N, _lib.ptr(thresh), _lib.ptr(bitfield), _lib.stream(grid)), "dwg_raymarch_packbits_dev")
    return bitfield


EMPTY_MIN = ("min(): Expected reduction dim to be specified for input.numel() == 0. Specify the reduction dim with the 'dim' argument.")


class OccupancyGrid:
    """The occupancy state of a NeRF: density_grid [C, H^3] fp32 (Morton order per cascade), density_bitfield [C H^3 / 8] uint8 and
    iter_density.  density_grid / density_bitfield: existing device buffers to adopt (written in place) instead of new zeroed ones."""

    def __init__(self, grid_size, bound, density_thresh, device=None, density_grid=None, density_bitfield=None):
        self.bound = float(bound)
        if not self.bound > 0:
            raise RuntimeError("bound must be positive, got %r" % (bound,))
        self.cascade, self.grid_size = check_limits(cascades(self.bound), grid_size)
        self.density_thresh = float(density_thresh)
        C, H = self.cascade, self.grid_size
        if density_grid is None:
            if device is None or torch.device(device).type != "cuda":
                raise RuntimeError("the occupancy grid lives on a CUDA device, got %r" % (device,))
            density_grid = torch.zeros((C, H ** 3), dtype=torch.float32, device=device)
        if density_bitfield is None:
            density_bitfield = torch.zeros(C * H ** 3 // 8, dtype=torch.uint8, device=density_grid.device if isinstance(density_grid, torch.Tensor) else device)
        _lib.check_tensor("density_grid", density_grid, torch.float32, (C, H ** 3))
        _lib.check_tensor("density_bitfield", density_bitfield, torch.uint8, (C * H ** 3 // 8,))
        _aligned("density_grid", density_grid)
        if density_bitfield.device != density_grid.device:
            raise RuntimeError("density_grid and density_bitfield must be on the same device")
        self.density_grid, self.density_bitfield = density_grid, density_bitfield
        dev = self.device = density_grid.device
        self.iter_density = 0
        self.axis = axis_table(H, dev)
        self.scale, self.half = cascade_tables(self.bound, C, H, dev)
        self.tmp_grid = torch.empty((C, H ** 3), dtype=torch.float32, device=dev)
        self.stats_dev = torch.zeros(8, dtype=torch.float32, device=dev)
        self.workspace = torch.empty(workspace_bytes(C, H), dtype=torch.uint8, device=dev)

    def draw_noise(self, generator=None):
        """[C, H^3, 3] uniform draws: torch.rand((H^3, 3)) once per cascade, in cascade order, from the device generator -- what the
        reference's rand_like consumes for S = None."""
        H3 = self.grid_size ** 3
        return torch.stack([torch.rand((H3, 3), dtype=torch.float32, device=self.device, generator=generator) for _ in range(self.cascade)])

    @torch.no_grad()
    def update(self, encoder, sigma_net, sigma_scale, density_activation='exp', density_prior='none', decay=0.95, random_sigmas=False,
               noise=None, generator=None, precision=None):
        """One update_extra_state: the density of the field at a jittered point of every cell, the decayed maximum, the statistics, the
        threshold and the bitfield.  noise [C, H^3, 3]: the draws to use instead of draw_noise(generator).  Launches only: the
        statistics stay on the device until stats()."""
        spec, emb, ss, wb = pointcloud.field_spec(encoder, sigma_net, sigma_scale, self.bound, density_activation, density_prior, True, precision)
        if emb.device != self.device:
            raise RuntimeError("the field's parameters are on %s, the grid on %s" % (emb.device, self.device))
        if noise is None:
            noise = self.draw_noise(generator)
        with torch.cuda.device(self.device):
            lattice_sigma(spec, emb, ss, wb, self.axis, noise, self.scale, self.half, random_sigmas, out=self.tmp_grid)
            update_grid(self.density_grid, self.tmp_grid, self.grid_size, decay, self.density_thresh, self.density_bitfield, self.stats_dev,
                        self.workspace)
        self.iter_density += 1
        return self

    def stats(self):
        """The one read-back (32 bytes) of the last update: mean_density, min_density and max_density (the reference's attributes: the
        latter two are the clamped logarithms), density_thresh (the threshold the bitfield was packed with), min, max and valid_count.
        With no valid cell it raises what the reference's torch.min of an empty tensor raises."""
        raw = self.stats_dev.cpu().numpy()
        count = int(raw[6:8].view(np.uint32)[0]) | (int(raw[6:8].view(np.uint32)[1]) << 32)
        if count == 0:
            raise RuntimeError(EMPTY_MIN)
        return {"mean_density": float(raw[0]), "min_density": float(raw[3]), "max_density": float(raw[4]), "density_thresh": float(raw[5]),
                "min": float(raw[1]), "max": float(raw[2]), "valid_count": count}

    def reset(self):
        """reset_extra_state (nerf_renderer.py:155-164) for the buffers held here."""
        self.density_grid.zero_()
        self.iter_density = 0
        return self
