"""CPU checks of the occupancy-grid update (boundary B13, include/dwg_occupancy.h, dreamwaltz_g_amd.occupancy): argument errors are reported
before any launch, the Python mirror of the cell order and of the tables against the arrays recorded from the reference's own
update_extra_state (tests/golden/occupancy.npz), the restatement against the same arrays, and the binding decisions on the reference's
own network class (in a subprocess; skipped when the reference tree is absent)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import nerf_field_cases as nc
from tests import occupancy_cases as occ
from tests.test_nerf_field_host import _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
REFERENCE = "/root/reference"
CALLS = ("first", "second", "above", "blob")


def _mod():
    from dreamwaltz_g_amd import occupancy
    return occupancy


# ------------------------------------------------------------------------------------------------------------------------------------
# argument errors
# ------------------------------------------------------------------------------------------------------------------------------------
BAD_SHAPES = [(0, 8), (9, 8), (1, 2), (1, 3), (1, 12), (1, 2048), (8, 1024), (4, 1024)]        # the last: 4 * 2^30 cells = 2^32


@pytest.mark.parametrize("C,H", BAD_SHAPES)
def test_c_entry_points_reject_shapes_outside_the_limits(C, H):
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    d = _desc()
    assert L.dwg_occ_lattice_sigma(ctypes.byref(d), p, p, p, p, C, H, 0, p, None) == -1
    assert L.dwg_occ_lattice_points(p, p, p, p, C, H, p, None) == -1
    assert L.dwg_occ_update_workspace_bytes(C, H) == 0
    assert L.dwg_occ_update(p, p, C, H, 0.95, 10.0, p, p, p, 1 << 20, None) == -1


def test_c_entry_points_reject_null_misaligned_and_short_arguments():
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    p, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    d = _desc()
    assert L.dwg_occ_lattice_sigma(None, p, p, p, p, 2, 8, 0, p, None) == -1
    assert L.dwg_occ_lattice_sigma(ctypes.byref(_desc(raw=1)), p, p, p, p, 2, 8, 0, p, None) == -1
    assert L.dwg_occ_lattice_sigma(ctypes.byref(_desc(num_levels=0)), p, p, p, p, 2, 8, 0, p, None) == -1
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert L.dwg_occ_lattice_sigma(ctypes.byref(d), args[0], args[1], args[2], args[3], 2, 8, 1, args[4], None) == -1
        assert L.dwg_occ_lattice_points(args[0], args[1], args[2], args[3], 2, 8, args[4], None) == -1
    need = L.dwg_occ_update_workspace_bytes(2, 8)
    assert need > 0 and need % 16 == 0
    assert L.dwg_occ_update_workspace_bytes(2, 128) >= need
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert L.dwg_occ_update(args[0], args[1], 2, 8, 0.95, 10.0, args[2], args[3], args[4], need, None) == -1
    assert L.dwg_occ_update(odd, p, 2, 8, 0.95, 10.0, p, p, p, need, None) == -1
    assert L.dwg_occ_update(p, odd, 2, 8, 0.95, 10.0, p, p, p, need, None) == -1
    assert L.dwg_occ_update(p, p, 2, 8, 0.95, 10.0, p, p, odd, need, None) == -1
    assert L.dwg_occ_update(p, p, 2, 8, 0.95, 10.0, p, p, p, need - 1, None) == -3          # DWG_E_CAPACITY
    assert L.dwg_raymarch_packbits_dev(p, 0, None, None, None) == 0                         # nothing to do
    assert L.dwg_raymarch_packbits_dev(None, 8, p, p, None) == -1 and L.dwg_raymarch_packbits_dev(p, 8, None, p, None) == -1
    assert L.dwg_raymarch_packbits_dev(p, 8, p, None, None) == -1 and L.dwg_raymarch_packbits_dev(odd, 8, p, p, None) == -1


def test_python_wrappers_raise_before_any_launch():
    m = _mod()
    H, C = 8, 2
    f = lambda *s: torch.zeros(*s)          # noqa: E731  CPU tensors
    with pytest.raises(RuntimeError, match="CUDA"):
        m.lattice_points(f(H), f(C, H ** 3, 3), f(C), f(C))
    with pytest.raises(RuntimeError, match="CUDA"):
        m.update_grid(f(C, H ** 3), f(C, H ** 3), H, 0.95, 10.0, torch.zeros(C * H ** 3 // 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CUDA"):
        m.packbits_dev(f(64), f(1), torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="tensor"):
        m.lattice_points(None, f(C, H ** 3, 3), f(C), f(C))
    net = nc.make_network(seed=1)
    from dreamwaltz_g_amd import pointcloud
    with pytest.raises(ValueError, match="CUDA"):
        pointcloud.field_spec(net.encoder, net.sigma_net, net.sigma_scale, net.bound, precision=0)
    for C_, H_ in BAD_SHAPES:
        with pytest.raises(RuntimeError):
            m.check_limits(C_, H_)
        assert not m.within_limits(C_, H_)
    assert m.check_limits(2, 128) == (2, 128) and m.within_limits(8, 512) and m.within_limits(3, 1024)
    with pytest.raises(RuntimeError, match="CUDA"):
        m.OccupancyGrid(8, 2, 10.0, device="cpu")
    with pytest.raises(RuntimeError, match="CUDA"):
        m.OccupancyGrid(8, 2, 10.0, density_grid=f(2, 512), density_bitfield=torch.zeros(128, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="power of two"):
        m.OccupancyGrid(12, 2, 10.0, device="cuda")
    with pytest.raises(RuntimeError, match="bound"):
        m.OccupancyGrid(8, 0, 10.0, device="cuda")


def test_cascade_count_and_tables_follow_the_reference():
    m = _mod()
    assert [m.cascades(b) for b in (1, 2, 3, 4, 1.5)] == [1, 2, 3, 3, 2]
    scale, half = m.cascade_values(3, 3, 32)
    assert half == [1 / 32, 2 / 32, 3 / 32] and scale == [1 - 1 / 32, 2 - 2 / 32, 3 - 3 / 32]       # min(2 ** c, bound) clamps the last


# ------------------------------------------------------------------------------------------------------------------------------------
# the recorded reference
# ------------------------------------------------------------------------------------------------------------------------------------
def test_cell_order_mirror_matches_the_recorded_scatter():
    """cell_order's Morton index is where the reference scattered each meshgrid cell: tmp[c, morton[n]] == sigma (+ blob) [c, n]."""
    m = _mod()
    fx = occ.load_fixture()
    H = int(fx["first.args"][0])
    coords, morton = m.cell_order(H)
    assert np.array_equal(morton, occ.morton3d_np(coords)) and sorted(morton.tolist()) == list(range(H ** 3))
    for name in ("first", "second", "above"):
        assert np.array_equal(fx[name + ".tmp"][:, morton], fx[name + ".sigma"]), name
    # and the recorded points are the cell points of that order: within 2 ulps of bound of the mirror evaluated in float64
    scale, half = m.cascade_values(2, 2, H)
    axis = 2 * np.arange(H, dtype=np.float64) / (H - 1) - 1
    for c in range(2):
        want = axis[coords] * scale[c] + (fx["first.noise"][c].astype(np.float64) * 2 - 1) * half[c]
        assert np.abs(fx["first.points"][c] - want).max() <= 2 * np.spacing(np.float32(2.0))


@pytest.mark.parametrize("name", CALLS)
def test_restatement_reproduces_the_recorded_reference_on_the_cpu(name):
    """tests/occupancy_cases.restate_update is the reference's statements: fed the recorded draws and a density that returns the recorded
    values, it reproduces every recorded array bit for bit on the CPU."""
    fx = occ.load_fixture()
    H, bound, thresh, decay, blob = fx[name + ".args"]
    H, bound = int(H), int(bound)
    sigma = iter(torch.from_numpy(fx[name + ".sigma"]))
    grid = torch.from_numpy(fx[name + ".grid_before"].copy())
    out = occ.restate_update(lambda x: {'sigma': next(sigma).clone()}, torch.from_numpy(fx[name + ".noise"]), grid,
                             torch.zeros(2 * H ** 3 // 8, dtype=torch.uint8), H, bound, 2, float(thresh),
                             lambda c: torch.from_numpy(occ.morton3d_np(c.numpy())), lambda g, t, b: torch.from_numpy(occ.packbits_np(g.numpy(), t)),
                             decay=float(decay), random_sigmas=bool(blob))
    assert np.array_equal(out["points"].numpy(), fx[name + ".points"])
    assert np.array_equal(out["tmp_grid"].numpy(), fx[name + ".tmp"])
    assert np.array_equal(grid.numpy(), fx[name + ".grid_after"])
    assert np.array_equal(out["bitfield"].numpy(), fx[name + ".bitfield"])
    assert [out["mean_density"], out["min_density"], out["max_density"], out["density_thresh"]] == fx[name + ".stats"].tolist()
    # the float64 variant agrees within the bounds the GPU tests use, and excuses no cell
    g64, mean, lo, hi, t64 = occ.update64(fx[name + ".grid_before"], fx[name + ".tmp"], float(decay), float(thresh))
    assert np.array_equal(g64, fx[name + ".grid_after"])
    occ.check_stats({"mean_density": mean, "min_density": float(np.clip(np.log(lo), -15, 15)), "max_density": float(np.clip(np.log(hi), -15, 15))},
                    dict(zip(("mean_density", "min_density", "max_density"), fx[name + ".stats"])), name)
    assert occ.bitfield_excuse(occ.packbits_np(g64, t64), fx[name + ".bitfield"], g64, t64, fx[name + ".stats"][3]) == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the binding decisions on the reference's class
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core", "nerf")), reason="reference tree not present")
def test_b13_binding_decisions_on_the_reference_network():
    code = r"""
import json, os, sys
sys.dont_write_bytecode = True
ROOT, DROPIN, REF = %r, %r, %r
sys.path.insert(0, ROOT); sys.path.insert(0, DROPIN); sys.path.insert(0, os.path.join(ROOT, "tests", "golden")); sys.path.insert(0, REF)
from oracle import animate as oa
import _ref_stubs
_ref_stubs.install(oa)
import dwg_bind
dwg_bind.install()
import core.nerf.nerf_model as nm
from configs import NeRFConfig
import dwg_import
from dreamwaltz_g_amd import nerf
out = {}
n = nm.build_NeRFNetwork(NeRFConfig(cuda_ray=True, grid_size=8))
out["cuda_ray"] = [bool(n._dwg_nerf_bound), "update_extra_state" in n.__dict__,
                   getattr(n.__dict__.get("update_extra_state"), "__wrapped__", None) is not None]
# the class method, counted
calls = []
cls_update = type(n).update_extra_state
def counted(self, *a, **k):
    calls.append((a, k))
type(n).update_extra_state = counted
try:
    nerf.unbind_nerf_network(n); nerf.bind_nerf_network(n)          # rebind over the counting class method
    n.update_extra_state(S=4)                                       # chunked: the original
    out["S4"] = len(calls)
    n.update_extra_state()                                          # buffers on the CPU: the original
    out["cpu"] = len(calls)
finally:
    type(n).update_extra_state = cls_update
nerf.unbind_nerf_network(n)
out["unbound"] = ["update_extra_state" in n.__dict__, "common_forward" in n.__dict__, bool(n._dwg_nerf_bound)]
m = nm.build_NeRFNetwork(NeRFConfig(cuda_ray=False, grid_size=8))
out["no_cuda_ray"] = [bool(m._dwg_nerf_bound), "update_extra_state" in m.__dict__]
u = nm.build_NeRFNetwork(NeRFConfig(cuda_ray=True, grid_size=8, structure="dual_mlp"))
out["dual_mlp"] = [bool(getattr(u, "_dwg_nerf_bound", False)), "update_extra_state" in u.__dict__]
o = nm.build_NeRFNetwork(NeRFConfig(cuda_ray=True, grid_size=12))
out["H12"] = [bool(o._dwg_nerf_bound), "update_extra_state" in o.__dict__]
print(json.dumps(out))
""" % (ROOT, DROPIN, REFERENCE)
    env = dict(os.environ)
    env.pop("DWG_BIND_NERF", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["cuda_ray"] == [True, True, True]                    # installed for a covered network with cuda_ray, __wrapped__ set
    assert out["S4"] == 1 and out["cpu"] == 2                       # both fall through to the original method
    assert out["unbound"] == [False, False, False]                  # removed by unbind
    assert out["no_cuda_ray"] == [True, False]                      # bound field, no occupancy state: not installed
    assert out["dual_mlp"] == [False, False]                        # not installed for an unbound network
    assert out["H12"] == [True, False]                              # a grid size outside the limits stays on the reference's method
