"""CPU checks of the point-cloud export boundary (B12, include/dwg_pointcloud.h, dreamwaltz_g_amd.pointcloud): argument errors are reported
before any launch through the C-ABI and through Python, the Python mirrors of the lattice order reproduce the order recorded from the
reference, to_basic gives the reference's container, the bounding-box argument forms, and the binding of the reference's
export_point_cloud / remove_points_inside_bboxes (in a subprocess with the real reference module; skipped when the reference tree is
absent)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from tests import nerf_field_cases as nc
from tests import pointcloud_cases as pcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
REFERENCE = "/root/reference"

FAKE = ctypes.c_void_p(4096)          # aligned, never dereferenced: every call below must fail (or succeed) before a launch
E = -1


def _desc(**over):
    d = _lib.NerfFieldDescC()
    d.embeddings, d.offsets, d.host_offsets = 4096, 4096, None
    d.num_levels, d.log2_per_level_scale, d.base_resolution = 16, 0.5, 16
    d.gridtype, d.align_corners, d.interp, d.bound = 1, 0, 1, 2.0
    d.num_layers, d.hidden, d.out_dim = 3, 64, 4
    for l in range(3):
        d.weight[l], d.bias[l] = 4096, 4096
    d.density_activation, d.density_prior, d.albedo_sigmoid, d.raw, d.sigma_scale, d.precision = 0, 0, 1, 0, 4096, 0
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _each_null(fn, base, positions):
    for k in positions:
        args = list(base)
        args[k] = None
        assert fn(*args) == E, k


def test_bad_arguments_return_arg_error_before_any_launch():
    L = _lib.lib()
    d = _desc()
    ls = [ctypes.byref(d), FAKE, FAKE, FAKE, 10, 10, 10, 4, FAKE, FAKE, None]
    _each_null(L.dwg_pc_lattice_sigma, ls, (0, 1, 2, 3, 8, 9))
    args = list(ls); args[7] = 0
    assert L.dwg_pc_lattice_sigma(*args) == E                                       # split 0
    args = list(ls); args[4:7] = [1626, 1626, 1626]
    assert L.dwg_pc_lattice_sigma(*args) == E                                       # 1626^3 >= 2^32
    args = list(ls); args[4:7] = [65536, 65536, 1]
    assert L.dwg_pc_lattice_sigma(*args) == E
    for bad in (_desc(raw=1), _desc(hidden=128), _desc(out_dim=17), _desc(num_levels=33), _desc(bound=0.0), _desc(precision=2)):
        args = list(ls); args[0] = ctypes.byref(bad)
        assert L.dwg_pc_lattice_sigma(*args) == E
    sa = [5000, FAKE, 0.5, FAKE, 5000, FAKE, FAKE, 12, None]
    _each_null(L.dwg_pc_select_above, sa, (1, 3, 5, 6))
    args = list(sa); args[0] = 1 << 32
    assert L.dwg_pc_select_above(*args) == E
    args = list(sa); args[6] = ctypes.c_void_p(4098)                                # misaligned workspace
    assert L.dwg_pc_select_above(*args) == E
    args = list(sa); args[7] = 8                                                    # three blocks need 12 bytes
    assert L.dwg_pc_select_above(*args) == -3
    sf = [5000, FAKE, FAKE, 5000, FAKE, FAKE, 12, None]
    _each_null(L.dwg_pc_select_flags, sf, (1, 2, 4, 5))
    args = list(sf); args[0] = 1 << 32
    assert L.dwg_pc_select_flags(*args) == E
    assert L.dwg_pc_select_workspace_bytes(5000) == 12 and L.dwg_pc_select_workspace_bytes(2048) == 4
    assert L.dwg_pc_select_workspace_bytes(0) == 0 and L.dwg_pc_select_workspace_bytes(1 << 32) == 0
    lp = [7, FAKE, FAKE, FAKE, FAKE, 10, 10, 10, 4, FAKE, None]
    _each_null(L.dwg_pc_lattice_points, lp, (1, 2, 3, 4, 9))
    args = list(lp); args[8] = 0
    assert L.dwg_pc_lattice_points(*args) == E
    args = list(lp); args[5:8] = [1626, 1626, 1626]
    assert L.dwg_pc_lattice_points(*args) == E
    fd = [7, FAKE, 1e-3, 2.0, FAKE, None]
    _each_null(L.dwg_pc_fd_points, fd, (1, 4))
    for bad in ((2, float('nan')), (3, -1.0), (3, float('nan'))):
        args = list(fd); args[bad[0]] = bad[1]
        assert L.dwg_pc_fd_points(*args) == E, bad
    fi = [7, 3, FAKE, FAKE, 1e-3, FAKE, FAKE, None]
    _each_null(L.dwg_pc_finish, fi, (2, 3, 5, 6))
    for C in (0, 2, 5):
        args = list(fi); args[1] = C
        assert L.dwg_pc_finish(*args) == E, C
    args = list(fi); args[1], args[2] = 4, ctypes.c_void_p(4100)                    # four channels are read 16 bytes at a time
    assert L.dwg_pc_finish(*args) == E
    ob = [7, FAKE, 2, FAKE, FAKE, None]
    _each_null(L.dwg_pc_outside_boxes, ob, (1, 3, 4))


def test_empty_calls_launch_nothing():
    L = _lib.lib()
    d = _desc()
    assert L.dwg_pc_lattice_sigma(ctypes.byref(d), None, None, None, 0, 10, 10, 4, None, None, None) == 0
    assert L.dwg_pc_select_above(0, None, 0.5, None, 0, None, None, 0, None) == 0
    assert L.dwg_pc_select_flags(0, None, None, 0, None, None, 0, None) == 0
    assert L.dwg_pc_lattice_points(0, None, None, None, None, 10, 10, 10, 4, None, None) == 0
    assert L.dwg_pc_fd_points(0, None, 1e-3, 2.0, None, None) == 0
    assert L.dwg_pc_finish(0, 3, None, None, 1e-3, None, None, None) == 0
    assert L.dwg_pc_outside_boxes(0, None, 0, None, None, None) == 0


def test_python_argument_errors_are_value_errors_before_any_launch():
    from dreamwaltz_g_amd import pointcloud as pc
    net = nc.make_network(L=4)                                                      # on the CPU: nothing here may reach a launch
    kw = dict(density_thresh=1.0)
    for bad in (dict(resolution=0), dict(resolution=-3), dict(resolution=8, split_size=0), dict(resolution=1626), dict(resolution=2.5)):
        with pytest.raises(ValueError):
            pc.export_point_cloud(net.encoder, net.sigma_net, net.sigma_scale, net.bound, **bad, **kw)
    with pytest.raises(ValueError, match="CUDA"):                                   # CPU parameters
        pc.export_point_cloud(net.encoder, net.sigma_net, net.sigma_scale, net.bound, resolution=4, **kw)
    wide = nc.make_network(L=4, hidden=128)
    with pytest.raises(ValueError):
        pc.export_point_cloud(wide.encoder, wide.sigma_net, wide.sigma_scale, wide.bound, resolution=4, **kw)
    with pytest.raises(ValueError, match="density_activation"):
        pc.export_point_cloud(net.encoder, net.sigma_net, net.sigma_scale, net.bound, resolution=4, density_activation='relu', **kw)
    net.density_prior_type = 'smpl'
    with pytest.raises(ValueError, match="does not cover.*density_prior"):
        pc.export_point_cloud_from(net, resolution=4, density_thresh=1.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        pc.select_above(torch.zeros(8), 0.5)
    with pytest.raises(RuntimeError, match="CUDA"):
        pc.outside_boxes(torch.zeros(4, 3), torch.zeros(1, 2, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="CUDA"):
        pc.lattice_points(torch.zeros(4, dtype=torch.int32), torch.zeros(2), torch.zeros(2), torch.zeros(2), 2)


@pytest.mark.parametrize("case", ["r10s4", "r5s8"])
def test_python_mirrors_of_the_index_function_reproduce_the_recorded_order(case):
    from dreamwaltz_g_amd import pointcloud as pc
    fx = pcc.load_fixture()
    R, split = (int(v) for v in fx[case + ".resolution_split"])
    ax = torch.linspace(-1, 1, R).numpy()
    order = pc.lattice_order(R, R, R, split)
    assert order.shape == (R ** 3, 3)
    assert np.array_equal(ax[order], fx[case + ".lattice"])
    assert all(pc.lattice_index(f, R, R, R, split) == tuple(order[f]) for f in range(R ** 3))
    # the recorded export is the recorded lattice filtered by the recorded density, in order
    keep = fx[case + ".sigma"] > np.float32(fx["thresh"][0])
    assert np.array_equal(fx[case + ".points"], fx[case + ".lattice"][keep].astype(np.float64))
    assert np.array_equal(fx[case + ".alphas"][:, 0], fx[case + ".sigma"][keep].astype(np.float64))
    # and the float64 restatement of the bounding-box loop reproduces the recorded remainder
    mask, kept = pcc.remove_inside(fx[case + ".points"], [fx[case + "." + k] for k in ("points", "colors", "normals", "alphas")], fx["box"].tolist())
    for k, a in zip(("points", "colors", "normals", "alphas"), kept):
        assert np.array_equal(a, fx[case + ".removed." + k]), k


def test_lattice_index_with_uneven_axes_and_a_large_lattice():
    from dreamwaltz_g_amd import pointcloud as pc
    for nx, ny, nz, split in ((5, 7, 3, 2), (1, 9, 4, 4), (6, 1, 1, 8), (3, 3, 3, 1)):
        order = pc.lattice_order(nx, ny, nz, split)
        assert len(set(map(tuple, order))) == nx * ny * nz
        assert all(pc.lattice_index(f, nx, ny, nz, split) == tuple(order[f]) for f in range(nx * ny * nz))
    R = 1300                                                                        # 2.197e9 points: indices past 2^31
    assert pc.lattice_index(0, R, R, R, 256) == (0, 0, 0) and pc.lattice_index(R ** 3 - 1, R, R, R, 256) == (R - 1, R - 1, R - 1)
    assert pc.lattice_index(256 * R * R, R, R, R, 256) == (256, 0, 0)


def test_to_basic_is_the_reference_container():
    from dreamwaltz_g_amd import pointcloud as pc
    g = torch.Generator().manual_seed(0)
    cloud = pc.PointCloud(torch.rand(5, 3, generator=g), torch.rand(5, 3, generator=g), torch.rand(5, 3, generator=g), torch.rand(5, 1, generator=g),
                          {"n_points": 5})
    b = cloud.to_basic()
    assert len(b) == 5 and len(cloud) == 5
    for k, shape in (("points", (5, 3)), ("colors", (5, 3)), ("normals", (5, 3)), ("alphas", (5, 1))):
        a = getattr(b, k)
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == shape
        assert np.array_equal(a, getattr(cloud, k).numpy().astype(np.float64))        # the fp32 values, widened

    class Other:
        pass
    assert isinstance(cloud.to_basic(Other), Other)
    z = lambda c: torch.empty((0, c))       # noqa: E731
    e = pc.PointCloud(z(3), z(3), z(3), z(1)).to_basic()
    assert len(e) == 0
    assert [getattr(e, k).shape for k in ("points", "colors", "normals", "alphas")] == [(0, 3), (0, 3), (0, 3), (0, 1)]
    assert all(getattr(e, k).dtype == np.float64 for k in ("points", "colors", "normals", "alphas"))


def test_bounding_box_argument_forms():
    from dreamwaltz_g_amd import pointcloud as pc
    one = pc.parse_boxes([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.1]])
    assert one.shape == (1, 2, 3) and one.dtype == np.float64
    assert one[0, 0].tolist() == [-0.5, -0.5, -0.5] and one[0, 1].tolist() == [0.5, 0.5, 0.1]
    swapped = pc.parse_boxes([[0.5, -0.5, 0.1], [-0.5, 0.5, -0.5]])                 # corners in any order: amin / amax per box
    assert np.array_equal(swapped, one)
    two = pc.parse_boxes([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], [[-1, -1, -1], [0, 0, 0]]])      # a list of boxes, int-valued ones included
    assert two.shape == (2, 2, 3) and two[1, 0].tolist() == [-1, -1, -1]
    assert pc.parse_boxes((np.array([[0.1, 0.2, 0.3], [0.0, 0.5, 0.1], [0.3, 0.3, 0.3]]),))[0].tolist() == [[0.0, 0.2, 0.1], [0.3, 0.5, 0.3]]
    assert pc.parse_boxes([[[0.1, 0.0, 0.0], [0.1, 1.0, 1.0]]])[0, 0, 0] == 0.1        # the double 0.1, not float32(0.1)
    for bad in ([[0, 0, 0], [1, 1, 1]],                   # an int-valued single box: the reference reads it as two "boxes" of scalars
                [[[0.0, 0.0], [1.0, 1.0]]], [[0.0, 0.0, 0.0], [1.0, 1.0]], [["a", "b", "c"]]):
        with pytest.raises(TypeError, match="accepted"):
            pc.parse_boxes(bad)

    class Basic:
        points = np.array([[0.1, 0.2, 0.3]])            # the double 0.1 is no fp32 value
    with pytest.raises(TypeError, match="fp32"):
        pc.remove_points_inside_bboxes(Basic(), [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])


_BIND_CODE = r"""
import inspect, json, os, sys
sys.dont_write_bytecode = True
ROOT, DROPIN, REF = %r, %r, %r
sys.path.insert(0, ROOT); sys.path.insert(0, DROPIN); sys.path.insert(0, os.path.join(ROOT, "tests", "golden")); sys.path.insert(0, REF)
from oracle import animate as oa
import _ref_stubs
_ref_stubs.install(oa)
import torch
import core.nerf.to_point_cloud as tp                 # imported BEFORE the hooks: install() patches what is already there
ref = {"export": tp.export_point_cloud, "remove": tp.remove_points_inside_bboxes}
calls = []
def export_stub(self, resolution=None, split_size=128, density_thresh=None):
    calls.append(("export", resolution, split_size, density_thresh)); return "export-stub"
def remove_stub(point_cloud, bboxes):
    calls.append("remove"); return "remove-stub"
import dwg_bind
dwg_bind.install()
out = {}
e, r = tp.export_point_cloud, tp.remove_points_inside_bboxes
out["patched"] = [bool(getattr(x, "__dwg_bound__", False)) for x in (e, r)]
out["wrapped_is_reference"] = getattr(e, "__wrapped__", None) is ref["export"] and getattr(r, "__wrapped__", None) is ref["remove"]
out["same_signatures"] = all(str(inspect.signature(a)) == str(inspect.signature(b)) for a, b in ((e, ref["export"]), (r, ref["remove"])))
dwg_bind.uninstall()
out["restored"] = tp.export_point_cloud is ref["export"] and tp.remove_points_inside_bboxes is ref["remove"]
# without a device the wrappers call what they wrapped: stubs in the originals' places, the device probe answering "none"
tp.export_point_cloud, tp.remove_points_inside_bboxes = export_stub, remove_stub
dwg_bind.install()
dwg_bind._hip_device = lambda: None
out["fallback"] = [tp.export_point_cloud(object(), resolution=7, split_size=3), tp.remove_points_inside_bboxes(None, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])]
out["calls"] = calls
out["rewrapped"] = bool(getattr(tp.export_point_cloud, "__dwg_bound__", False))
# the reference's own functions still run through the wrappers without a device (its bbox loop on a BasicPointCloud)
dwg_bind.uninstall()
tp.export_point_cloud, tp.remove_points_inside_bboxes = ref["export"], ref["remove"]
dwg_bind.install()
dwg_bind._hip_device = lambda: None
pc = tp.BasicPointCloud()
import numpy as np
pc.points = np.array([[0.0, 0.0, 0.0], [0.9, 0.9, 0.9]]); pc.colors = pc.points.copy(); pc.normals = pc.points.copy(); pc.alphas = np.ones((2, 1))
out["reference_loop"] = tp.remove_points_inside_bboxes(pc, [[-0.5, -0.5, -0.5], [0.5, 0.5, 0.1]]).points.tolist()
print(json.dumps(out))
"""


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core")), reason="reference tree not present")
def test_b12_binding_of_the_reference_point_cloud_module():
    code = _BIND_CODE % (ROOT, DROPIN, REFERENCE)
    env = dict(os.environ)
    env.pop("DWG_BIND_POINTCLOUD", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["patched"] == [True, True] and out["wrapped_is_reference"] and out["same_signatures"] and out["restored"], out
    assert out["fallback"] == ["export-stub", "remove-stub"] and out["rewrapped"], out
    assert out["calls"] == [["export", 7, 3, None], "remove"], out
    assert out["reference_loop"] == [[0.9, 0.9, 0.9]], out
    env["DWG_BIND_POINTCLOUD"] = "0"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["patched"] == [False, False] and not out["rewrapped"], out
    assert out["fallback"] == ["export-stub", "remove-stub"] and out["reference_loop"] == [[0.9, 0.9, 0.9]], out      # the stubs themselves
