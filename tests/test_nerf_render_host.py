"""CPU-side checks of the one-launch inference render (boundary B14): the C entry point validates its arguments before any device
call, and bind_nerf_network installs run_cuda only where it belongs.  No test here needs a device."""
import ctypes

import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from dreamwaltz_g_amd import nerf
from tests import nerf_render_cases as rc
from tests import occupancy_cases as occ

FAKE = 4096                     # 16-byte aligned, never dereferenced on the host


def _desc(out_dim=4, raw=0, precision=0):
    d = _lib.NerfFieldDescC()
    d.embeddings = d.offsets = d.host_offsets = d.sigma_scale = FAKE
    d.num_levels, d.log2_per_level_scale, d.base_resolution = 16, 0.5, 16
    d.gridtype, d.align_corners, d.interp, d.bound = 1, 0, 0, 2.0
    d.num_layers, d.hidden, d.out_dim = 3, 64, out_dim
    for l in range(3):
        d.weight[l] = d.bias[l] = FAKE
    d.density_activation, d.density_prior, d.albedo_sigmoid, d.raw, d.precision = 0, 1, 1, raw, precision
    return d


def _call(d, N=8, H=16, C=2, outs=(FAKE, FAKE, FAKE), bound=2.0, max_steps=256, bitfield=FAKE):
    f = ctypes.c_void_p
    return _lib.lib().dwg_nerf_render_infer(ctypes.byref(d), f(FAKE), f(FAKE), f(FAKE), f(FAKE), N, f(bitfield) if bitfield else None,
                                            ctypes.c_float(bound), 0, ctypes.c_float(0.0), max_steps, C, H, ctypes.c_float(1e-4), 0,
                                            *(f(o) if o else None for o in outs), None, 0, None)


def test_symbol_is_exported_and_has_a_signature():
    assert "dwg_nerf_render_infer" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "dwg_nerf_render_infer")
    assert len(_lib.SIGNATURES["dwg_nerf_render_infer"][1]) == 21


def test_bad_arguments_are_refused_before_any_device_call():
    for outs in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert _call(_desc(), outs=outs) != 0
    assert _call(_desc(), bitfield=None) != 0
    for out_dim in (3, 6):                                  # out_dim - 1 of 2 and 5
        assert _call(_desc(out_dim=out_dim)) != 0
    assert _call(_desc(raw=1)) != 0
    assert _call(_desc(), H=0) != 0
    assert _call(_desc(), C=9) != 0 and _call(_desc(), bound=0.0) != 0 and _call(_desc(), max_steps=0) != 0
    assert _call(_desc(), H=0, N=0) != 0                    # the limits hold for an empty call too


def test_no_rays_is_not_an_error():
    for precision in (0, 1):
        for out_dim in (4, 5):
            assert _call(_desc(out_dim=out_dim, precision=precision), N=0, outs=(None, None, None)) == 0


def test_run_cuda_is_installed_only_with_cuda_ray():
    net = rc.make_render_network(16, 2.0)
    assert nerf.bind_nerf_network(net) is None
    assert "run_cuda" in net.__dict__ and net.run_cuda.__wrapped__.__func__ is rc._NeRFNetwork.run_cuda
    nerf.unbind_nerf_network(net)
    assert "run_cuda" not in net.__dict__
    off = rc.make_render_network(16, 2.0)
    off.cuda_ray = False
    assert nerf.bind_nerf_network(off) is None
    assert "run_cuda" not in off.__dict__
    plain = occ.make_occ_network(16)                        # cuda_ray, but a class without run_cuda: nothing to wrap
    assert nerf.bind_nerf_network(plain) is None
    assert "run_cuda" not in plain.__dict__


def test_a_cpu_call_on_a_bound_network_reaches_the_original():
    """CPU rays are not the native render's: the call goes to the class method, which records it and then fails where the package's
    ray marcher refuses CPU tensors (there is no CPU fallback)."""
    net = rc.make_render_network(16, 2.0).eval()
    assert nerf.bind_nerf_network(net) is None
    o = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        net.run_cuda(o, o + 1.0, max_steps=64)
    assert net.run_calls == [(False, 'albedo', False)]


def test_dwg_bind_nerf_0_binds_nothing(monkeypatch):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "dropin"))
    monkeypatch.setenv("DWG_BIND_NERF", "0")
    import dwg_bind
    net = rc.make_render_network(16, 2.0)
    assert dwg_bind.bind_nerf(net) is net
    assert "run_cuda" not in net.__dict__ and "common_forward" not in net.__dict__
    monkeypatch.setenv("DWG_BIND_NERF", "1")
    assert dwg_bind.bind_nerf(net) is net
    assert "run_cuda" in net.__dict__
