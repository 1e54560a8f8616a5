"""CPU-side checks of the shaded one-launch inference render (boundary B15): the C entry point validates its arguments before any device
call, the binding flag is off by default, and the crafted face rays do what the GPU test relies on.  No test here needs a device."""
import ctypes
import inspect
import math

import numpy as np

import dreamwaltz_g_amd._lib as _lib
from dreamwaltz_g_amd import nerf, nerf_render
from tests import nerf_shading_cases as sc
from tests import raymarch_cases as rmc
from tests.test_nerf_render_host import FAKE, _desc


def _call(d, N=8, H=16, C=2, outs=(FAKE, FAKE, FAKE), bound=2.0, max_steps=256, bitfield=FAKE, shading=1, light=FAKE, ratio=0.1, eps=1e-3):
    f = ctypes.c_void_p
    return _lib.lib().dwg_nerf_render_shaded(ctypes.byref(d), f(FAKE), f(FAKE), f(FAKE), f(FAKE), N, f(bitfield) if bitfield else None,
                                             ctypes.c_float(bound), 0, ctypes.c_float(0.0), max_steps, C, H, ctypes.c_float(1e-4), 0,
                                             shading, f(light) if light else None, ctypes.c_float(ratio), ctypes.c_float(eps),
                                             *(f(o) if o else None for o in outs), None, 0, None)


def test_symbol_is_exported_and_has_a_signature():
    assert "dwg_nerf_render_shaded" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "dwg_nerf_render_shaded")
    assert len(_lib.SIGNATURES["dwg_nerf_render_shaded"][1]) == 25
    assert len(_lib.SIGNATURES["dwg_nerf_render_infer"][1]) == 21         # the albedo entry keeps its arguments


def test_bad_shading_arguments_are_refused_before_any_device_call():
    for shading in (0, 4, 255):
        assert _call(_desc(), shading=shading) != 0
    for shading in (2, 3):
        assert _call(_desc(), shading=shading, light=None) != 0
    assert _call(_desc(out_dim=5), shading=3) != 0                          # latent lambertian: five channels into four
    for eps in (0.0, -1e-3, math.nan):
        assert _call(_desc(), eps=eps) != 0
    assert _call(_desc(), shading=0, N=0) != 0 and _call(_desc(), eps=0.0, N=0) != 0        # the limits hold for an empty call too


def test_what_the_albedo_entry_refuses_is_refused():
    for outs in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert _call(_desc(), outs=outs) != 0
    assert _call(_desc(), bitfield=None) != 0
    for out_dim in (3, 6):
        assert _call(_desc(out_dim=out_dim)) != 0
    assert _call(_desc(raw=1)) != 0
    assert _call(_desc(), H=0) != 0
    assert _call(_desc(), C=9) != 0 and _call(_desc(), bound=0.0) != 0 and _call(_desc(), max_steps=0) != 0
    assert _call(_desc(), H=0, N=0) != 0


def test_no_rays_is_not_an_error():
    for precision in (0, 1):
        for out_dim in (4, 5):
            for shading in (1, 2, 3):
                if shading == 3 and out_dim == 5:
                    continue
                assert _call(_desc(out_dim=out_dim, precision=precision), N=0, outs=(None, None, None), shading=shading) == 0
    assert _call(_desc(), N=0, outs=(None, None, None), shading=1, light=None) == 0     # 'normal' reads no light


def test_shaded_render_is_off_by_default():
    assert inspect.signature(nerf.bind_nerf_network).parameters["shaded_render"].default is False
    net = sc.make_shading_network(16, 2.0).eval()
    assert nerf.bind_nerf_network(net) is None
    assert net._dwg_shaded_render is False
    # covered_call looks at the flag before it looks at any tensor
    assert not nerf_render.covered_call(net, None, None, 'normal', False)
    nerf.unbind_nerf_network(net)
    assert nerf.bind_nerf_network(net, shaded_render=True) is None
    assert net._dwg_shaded_render is True
    nerf.unbind_nerf_network(net)
    assert "_dwg_shaded_render" not in net.__dict__ and "run_cuda" not in net.__dict__


def test_dwg_bind_turns_the_shaded_render_on(monkeypatch):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "dropin"))
    monkeypatch.setenv("DWG_BIND_NERF", "1")
    import dwg_bind
    net = sc.make_shading_network(16, 2.0)
    assert dwg_bind.bind_nerf(net) is net
    assert net._dwg_shaded_render is True


def test_render_rays_refuses_bad_shading_arguments_without_a_device():
    import pytest
    net = sc.make_shading_network(16, 2.0)
    with pytest.raises(RuntimeError, match="shading"):
        nerf_render.render_rays(None, None, None, None, None, 2, 16, net.encoder, net.sigma_net, net.sigma_scale, 2.0, density_activation='exp',
                                density_prior='gaussian', albedo_sigmoid=True, shading='phong')


def test_the_face_rays_keep_the_clamp_active_on_every_sample():
    """The CPU march of the 96 crafted rays of test_nerf_shading_gpu's clamp test (dense bitfield, C = 1, H = 16, bound 1, max_steps 64):
    every ray is hit and takes 37 samples, and the coordinate normal to its face lies within epsilon of the face on every sample."""
    o, d, face = sc.face_rays()
    assert o.shape == (96, 3)
    _, bits = rmc.make_grid(1, 16, 1.0, "dense")
    counts, per_face, active, total = sc.face_check(o, d, face, bits)
    print("face rays: samples per ray %d..%d, clamp active on %d of %d, per face %s" % (counts.min(), counts.max(), active, total, per_face))
    assert (counts == 37).all(), (counts.min(), counts.max())
    assert active == total == 96 * 37
    assert (per_face == 16 * 37).all(), per_face
