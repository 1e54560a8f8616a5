"""Host-side tests of the shaded training render (boundary B19): the exported symbols, the argument checks that precede any launch, the
binding's opt-in value, the drop-in's switch and the CPU figures of the test scenes.  No test here needs a device."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from dreamwaltz_g_amd import nerf, nerf_render
from tests import nerf_field_cases as nc
from tests import nerf_render_cases as rc
from tests import nerf_shade_train_cases as stc
from tests import nerf_train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_CAPACITY = -1, -3
NEW = {"dwg_nerf.h": ("dwg_nerf_field_forward_fd", "dwg_nerf_field_backward_fd"),
       "dwg_nerf_train.h": ("dwg_nerf_train_gather_live_rows", "dwg_nerf_train_shade_forward", "dwg_nerf_train_shade_backward")}


def test_the_library_exports_the_shaded_training_render():
    L = _lib.lib()
    for header, names in NEW.items():
        text = open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            assert hasattr(L, name) and name in _lib.SIGNATURES and name in text, name
    assert os.path.exists(os.path.join(ROOT, "dreamwaltz-g_amd", "csrc", "shade_math.h"))


def _desc(precision=0, raw=0):
    net = nc.make_network()
    spec = nerf.FieldSpec(net.encoder, net.sigma_net, nc.BOUND, 'exp', 'none', True, raw, precision)
    wb = [t for lin in net.sigma_net.net for t in (lin.weight, lin.bias)]
    return net, spec.desc(net.encoder.embeddings, net.sigma_scale.reshape(1), wb)


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL pointers, misaligned buffers, a bad shading or channel count, a non-positive epsilon and a small workspace return an error
    code; empty calls return DWG_OK.  The descriptor's pointers are host addresses never dereferenced: no call here reaches a launch."""
    L = _lib.lib()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    net, d = _desc()
    eps = ctypes.c_float(1e-3)
    fwd = L.dwg_nerf_field_forward_fd
    assert fwd(ctypes.byref(d), None, 0, eps, None, None, None, None) == 0                       # M = 0
    assert fwd(ctypes.byref(d), p, 8, ctypes.c_float(0.0), p, p, p, None) == E_ARG               # epsilon
    assert fwd(ctypes.byref(d), p, 8, ctypes.c_float(float("nan")), p, p, p, None) == E_ARG
    assert fwd(ctypes.byref(d), p, 8, eps, p, p, None, None) == E_ARG                            # sigma_fd
    assert fwd(ctypes.byref(d), None, 8, eps, p, p, p, None) == E_ARG
    _, raw = _desc(raw=1)
    assert fwd(ctypes.byref(raw), p, 8, eps, p, p, p, None) == E_ARG                             # raw has no density to shift
    gr = _lib.NerfFieldGradsC()
    gr.weight[0] = 4096
    bwd = L.dwg_nerf_field_backward_fd
    assert bwd(ctypes.byref(d), None, 0, eps, None, None, None, ctypes.byref(gr), None, 0, None) == 0
    assert bwd(ctypes.byref(d), p, 8, eps, p, None, p, None, p, 1 << 30, None) == E_ARG          # grads
    assert bwd(ctypes.byref(d), p, 8, eps, p, None, None, ctypes.byref(gr), p, 1 << 30, None) == E_ARG   # dsigma_fd
    assert bwd(ctypes.byref(d), p, 8, ctypes.c_float(-1.0), p, None, p, ctypes.byref(gr), p, 1 << 30, None) == E_ARG
    assert bwd(ctypes.byref(d), p, 8, eps, p, None, p, ctypes.byref(gr), None, 1 << 30, None) == E_ARG   # workspace
    assert bwd(ctypes.byref(d), p, 8, eps, p, None, p, ctypes.byref(gr), odd, 1 << 30, None) == E_ARG    # 256-byte alignment
    assert bwd(ctypes.byref(d), p, 8, eps, p, None, p, ctypes.byref(gr), p, 16, None) == E_CAPACITY
    assert bwd(ctypes.byref(d), p, 8, eps, p, None, p, ctypes.byref(_lib.NerfFieldGradsC()), None, 0, None) == 0     # nothing asked for
    # the workspace is one dwg_nerf_field_backward call's: no sizing function of its own
    assert L.dwg_nerf_field_backward_workspace_bytes(ctypes.byref(d), 1 << 21) == L.dwg_nerf_field_backward_workspace_bytes(ctypes.byref(d), 1 << 20)
    g = L.dwg_nerf_train_gather_live_rows
    assert g(p, p, 0, 10, 5, p, p, 6, None) == 0 and g(p, p, 4, 0, 0, p, p, 6, None) == 0 and g(p, p, 4, 10, 0, p, p, 6, None) == 0
    assert g(p, p, 4, 10, 5, p, p, 0, None) == E_ARG and g(p, p, 4, 10, 5, p, p, 65, None) == E_ARG
    assert g(p, p, 4, 10, 11, p, p, 6, None) == E_ARG                                            # M_live > M
    assert g(None, p, 4, 10, 5, p, p, 6, None) == E_ARG and g(p, odd, 4, 10, 5, p, p, 6, None) == E_ARG
    assert g(p, p, 4, 10, 5, None, p, 6, None) == E_ARG and g(p, p, 4, 10, 5, p, ctypes.c_void_p(4098), 6, None) == E_ARG
    sf, sb = L.dwg_nerf_train_shade_forward, L.dwg_nerf_train_shade_backward
    r = ctypes.c_float(0.1)
    assert sf(1, None, None, 0, None, r, eps, 0, 3, None, None) == 0                             # M = 0
    assert sf(0, p, p, 0, p, r, eps, 8, 3, p, None) == E_ARG and sf(4, p, p, 0, p, r, eps, 8, 3, p, None) == E_ARG
    assert sf(4, None, None, 0, None, r, eps, 0, 3, None, None) == E_ARG                         # a bad shading is refused at M = 0 too
    assert sf(1, p, None, 0, None, r, eps, 8, 5, p, None) == E_ARG                               # channels
    assert sf(1, p, None, 0, None, r, ctypes.c_float(0.0), 8, 3, p, None) == E_ARG               # epsilon
    assert sf(2, p, None, 0, None, r, eps, 8, 3, p, None) == E_ARG                               # the lambert shadings need the light
    assert sf(3, p, None, 0, p, r, eps, 8, 3, p, None) == E_ARG                                  # 'lambertian' reads the albedo
    assert sf(3, p, p, 0, p, r, eps, 8, 4, p, None) == E_ARG                                     # ... of three channels
    assert sf(1, odd, None, 0, None, r, eps, 8, 3, p, None) == E_ARG                             # sigma_fd rows are read as pairs
    assert sf(1, p, None, 0, None, r, eps, 8, 3, None, None) == E_ARG
    assert sb(1, None, None, 0, None, r, eps, 0, 3, None, None, None, None) == 0
    assert sb(1, p, None, 0, None, r, eps, 8, 3, None, p, None, None) == E_ARG                   # grad_rgbs
    assert sb(1, p, None, 0, None, r, eps, 8, 3, p, odd, None, None) == E_ARG                    # dsigma_fd alignment
    assert sb(3, p, p, 0, p, r, eps, 8, 3, p, p, None, None) == E_ARG                            # 'lambertian' writes dalbedo
    assert sb(2, p, None, 0, None, r, eps, 8, 3, p, p, None, None) == E_ARG


def test_signatures_and_cpu_refusals():
    sig = inspect.signature(nerf_render.render_rays_train).parameters
    assert sig["shading"].default == 'albedo' and sig["light_d"].default is None and sig["ambient_ratio"].default == 1.0
    assert sig["epsilon"].default == 1e-3
    for k in ("shading", "light_d", "ambient_ratio", "epsilon"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert list(inspect.signature(nerf.bind_nerf_network).parameters) == ["ref", "shaded_render", "train_render"]
    net = rc.make_render_network(16, 1.0)
    z3, z1 = torch.zeros(4, 3), torch.zeros(4)
    args = [z3, z3.clone(), z1, z1.clone(), torch.zeros(16 ** 3 // 8, dtype=torch.uint8), 1, 16, net.encoder, net.sigma_net, net.sigma_scale, 1.0]
    kw = dict(density_activation='exp', density_prior='gaussian', albedo_sigmoid=True)
    with pytest.raises(RuntimeError, match="shading must be one of"):
        nerf_render.render_rays_train(*args, **kw, shading='phong')
    with pytest.raises(RuntimeError, match="CUDA"):
        nerf_render.render_rays_train(*args, **kw, shading='normal')


def test_the_opt_in_is_a_value_of_train_render():
    net = rc.make_render_network(16, 1.0)
    net.cuda_ray = True
    for value, want in ((False, (False, False)), (True, (True, False)), ('shaded', (True, True)), ('other', (True, False))):
        assert nerf.bind_nerf_network(net, train_render=value) is None
        assert (net._dwg_train_render, net._dwg_train_shaded) == want, value
    assert "run_cuda" in net.__dict__
    # CPU rays: no native render takes the call, whatever the flags say
    z = torch.zeros(1, 4, 3)
    net.train()
    assert not nerf_render.covered_train_call(net, z, z, 'normal') and not nerf_render.covered_train_call(net, z, z, 'albedo')
    net.eval()
    nerf.unbind_nerf_network(net)
    # the two status marks stay, as other tests read them after unbinding; everything the binding installed is gone
    left = sorted(k for k in net.__dict__ if k.startswith("_dwg_"))
    assert left == ["_dwg_nerf_bound", "_dwg_nerf_unbound"] and net._dwg_nerf_bound is False and net._dwg_nerf_unbound is None, left


_BIND_PROBE = r"""
import json, os, sys, types
sys.path.insert(0, %r); sys.path.insert(0, %r)
import dwg_import  # noqa: F401
import dwg_bind
from dreamwaltz_g_amd import nerf
calls = []
nerf.bind_nerf_network = lambda ref, *a, **kw: calls.append([list(a), kw])
dwg_bind.bind_nerf(types.SimpleNamespace())
print("DWG_NERF_TRAIN_BIND " + json.dumps(calls))
"""


def _bind_probe(value):
    env = dict(os.environ)
    env.pop("DWG_BIND_NERF_TRAIN", None)
    env.pop("DWG_BIND_NERF", None)
    if value is not None:
        env["DWG_BIND_NERF_TRAIN"] = value
    r = subprocess.run([sys.executable, "-c", _BIND_PROBE % (ROOT, os.path.join(ROOT, "dropin"))], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DWG_NERF_TRAIN_BIND ")][-1]
    return json.loads(line[len("DWG_NERF_TRAIN_BIND "):])


def test_the_drop_in_binds_the_shaded_training_render_only_on_request():
    assert _bind_probe("shaded") == [[[], {"shaded_render": True, "train_render": "shaded"}]]
    assert _bind_probe("1") == [[[], {"shaded_render": True, "train_render": True}]]
    assert _bind_probe(None) == _bind_probe("0") == [[[], {"shaded_render": True}]]


@pytest.mark.parametrize("C,H,n,seed", tc.SCENES[:2])
def test_cpu_figures_of_the_scenes(C, H, n, seed):
    """The camera scenes on the CPU (numpy march, nerf_field_cases.restate at the seven fp32 points, live samples only): every live
    sample has a non-zero finite normal, about half are lit by LIGHT, the clamp of the shifted points is active on none, and the
    magnification 0.5 / (eps |g|) stays below 500.  5 rays: M 163, M_live 69, least |g| 56; 1000 rays: 84 333 / 76 689, least |g| 1.7."""
    fig = stc.host_figures(C, H, n, seed)
    print("host figures:", fig)
    assert (fig["M"], fig["M_live"]) == {5: (163, 69), 1000: (84333, 76689)}[n]
    assert fig["nonzero_normal"] == 1.0 and fig["below_clamp"] == 0 and fig["non_finite"] == 0 and fig["clamp_active"] == 0
    assert fig["g_min"] > (50 if n == 5 else 1.5) and fig["g_max"] < 4e4
    if n >= 1000:
        assert 0.49 <= fig["lit"] <= 0.51, fig


def test_the_crafted_scenes_reach_their_branches():
    """(a) the perturbed face rays: the clamp is active on at least one LIVE sample of each of the six faces.  (b) the flat field: the
    density is one constant, so every normal is exactly zero."""
    per_face, M, M_live = stc.face_live_check()
    print("face rays: M %d, M_live %d, live samples with the clamp active per face %s" % (M, M_live, per_face))
    assert (per_face >= 1).all() and 0 < M_live <= M
    net = stc.flat_network(16, 1.0)
    x = nc.make_points(256, seed=5, bound=1.0)
    with torch.no_grad():
        s0 = nc.restate(net, x)[0].numpy()
        sfd = np.stack([nc.restate(net, p)[0].numpy() for p in stc.shifted(x, 1.0)], -1)
    assert (sfd == s0[:, None]).all() and s0.min() == s0.max() > 0
    g, n = stc.normals(sfd)
    assert (g == 0).all() and (n == 0).all()
