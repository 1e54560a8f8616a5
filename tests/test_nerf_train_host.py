"""Host-side tests of the training render (boundary B18): the exported symbols, the argument checks that precede any launch, the CPU
figures of the test scenes, and the drop-in binding's switch."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import dreamwaltz_g_amd._lib as _lib
from dreamwaltz_g_amd import nerf_render
from tests import nerf_render_cases as rc
from tests import nerf_train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_CAPACITY = -1, -3


def test_the_library_exports_the_training_render():
    L = _lib.lib()
    for name in ("dwg_raymarch_composite_rays_train_forward_live", "dwg_nerf_train_workspace_bytes", "dwg_nerf_train_compact_offsets",
                 "dwg_nerf_train_gather_live"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert "dwg_nerf_train_gather_live" in open(os.path.join(ROOT, "include", "dwg_nerf_train.h")).read()
    assert L.dwg_nerf_train_workspace_bytes(0) == 0
    assert L.dwg_nerf_train_workspace_bytes(1024) == 4 and L.dwg_nerf_train_workspace_bytes(1025) == 8


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    """NULL pointers, misaligned buffers, a bad channel count and a small workspace return an error code; empty calls return DWG_OK.
    The pointers are never dereferenced on the host and no call here reaches a launch."""
    L = _lib.lib()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    fwd = L.dwg_raymarch_composite_rays_train_forward_live
    assert fwd(p, p, p, p, 10, 0, 3, 1e-4, 0, p, p, p, p, p, None) == 0                          # N = 0
    assert fwd(p, p, p, p, 10, 4, 5, 1e-4, 0, p, p, p, p, p, None) == E_ARG                      # channels
    assert fwd(p, p, p, p, 10, 4, 3, 1e-4, 0, p, p, p, p, None, None) == E_ARG                   # live
    assert fwd(None, p, p, p, 10, 4, 3, 1e-4, 0, None, p, p, p, p, None) == E_ARG                # sigmas with M > 0
    assert fwd(p, p, odd, p, 10, 4, 3, 1e-4, 0, None, p, p, p, p, None) == E_ARG                 # ts not 8-byte aligned
    assert fwd(p, ctypes.c_void_p(4104), p, p, 10, 4, 4, 1e-4, 0, None, p, p, p, p, None) == E_ARG   # four channels: 16-byte rows
    off = L.dwg_nerf_train_compact_offsets
    assert off(None, 0, None, None, None, 0, None) == 0                                          # N = 0
    assert off(None, 8, p, p, p, 4, None) == E_ARG and off(p, 8, None, p, p, 4, None) == E_ARG
    assert off(p, 8, p, None, p, 4, None) == E_ARG and off(p, 8, odd, p, p, 4, None) == E_ARG
    assert off(p, 8, p, p, None, 4, None) == E_ARG
    assert off(p, 2000, p, p, p, 4, None) == E_CAPACITY
    g = L.dwg_nerf_train_gather_live
    assert g(p, p, 0, 10, 5, p, p, p, p, p, p, p, p, 3, 0, None) == 0                            # N = 0
    assert g(p, p, 4, 0, 0, p, p, p, p, p, p, p, p, 3, 0, None) == 0                             # M = 0
    assert g(p, p, 4, 10, 0, p, p, p, p, p, p, p, p, 3, 0, None) == 0                            # M_live = 0
    assert g(p, p, 4, 10, 5, p, p, p, p, p, p, p, p, 2, 0, None) == E_ARG                        # channels
    assert g(p, p, 4, 10, 5, p, p, p, p, p, p, p, p, 3, 2, None) == E_ARG                        # rgbs_f16
    assert g(p, p, 4, 10, 11, p, p, p, p, p, p, p, p, 3, 0, None) == E_ARG                       # M_live > M
    assert g(p, p, 4, 10, 5, p, None, p, p, p, p, p, p, 3, 0, None) == E_ARG                     # a source without its destination
    assert g(None, p, 4, 10, 5, p, p, p, p, p, p, p, p, 3, 0, None) == E_ARG
    assert g(p, None, 4, 10, 5, p, p, p, p, p, p, p, p, 3, 0, None) == E_ARG
    assert g(p, p, 4, 10, 5, p, p, p, p, p, p, p, ctypes.c_void_p(4098), 3, 0, None) == E_ARG    # fp32 rgbs_live at a 2-byte address
    assert g(p, p, 4, 10, 5, None, None, None, None, None, None, None, None, 3, 0, None) == 0    # nothing named: nothing to move


def _cpu_args(n=4):
    net = rc.make_render_network(16, 1.0)
    z3, z1 = torch.zeros(n, 3), torch.zeros(n)
    bits = torch.zeros(16 ** 3 // 8, dtype=torch.uint8)
    kw = dict(density_activation='exp', density_prior='gaussian', albedo_sigmoid=True)
    return net, [z3, z3.clone(), z1, z1.clone(), bits, 1, 16, net.encoder, net.sigma_net, net.sigma_scale, 1.0], kw


def test_render_rays_train_refuses_cpu_tensors_and_bad_arguments():
    net, args, kw = _cpu_args()
    with pytest.raises(RuntimeError, match="CUDA"):
        nerf_render.render_rays_train(*args, **kw)
    with pytest.raises(RuntimeError):
        nerf_render.render_rays_train(*args, **dict(kw, density_activation='relu'))
    with pytest.raises(RuntimeError):
        nerf_render.render_rays_train(*args, **dict(kw, density_prior='smpl'))
    with pytest.raises(TypeError):
        nerf_render.render_rays_train(*args)                       # the field's settings are keyword-only and required


def test_binding_signature_and_default():
    import inspect
    from dreamwaltz_g_amd import nerf
    sig = inspect.signature(nerf.bind_nerf_network)
    assert list(sig.parameters) == ["ref", "shaded_render", "train_render"]
    assert sig.parameters["train_render"].default is False and sig.parameters["shaded_render"].default is False
    names = list(inspect.signature(nerf_render.render_rays_train).parameters)
    assert names[:11] == ["rays_o", "rays_d", "nears", "fars", "density_bitfield", "cascade", "grid_size", "encoder", "sigma_net", "sigma_scale",
                          "bound"]
    for k in ("perturb", "noises", "counter", "return_weights", "return_sigmas", "return_stats", "T_thresh", "binarize", "contract", "precision"):
        assert inspect.signature(nerf_render.render_rays_train).parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k


@pytest.mark.parametrize("C,H,n,seed", tc.SCENES)
def test_cpu_figures_of_the_scenes(C, H, n, seed):
    """The scenes of the GPU tests, on the CPU without a device: raymarch_cases.march_train (max_steps 1024, noises RandomState(seed +
    100)), nerf_field_cases.restate for the density, stop = first post-sample T < 1e-4, inclusive.  f32, three albedo channels:
    (1, 16, 5, 1): M 163, M_live 69; (2, 32, 1000, 9): 84 333 / 76 689, 130 cut / 745 whole / 125 without a sample, longest 190;
    (2, 64, 3000, 3): 172 556 / 164 269, 138 / 2203 / 659, longest 212, 2 borderline."""
    want = {5: (163, 69, 1, 1, 3, 148, 0), 1000: (84333, 76689, 130, 745, 125, 190, 0), 3000: (172556, 164269, 138, 2203, 659, 212, 2)}[n]
    fig = tc.host_figures(C, H, n, seed)
    print("host figures:", fig)
    assert (fig["M"], fig["M_live"], fig["cut"], fig["whole"], fig["no_sample"], fig["longest"], fig["borderline"]) == want, fig
    if n >= 1000:
        tc.assert_fair(fig, n)


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


def test_the_drop_in_binds_the_training_render_only_on_request():
    """Without DWG_BIND_NERF_TRAIN the drop-in's call of bind_nerf_network is the one it made before this switch existed."""
    assert _bind_probe(None) == [[[], {"shaded_render": True}]]
    assert _bind_probe("0") == [[[], {"shaded_render": True}]]
    assert _bind_probe("1") == [[[], {"shaded_render": True, "train_render": True}]]
