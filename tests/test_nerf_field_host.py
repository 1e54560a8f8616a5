"""CPU-side checks of the fused NeRF field (boundary B7): argument errors before any launch, the float64 restatement's gradients, and the
B7 binding decisions on the reference's own network classes (in a subprocess; skipped when the reference tree is absent)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import nerf_field_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "dropin")
REFERENCE = "/root/reference"


def _desc(**over):
    from dreamwaltz_g_amd import _lib
    d = _lib.NerfFieldDescC()
    d.embeddings, d.offsets = 0x1000, 0x2000
    d.num_levels, d.log2_per_level_scale, d.base_resolution = 16, 0.5, 16
    d.gridtype, d.align_corners, d.interp, d.bound = 1, 0, 1, 2.0
    d.num_layers, d.hidden, d.out_dim = 3, 64, 4
    for l in range(3):
        d.weight[l], d.bias[l] = 0x3000 + 0x100 * l, 0x4000 + 0x100 * l
    d.density_activation, d.density_prior, d.albedo_sigmoid, d.raw = 0, 0, 1, 0
    d.sigma_scale, d.precision = 0x5000, 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


BAD = [dict(num_levels=0), dict(num_levels=33), dict(num_layers=0), dict(num_layers=5), dict(hidden=65), dict(out_dim=1), dict(out_dim=17),
       dict(precision=2), dict(density_activation=3), dict(density_prior=3), dict(gridtype=2), dict(interp=2), dict(bound=0.0),
       dict(bound=float("nan")), dict(embeddings=None), dict(offsets=None)]


@pytest.mark.parametrize("over", BAD, ids=[",".join("%s=%s" % kv for kv in o.items()) for o in BAD])
def test_bad_descriptors_are_rejected_before_any_launch(over):
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    d = _desc(**over)
    x = ctypes.c_void_p(0x6000)
    assert L.dwg_nerf_field_forward(ctypes.byref(d), x, 1000, x, x, None) == -1
    g = _lib.NerfFieldGradsC()
    assert L.dwg_nerf_field_backward(ctypes.byref(d), x, 1000, x, x, ctypes.byref(g), None, 0, None) == -1
    assert L.dwg_nerf_field_backward_workspace_bytes(ctypes.byref(d), 1000) == 0


def test_null_and_empty_calls_launch_nothing():
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    d = _desc()
    x = ctypes.c_void_p(0x6000)
    g = _lib.NerfFieldGradsC()
    assert L.dwg_nerf_field_forward(None, x, 10, x, x, None) == -1
    assert L.dwg_nerf_field_forward(ctypes.byref(d), x, 0, None, None, None) == 0           # M == 0: nothing to do
    assert L.dwg_nerf_field_forward(ctypes.byref(d), None, 10, x, x, None) == -1
    assert L.dwg_nerf_field_backward(ctypes.byref(d), x, 0, x, x, ctypes.byref(g), None, 0, None) == 0
    assert L.dwg_nerf_field_backward(ctypes.byref(d), x, 10, x, x, None, None, 0, None) == -1
    g.sigma_scale = 0x7000          # sigma_scale gradient without the `scaling` activation
    assert L.dwg_nerf_field_backward(ctypes.byref(d), x, 10, x, x, ctypes.byref(g), None, 0, None) == -1
    g.sigma_scale = None
    g.embeddings = 0x7000           # a table gradient needs the host copy of the offsets
    assert L.dwg_nerf_field_backward(ctypes.byref(d), x, 10, x, x, ctypes.byref(g), None, 0, None) == -1


def test_python_checks_raise_before_launch():
    from dreamwaltz_g_amd import nerf
    net = nc.make_network(seed=1)
    x = torch.from_numpy(nc.make_points(64, seed=1))
    with pytest.raises(RuntimeError, match="CUDA"):
        nerf.nerf_field(x, net.encoder, net.sigma_net, net.sigma_scale, net.bound, precision=0)
    with pytest.raises(RuntimeError, match="density_activation"):
        nerf.nerf_field(x, net.encoder, net.sigma_net, net.sigma_scale, net.bound, density_activation="relu", precision=0)
    with pytest.raises(RuntimeError, match="gradient with respect to x"):
        nerf.nerf_field(x.requires_grad_(True), net.encoder, net.sigma_net, net.sigma_scale, net.bound, precision=0)


@pytest.mark.parametrize("act,prior,latent", [("exp", "gaussian", False), ("softplus", "sqrt", True), ("scaling", "none", False)])
def test_restatement_gradient_equals_finite_differences(act, prior, latent):
    """The float64 restatement differentiates as the composition it writes out: torch.autograd.gradcheck over sigma_scale, every weight and
    bias and a few table rows, on a small network."""
    net = nc.make_network(L=2, hidden=8, num_layers=3, density_activation=act, density_prior=prior, latent_mode=latent,
                          additional_dim_size=1 if latent else 0, seed=3, log2_hashmap_size=8)
    x = nc.make_points(6, seed=3, edge=False)

    s, a, leaves = nc.restate(net, x)
    names = [k for k in leaves if k != 'embeddings'] + ['embeddings']
    base = {k: v.detach().clone() for k, v in leaves.items()}

    def f(*vals):
        lv = dict(zip(names, vals))
        h = nc.oa.grid_encode((torch.from_numpy(x) + np.float32(2.0)) * np.float32(0.25), lv["embeddings"],
                              net.encoder.offsets.numpy().astype(np.int64), net.encoder.per_level_scale, net.encoder.base_resolution,
                              gridtype=net.encoder.gridtype_id, align_corners=False, interp=net.encoder.interp_id)
        n = len(net.sigma_net.net)
        for l in range(n):
            h = torch.nn.functional.linear(h, lv['w%d' % l], lv['b%d' % l])
            if l != n - 1:
                h = torch.relu(h)
        return h

    # the restatement's autograd gradient equals autograd of the written-out float64 composition (same graph built independently)
    ws = torch.randn(6, dtype=torch.float64)
    wa = torch.randn(6, a.shape[1], dtype=torch.float64)
    ((s * ws).sum() + (a * wa).sum()).backward()
    vals = [base[k].clone().requires_grad_(True) for k in names]
    h = f(*vals)
    sig, alb = h[:, 0], h[:, 1:]
    if not latent:
        alb = torch.sigmoid(alb)
    x64 = torch.from_numpy(x).double()
    pre = sig
    if prior != 'none':
        d = (x64 ** 2).sum(-1)
        pre = pre + (5 * torch.exp(-d / 0.08) if prior == 'gaussian' else 10 * (1 - torch.sqrt(d) / 0.5))
    ss = vals[names.index('sigma_scale')]
    sig = torch.exp(pre) if act == 'exp' else torch.nn.functional.softplus(pre) if act == 'softplus' else \
        torch.nn.functional.softplus(pre * torch.exp(ss) - 1.0)
    ((sig * ws).sum() + (alb * wa).sum()).backward()
    for k, v in zip(names, vals):
        g = v.grad if v.grad is not None else torch.zeros_like(v)
        lg = leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(v)
        assert torch.allclose(lg, g, rtol=1e-12, atol=1e-14), k
    # and gradcheck (finite differences) of the MLP and activation part
    mlp_names = [k for k in names if k != 'embeddings']
    idx = [names.index(k) for k in mlp_names]

    def g_fn(*mv):
        vv = [base[k] for k in names]
        for i, m in zip(idx, mv):
            vv[i] = m
        hh = f(*vv)
        s_ = hh[:, 0]
        pr = s_
        if prior != 'none':
            d = (x64 ** 2).sum(-1)
            pr = pr + (5 * torch.exp(-d / 0.08) if prior == 'gaussian' else 10 * (1 - torch.sqrt(d) / 0.5))
        sc = vv[names.index('sigma_scale')]
        return (torch.exp(pr) if act == 'exp' else torch.nn.functional.softplus(pr) if act == 'softplus' else
                torch.nn.functional.softplus(pr * torch.exp(sc) - 1.0)), hh[:, 1:]
    assert torch.autograd.gradcheck(g_fn, [base[k].clone().requires_grad_(True) for k in mlp_names], eps=1e-6, atol=1e-5)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "core", "nerf")), reason="reference tree not present")
def test_b7_binding_decisions_on_the_reference_network():
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
out = {"hooked": bool(getattr(nm.build_NeRFNetwork, "__dwg_bound__", False))}
def decide(**kw):
    n = nm.build_NeRFNetwork(NeRFConfig(**kw))
    return [type(n).__name__, bool(getattr(n, "_dwg_nerf_bound", False)), getattr(n, "_dwg_nerf_unbound", None),
            "common_forward" in n.__dict__ and "local_geometry_forward" in n.__dict__]
out["default"] = decide()
out["dual_mlp"] = decide(structure="dual_mlp")
out["smpl"] = decide(density_prior="smpl")
out["latent_tune"] = decide(nerf_type="latent_tune")
print(json.dumps(out))
""" % (ROOT, DROPIN, REFERENCE)
    env = dict(os.environ)
    env.pop("DWG_BIND_NERF", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["hooked"]
    assert out["default"][:2] == ["_NeRFNetwork", True] and out["default"][2] is None and out["default"][3]
    for k in ("dual_mlp", "smpl", "latent_tune"):
        assert out[k][1] is False and out[k][2] and not out[k][3], (k, out[k])
    assert "dual" in out["dual_mlp"][2] and "smpl" in out["smpl"][2] and "decoder_layer" in out["latent_tune"][2]
    env["DWG_BIND_NERF"] = "0"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("default", "dual_mlp", "smpl", "latent_tune"):
        assert out[k][1] is False and out[k][2] is None and not out[k][3], (k, out[k])
