"""CPU checks of the learned background (boundary B22): csrc/freq_math.h compiled for the host as a stand-alone program against the
float64 restatement, the model classes and their optimizer groups, the argument checks of nerf_background.learned_background and the
decisions of nerf_view.covered_view.  Needs no device.

THE BOUND of the encoding.  Columns 0..2 are the input: exact.  Every other column is sinf or cosf of scalbnf(x, f), which is exact, so
its error is that of the host's sinf / cosf on an exact argument of magnitude at most 2^5 (degree 6, |x| <= 1).  Measured in this run on
this file's 300 directions per degree (1, 6 and 8): max |error| 3.23e-8, a little over 2^-25 = 2.98e-8, half an ulp of a value in
[0.5, 1) -- the host's functions are within 0.55 ulp here.  FREQ_ERR records it; the test asserts no more than twice that."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import nerf_background_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32
FREQ_ERR = 3.23e-8           # measured: see the module docstring
E_ARG = -1


@pytest.fixture(scope="module")
def freq_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("freq_math") / "freq_math_host"
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-o", str(exe),
                    os.path.join(HERE, "hostmath", "freq_math_host.c"), "-lm"], check=True)
    return str(exe)


def _host_encode(exe, x, degree):
    r = subprocess.run([exe, str(degree), str(len(x))], input=np.ascontiguousarray(x, f32).tobytes(), capture_output=True, check=True, timeout=60)
    return np.frombuffer(r.stdout, f32).reshape(len(x), 3 + 6 * degree)


@pytest.mark.parametrize("degree", [6, 1, 8])
def test_freq_math_on_the_host_against_float64(freq_program, degree):
    x = bc.directions(300, seed=degree)
    assert (np.abs(x[:6]).sum(1) == 1).all() and (x[:6] != 0).sum() == 6                 # the axis-aligned directions
    assert np.abs(x[np.abs(x) > 0]).min() == 2.0 ** -149                                 # ... and the smallest magnitude there is
    got = _host_encode(freq_program, x, degree)
    assert got.shape == (300, 3 + 6 * degree)
    want = bc.encode(torch.from_numpy(x), degree).numpy()
    # the layout, index by index: c = 3 + (2 f + s) * 3 + d
    x64 = x.astype(np.float64)
    for c in range(3 + 6 * degree):
        kind, f, d = bc.column(degree, c)
        col = x64[:, d] if kind == 'x' else (np.sin if kind == 'sin' else np.cos)(2.0 ** f * x64[:, d])
        assert np.abs(col - want[:, c]).max() <= 4e-16, c                               # the restatement has the issue's layout
        if kind == 'x':
            assert np.array_equal(got[:, c], x[:, d]), c
    err = np.abs(got.astype(np.float64) - want)
    worst = float(err.max())
    print("freq_math host degree %d: max |error| %.3g (FREQ_ERR %.3g), worst column %d" % (degree, worst, FREQ_ERR, int(err.max(0).argmax())))
    assert worst <= 2 * FREQ_ERR
    # the exact columns of the axis-aligned rows: sin(0) = 0, cos(0) = 1
    zero = x[:6] == 0
    for c in range(3, 3 + 6 * degree):
        kind, f, d = bc.column(degree, c)
        assert (got[:6, c][zero[:, d]] == (0.0 if kind == 'sin' else 1.0)).all()


def _cfg(**kw):
    from dreamwaltz_g_amd import configs
    c = configs.NeRFConfig(bound=1.0, grid_size=16, num_levels=4, desired_resolution=128)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_the_factory_picks_the_class_and_nerf_network_still_refuses():
    from dreamwaltz_g_amd import nerf_model
    net = nerf_model.build_nerf_network(_cfg())
    assert type(net) is nerf_model.NeRFNetwork and net.bg_net is None and net.bg_radius == 0.0
    bg = nerf_model.build_nerf_network(_cfg(bg_mode='nerf'))
    assert type(bg) is nerf_model.BackgroundNeRFNetwork and isinstance(bg, nerf_model.NeRFNetwork)
    assert bg.bg_mode == 'nerf' and bg.bg_radius == _cfg().bg_radius and bg.decoder_layer is None
    assert type(nerf_model.build_nerf_network(_cfg(bg_mode='nerf'), hidden_dim_bg=32, num_layers_bg=3)) is nerf_model.BackgroundNeRFNetwork
    with pytest.raises(NotImplementedError, match="'nerf' background"):
        nerf_model.NeRFNetwork(_cfg(bg_mode='nerf'))
    with pytest.raises(NotImplementedError, match="hidden width"):
        nerf_model.BackgroundNeRFNetwork(_cfg(bg_mode='nerf'), hidden_dim_bg=48)
    for kw, word in ((dict(dmtet=True), "dmtet"), (dict(cuda_ray=False), "cuda_ray"), (dict(nerf_type='latent_tune'), "latent_tune")):
        with pytest.raises(NotImplementedError, match=word):
            nerf_model.BackgroundNeRFNetwork(_cfg(bg_mode='nerf', **kw))


def test_background_network_has_the_references_modules_and_state_dict_keys():
    from dreamwaltz_g_amd import nerf_model, nerf_background
    plain = nerf_model.NeRFNetwork(_cfg())
    for latent, C in ((False, 3), (True, 4)):
        net = nerf_model.BackgroundNeRFNetwork(_cfg(bg_mode='nerf', nerf_type='latent' if latent else 'rgb'))
        enc = net.encoder_bg
        assert isinstance(enc, nerf_background.FreqEncoder) and (enc.input_dim, enc.degree, enc.output_dim) == (3, 6, 39)
        assert list(enc.parameters()) == [] and net.in_dim_bg == 39
        sd = net.state_dict()
        new = {k: tuple(v.shape) for k, v in sd.items() if k not in plain.state_dict()}
        assert new == {'bg_net.net.0.weight': (64, 39), 'bg_net.net.0.bias': (64,), 'bg_net.net.1.weight': (C, 64), 'bg_net.net.1.bias': (C,)}
        assert set(plain.state_dict()) <= set(sd)
    with pytest.raises(NotImplementedError, match="input_dim"):
        nerf_background.FreqEncoder(input_dim=2)
    assert repr(nerf_background.FreqEncoder(3, 4)) == "FreqEncoder: input_dim=3 degree=4 output_dim=27"


def test_get_optimizer_adds_the_bg_net_group():
    from dreamwaltz_g_amd import nerf_model, optim
    cfg = _cfg(bg_mode='nerf', lr=2e-3, bg_lr=5e-4)
    net = nerf_model.BackgroundNeRFNetwork(cfg)
    opts, scheduler = net.get_optimizer(cfg)
    assert scheduler is None and isinstance(opts, optim.FlatOptimizerDict) and list(opts) == ['nerf']
    o = opts['nerf']
    assert [pg['name'] for pg in o.param_groups] == ['encoder', 'sigma_net', 'sigma_scale', 'bg_net']
    assert [pg['lr'] for pg in o.param_groups] == [2e-3 * 10, 2e-3, 2e-3, 5e-4]
    assert all(pg['betas'] == (0.9, 0.99) and pg['eps'] == 1e-15 for pg in o.param_groups)
    assert [len(pg['params']) for pg in o.param_groups] == [1, 6, 1, 4]
    assert [p is q for p, q in zip(o.param_groups[3]['params'], net.bg_net.parameters())] == [True] * 4
    # the other three groups are NeRFNetwork's: same names, rates, parameters and ranges
    plain_cfg = _cfg(lr=2e-3, bg_lr=5e-4)
    po = nerf_model.NeRFNetwork(plain_cfg).get_optimizer(plain_cfg)[0]['nerf']
    for a, b in zip(o.param_groups[:3], po.param_groups):
        assert {k: v for k, v in a.items() if k != 'params'} == {k: v for k, v in b.items() if k != 'params'}
        assert [tuple(p.shape) for p in a['params']] == [tuple(p.shape) for p in b['params']]
    assert o.param_groups[3]['start'] >= o.param_groups[2]['end'] and all(opts.buffers.owns_grad(p) for p in net.parameters())


def test_learned_background_refuses_bad_arguments_before_the_library(monkeypatch):
    from dreamwaltz_g_amd import _lib, nerf_background as nb

    def untouched():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", untouched)
    enc, bg = bc.make_bg()
    d = torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        nb.learned_background(d, enc, bg)
    with pytest.raises(RuntimeError, match="CUDA"):
        nb.freq_encode(d)
    with pytest.raises(RuntimeError, match="float32|CUDA"):
        nb.learned_background(d.double(), enc, bg)
    with pytest.raises(RuntimeError, match=r"\[\.\.\., 3\]"):
        nb.learned_background(torch.zeros(8, 4), enc, bg)
    with pytest.raises(RuntimeError, match="tensor"):
        nb.learned_background(d.numpy(), enc, bg)
    with pytest.raises(RuntimeError, match="require grad"):
        nb.learned_background(d.clone().requires_grad_(True), enc, bg)
    with pytest.raises(RuntimeError, match="require grad"):
        nb.freq_encode(d.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="precision"):
        nb.learned_background(d, enc, bg, precision=2)
    with pytest.raises(RuntimeError, match="degree"):
        nb.freq_encode(d, degree=9)
    with pytest.raises(RuntimeError, match="degree"):
        nb.freq_encode(d, degree=0)
    # the fake device tensor passes the device checks: what is left to refuse is the shape of the network
    monkeypatch.setattr(_lib, "check_tensor", lambda *a, **k: None)
    for kw, word in ((dict(layers=4), "layers"), (dict(hidden=48), "hidden width"), (dict(hidden=128), "hidden width"), (dict(C=5), "output width"),
                     (dict(C=2), "output width")):
        e, b = bc.make_bg(**kw)
        with pytest.raises(RuntimeError, match=word):
            nb.learned_background(d, e, b)
    for degree in (0, 9, 6.0, None):
        with pytest.raises(RuntimeError, match="degree"):
            nb.learned_background(d, types.SimpleNamespace(input_dim=3, degree=degree), bg)
    with pytest.raises(RuntimeError, match="3 inputs"):
        nb.learned_background(d, types.SimpleNamespace(input_dim=2, degree=6), bg)
    e, b = bc.make_bg()
    b.net[0] = torch.nn.Linear(39, 64, bias=False)
    with pytest.raises(RuntimeError, match="biased"):
        nb.learned_background(d, e, b)
    e, b = bc.make_bg(degree=4)
    with pytest.raises(RuntimeError, match="expected 39 -> 64"):
        nb.learned_background(d, types.SimpleNamespace(input_dim=3, degree=6), b)
    with pytest.raises(RuntimeError, match="layers"):
        nb.learned_background(d, e, types.SimpleNamespace())
    monkeypatch.undo()
    # the real check is back
    with pytest.raises(RuntimeError, match="CUDA"):
        nb.learned_background(d, *bc.make_bg())


def test_the_c_entry_points_refuse_unsupported_descriptors():
    """Host only: every refusal comes before a launch."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)

    def desc(**kw):
        d = _lib.NerfBgDescC()
        d.degree, d.num_layers, d.hidden, d.out_dim, d.sigmoid, d.precision = 6, 2, 64, 3, 1, 0
        for l in range(3):
            d.weight[l], d.bias[l] = 4096, 4096
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    good = desc()
    assert L.dwg_nerf_bg_backward_workspace_bytes(ctypes.byref(good)) == 512 * (39 * 64 + 64 + 64 * 3 + 3) * 4
    assert L.dwg_nerf_bg_forward(0, None, ctypes.byref(good), None, None) == 0                       # no rays: nothing to launch
    g = _lib.NerfBgGradsC()
    for kw in (dict(degree=0), dict(degree=9), dict(num_layers=0), dict(num_layers=4), dict(hidden=48), dict(hidden=128), dict(out_dim=2),
               dict(out_dim=5), dict(precision=2), dict(sigmoid=2)):
        d = desc(**kw)
        assert L.dwg_nerf_bg_forward(64, p, ctypes.byref(d), p, None) == E_ARG, kw
        assert L.dwg_nerf_bg_backward_workspace_bytes(ctypes.byref(d)) == 0, kw
        assert L.dwg_nerf_bg_backward(64, p, p, ctypes.byref(d), ctypes.byref(g), p, 1 << 30, None) == E_ARG, kw
    d = desc()
    d.bias[1] = None
    assert L.dwg_nerf_bg_forward(64, p, ctypes.byref(d), p, None) == E_ARG                           # an unbiased layer
    assert L.dwg_nerf_bg_forward(64, None, ctypes.byref(good), p, None) == E_ARG
    assert L.dwg_nerf_bg_forward(1 << 31, p, ctypes.byref(good), p, None) == E_ARG
    assert L.dwg_nerf_bg_backward(64, p, p, ctypes.byref(good), ctypes.byref(g), None, 0, None) == 0  # no gradient asked for
    g.weight[0] = 4096
    assert L.dwg_nerf_bg_backward(64, p, p, ctypes.byref(good), ctypes.byref(g), None, 0, None) == E_ARG
    assert L.dwg_nerf_bg_backward(64, p, p, ctypes.byref(good), ctypes.byref(g), ctypes.c_void_p(4100), 1 << 30, None) == E_ARG
    assert L.dwg_nerf_bg_backward(64, p, p, ctypes.byref(good), ctypes.byref(g), p, 1024, None) == -3  # DWG_E_CAPACITY
    assert L.dwg_nerf_freq_encode(64, p, 0, p, None) == E_ARG and L.dwg_nerf_freq_encode(64, p, 9, p, None) == E_ARG
    assert L.dwg_nerf_freq_encode(64, None, 6, p, None) == E_ARG and L.dwg_nerf_freq_encode(0, None, 6, None, None) == 0


def test_ctypes_mirrors_of_the_background_structs(tmp_path):
    from dreamwaltz_g_amd import _lib
    for struct, mirror in (("dwg_nerf_bg_desc", _lib.NerfBgDescC), ("dwg_nerf_bg_grads", _lib.NerfBgGradsC)):
        names = [f[0] for f in mirror._fields_]
        src, exe = tmp_path / (struct + ".c"), tmp_path / struct
        lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dwg_nerf_background.h"', 'int main(void) {',
                 '  printf("%%zu\\n", sizeof(%s));' % struct]
        lines += ['  printf("%%zu\\n", offsetof(%s, %s));' % (struct, f) for f in names] + ['  return 0; }']
        src.write_text("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert out[0] == ctypes.sizeof(mirror) and out[1:] == [getattr(mirror, n).offset for n in names], struct


class _StubNet:
    """What nerf_view.covered_view reads of a reference network (tests/test_nerf_view_host.py's stub)."""

    def __init__(self, **kw):
        self.training, self.cuda_ray, self.dmtet = False, True, False
        self.bg_mode, self.bg_colors = 'gray', {'gray': None, 'white': None, 'black': None}
        self.aabb_train = self.aabb_infer = torch.zeros(6)
        self.__dict__.update(kw)


def test_covered_view_decisions_for_the_learned_background(monkeypatch):
    from dreamwaltz_g_amd import nerf_view, nerf_render
    seen = []
    monkeypatch.setattr(nerf_render, "covered_call", lambda ref, o, d, shading, perturb, light_d=None: seen.append(shading) or True)
    monkeypatch.setattr(nerf_render, "covered_train_call", lambda ref, o, d, shading, light_d=None: seen.append(shading) or True)
    monkeypatch.setattr(nerf_view, "_camera_ok", lambda t, tail: isinstance(t, torch.Tensor) and t.dtype == torch.float32
                        and tuple(t.shape) == (1,) + tuple(tail))
    data = {'c2w': torch.eye(4)[None], 'intrinsics': torch.eye(3)[None], 'image_height': 5, 'image_width': 7}
    enc, bg = bc.make_bg()
    with_bg = dict(bg_net=bg, encoder_bg=enc, decoder_layer=None)
    assert nerf_view.covered_view(_StubNet(bg_mode='nerf', **with_bg), data) and seen == ['albedo']
    assert nerf_view.covered_view(_StubNet(**with_bg), data, bg_mode='nerf')                       # asked for at the call
    assert nerf_view.covered_view(_StubNet(bg_mode='nerf', bg_net=bg, encoder_bg=enc), data)       # a network without the attribute
    n = len(seen)
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf'), data)                              # no bg_net
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf', bg_net=None, encoder_bg=enc), data)
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf', bg_net=bg), data)                   # no encoder_bg
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf', **dict(with_bg, decoder_layer=torch.nn.Linear(4, 3, bias=False))), data)
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf', **dict(with_bg, encoder_bg=types.SimpleNamespace(input_dim=3, degree=12))), data)
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf', **dict(with_bg, bg_net=bc.make_bg(hidden=128)[1])), data)
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf', **dict(with_bg, bg_net=bc.make_bg(layers=4)[1])), data)
    assert not nerf_view.covered_view(_StubNet(bg_mode='nerf', **with_bg), dict(data, c2w=torch.eye(4)[None].double()))
    assert len(seen) == n                                                                          # no refusal reached the render's own check
    # the parameters must live where the camera does
    cam = types.SimpleNamespace(device=torch.device("meta"))
    assert nerf_view._learned_background_reason(_StubNet(**with_bg), torch.device("cpu")) is None
    assert "not on" in nerf_view._learned_background_reason(_StubNet(**with_bg), cam.device)
    # render_view keeps refusing a network without bg_net, whoever asks
    with pytest.raises(NotImplementedError, match="'nerf' background"):
        nerf_view.render_view(_StubNet(bg_mode='nerf'), data)
    with pytest.raises(NotImplementedError, match="'nerf' background"):
        nerf_view.render_view(_StubNet(**dict(with_bg, decoder_layer=torch.nn.Linear(4, 3, bias=False))), data, bg_mode='nerf')
