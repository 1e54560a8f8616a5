"""Host-side tests of the device-resident loss scaler (boundary B21): csrc/scaler_math.h compiled for the host (gcc -O2
-ffp-contract=off) against torch._amp_update_scale_ on CPU tensors and against the Python statements of FlatOptimizer.prepare_step, and
the Python logic of grad_scaler.FlatGradScaler / nerf_trainer.NeRFSDSTrainer that needs no device.  Everything here is exact equality."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32


def _hostlib():
    src = os.path.join(HERE, "hostmath", "scaler_math_host.c")
    out = os.path.join(HERE, "hostmath", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libscaler_math_host.so")
    hdr = os.path.join(ROOT, "dreamwaltz-g_amd", "csrc", "scaler_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src, "-lm"], check=True)
    L = ctypes.CDLL(so)
    L.host_scaler_sequence.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    L.host_adam_hyper_row.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_void_p]
    L.host_scaler_nonfinite.argtypes = [ctypes.c_float]
    return L


def _host_sequence(found, scale0, tracker0, growth, backoff, interval):
    found = np.asarray(found, np.int32)
    scales, trackers = np.zeros(len(found), f32), np.zeros(len(found), np.int32)
    _hostlib().host_scaler_sequence(len(found), found.ctypes.data_as(ctypes.c_void_p), scale0, tracker0, growth, backoff, interval,
                                    scales.ctypes.data_as(ctypes.c_void_p), trackers.ctypes.data_as(ctypes.c_void_p))
    return scales, trackers


def _torch_sequence(found, scale0, tracker0, growth, backoff, interval):
    scale, tracker = torch.tensor(scale0, dtype=torch.float32), torch.tensor(tracker0, dtype=torch.int32)
    scales, trackers = [], []
    for f in found:
        torch._amp_update_scale_(scale, tracker, torch.tensor(float(f)), growth, backoff, interval)
        scales.append(scale.item())
        trackers.append(tracker.item())
    return np.asarray(scales, f32), np.asarray(trackers, np.int32)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


SEQUENCES = [
    [0, 0, 0, 0, 0, 0, 0],                                  # growth at every interval
    [0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0],                   # tracker reset on backoff, in the middle of an interval too
    [1, 1, 1, 0, 0, 0, 0, 1],
    list(np.random.RandomState(21).randint(0, 2, 40)),
]


@pytest.mark.parametrize("interval", [1, 2, 3])
def test_scale_update_against_torch_amp_update_scale(interval):
    for found in SEQUENCES:
        for scale0, growth, backoff in ((65536.0, 2.0, 0.5), (1000.0, 1.7, 0.3), (3.0, 1.0 + 2.0 ** -20, 0.999)):
            got = _host_sequence(found, scale0, 0, growth, backoff, interval)
            want = _torch_sequence(found, scale0, 0, growth, backoff, interval)
            assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), (interval, found, scale0, got, want)


@pytest.mark.parametrize("interval", [1, 2, 3])
def test_a_scale_of_2_to_127_does_not_grow_to_inf(interval):
    found = [0] * 7
    got = _host_sequence(found, 2.0 ** 127, 0, 2.0, 0.5, interval)
    want = _torch_sequence(found, 2.0 ** 127, 0, 2.0, 0.5, interval)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] == f32(2.0 ** 127)).all() and 0 in got[1]            # the tracker still resets at the interval
    # FLT_MAX / 1.5: the product overflows by rounding, not by exponent alone
    got = _host_sequence(found, float(np.finfo(f32).max) / 1.5, 0, 1.5 + 2.0 ** -20, 0.5, interval)
    want = _torch_sequence(found, float(np.finfo(f32).max) / 1.5, 0, 1.5 + 2.0 ** -20, 0.5, interval)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.isfinite(got[0]).all()


@pytest.mark.parametrize("interval", [1, 2, 3])
def test_repeated_backoff_runs_through_the_denormals_to_zero(interval):
    found = [1] * 170 + [0] * 4                            # 2^16 halved 166 times rounds to zero
    got = _host_sequence(found, 65536.0, 1, 2.0, 0.5, interval)
    want = _torch_sequence(found, 65536.0, 1, 2.0, 0.5, interval)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    tiny = float(np.finfo(f32).tiny)
    assert ((got[0] > 0) & (got[0] < tiny)).any() and got[0][169] == 0.0 and got[0][-1] == 0.0
    # factors that are no power of two: every backoff in the denormal range rounds (0.7 x the smallest denormal rounds back up to it,
    # 0.4 x rounds to zero)
    for backoff, last in ((0.7, 2.0 ** -149), (0.4, 0.0)):
        got = _host_sequence([1] * 400, 1.0, 0, 2.0, backoff, interval)
        want = _torch_sequence([1] * 400, 1.0, 0, 2.0, backoff, interval)
        assert _same_bits(got[0], want[0]) and got[0][-1] == f32(last)


def test_nonfinite_is_inf_and_nan_only():
    L = _hostlib()
    fmax = float(np.finfo(f32).max)
    for x in (0.0, -0.0, 1.0, fmax, -fmax, float(np.finfo(f32).tiny), 1e-45, -1e-45):
        assert L.host_scaler_nonfinite(x) == 0, x
    for x in (float("inf"), float("-inf"), float("nan")):
        assert L.host_scaler_nonfinite(x) == 1, x


def _python_row(lr, betas, t, grad_scale, scale):
    """The statements of FlatOptimizer.prepare_step, with the unscale as GradScaler forms it (a double reciprocal rounded once)."""
    b1, b2, lr = (struct.unpack("f", struct.pack("f", float(x)))[0] for x in (betas[0], betas[1], lr))
    return np.asarray([lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), float(f32(grad_scale)) / float(f32(scale)), 0.0], np.float64).astype(f32)


@pytest.mark.parametrize("betas", [(0.9, 0.99), (0.9, 0.999)])
def test_bias_correction_scalars_against_prepare_step(betas):
    L = _hostlib()
    for t in list(range(1, 51)) + [1000, 10000]:
        for lr, grad_scale, scale in ((1e-3, 1.0, 65536.0), (1e-2, 0.25, 3.0), (5e-4, 1.0, 1.0)):
            row = np.zeros(4, f32)
            L.host_adam_hyper_row(lr, betas[0], betas[1], t, grad_scale, scale, row.ctypes.data_as(ctypes.c_void_p))
            assert _same_bits(row, _python_row(lr, betas, t, grad_scale, scale)), (betas, t, lr, row)
    # and prepare_step itself writes those bits (grad_scale alone in the third float: no scaler there)
    from dreamwaltz_g_amd import optim
    p = torch.nn.Parameter(torch.zeros(8))
    o = optim.build_flat_optimizers({'a': optim.AdamSpec([{'params': [p], 'lr': 1e-3}], betas=betas, eps=1e-15)}, 'cpu')['a']
    table = torch.zeros(1, 4)
    for t in range(1, 6):
        o.prepare_step(table, 0)
        row = np.zeros(4, f32)
        L.host_adam_hyper_row(1e-3, betas[0], betas[1], t, 1.0, 1.0, row.ctypes.data_as(ctypes.c_void_p))
        assert _same_bits(table[0].numpy(), row), t


def test_state_dict_keys_and_round_trip_through_torchs_grad_scaler():
    from dreamwaltz_g_amd.grad_scaler import FlatGradScaler
    s = FlatGradScaler(init_scale=1024.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7, device='cpu')
    s._growth_tracker.fill_(5)
    sd = s.state_dict()
    assert sorted(sd) == sorted(["scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"])
    assert sd == {"scale": 1024.0, "growth_factor": 3.0, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 5}
    ts = torch.amp.GradScaler('cpu')
    ts.load_state_dict(sd)
    back = ts.state_dict()
    assert back == sd
    s2 = FlatGradScaler(device='cpu')
    assert s2.get_scale() == 65536.0 and s2._get_growth_tracker() == 0 and s2._enabled
    s2.load_state_dict(back)
    assert s2.state_dict() == sd
    assert s2._get_scale_async().dtype == torch.float32 and s2._get_scale_async().dim() == 0 and float(s2._get_scale_async()) == 1024.0
    # the members are views of one 16-byte block: {scale, growth_tracker, found_inf, reserved}
    assert s2._state.view(torch.float32)[0].item() == 1024.0 and s2._state[1].item() == 5 and s2._state[2].item() == 0
    # disabled: torch's empty dict, the loss passes through
    off = FlatGradScaler(enabled=False, device='cpu')
    loss = torch.ones(1)
    assert off.state_dict() == {} and off.scale(loss) is loss and not off._enabled and off.get_scale() == 1.0
    with pytest.raises(RuntimeError, match="empty"):
        s2.load_state_dict({})


def test_scale_multiplies_and_step_refuses_other_optimizers():
    from dreamwaltz_g_amd.grad_scaler import FlatGradScaler
    s = FlatGradScaler(init_scale=8.0, device='cpu')
    assert torch.equal(s.scale(torch.tensor([1.5])), torch.tensor([12.0]))
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(TypeError, match="FlatOptimizer"):
        s.step(torch.optim.Adam([p], lr=1e-3))
    with pytest.raises(TypeError, match="FlatOptimizer"):
        FlatGradScaler(enabled=False, device='cpu').step(object())
    with pytest.raises(NotImplementedError, match="unscale_"):
        s.unscale_(None)


def _trainer(fp16):
    from dreamwaltz_g_amd import configs, nerf_model, nerf_trainer
    cfg = configs.TrainConfig()
    cfg.stage = 'nerf'
    cfg.nerf = configs.NeRFConfig(bound=1.0, grid_size=16, num_levels=4, desired_resolution=128)
    cfg.prompt.text_augmentation = False
    cfg.optim.fp16 = fp16
    net = nerf_model.NeRFNetwork(cfg.nerf)
    opts, _ = net.get_optimizer(cfg.nerf)
    return nerf_trainer.NeRFSDSTrainer(cfg, net, lambda **kw: None, opts, use_controlnet=False)


def test_the_trainer_builds_a_scaler_under_fp16_only():
    from dreamwaltz_g_amd.grad_scaler import FlatGradScaler
    tr = _trainer(True)
    assert isinstance(tr.scaler, FlatGradScaler) and tr.scaler._enabled is True
    assert tr.scaler.state_dict() == torch.amp.GradScaler('cpu').state_dict()          # torch's defaults
    assert _trainer(False).scaler is None


def test_step_after_step_scaled_needs_a_sync():
    """The device step counts are authoritative after step_scaled: the host-counting step() refuses until state_dict() read them back."""
    from dreamwaltz_g_amd import optim
    p = torch.nn.Parameter(torch.zeros(8))
    o = optim.build_flat_optimizers({'a': optim.AdamSpec([{'params': [p], 'lr': 1e-3}])}, 'cpu')['a']
    o._dev_ahead = True                                    # what step_scaled leaves behind (it needs a device)
    with pytest.raises(RuntimeError, match="step_scaled"):
        o.step()
    with pytest.raises(RuntimeError, match="step_scaled"):
        o.prepare_step(torch.zeros(1, 4), 0)
