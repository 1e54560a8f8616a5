"""GPU tests of the device-resident loss scaler (boundary B21, csrc/grad_scaler.hip; the scaled fused Adam is csrc/adam.hip's): the Inf / NaN scan, the scaled fused Adam against
torch.optim.Adam + torch.amp.GradScaler('cuda'), participation, and the gradient hooks with a FlatGradScaler.

Bounds: the skip decision, scale and growth tracker are exact; parameters after a taken step rtol 2e-5 / atol 2e-6 (the project's Adam
bound, tests/test_nerf_step_gpu.py); the device-computed hyper rows within one fp32 ulp of the host statements (a device pow in double
need not match libm's last bit)."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda"
SLOTS = 2048                            # DWG_SCALER_MAX_SLOTS: the scan's grid cap
PASS = SLOTS * 256 * 4                  # floats one grid-stride pass covers
BIG = 2 * PASS + 5                      # more than one pass of the capped grid, plus a tail
LENGTHS = (1, 3, 4, 1021, BIG)


def _scan(buf, n, slots):
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.dwg_grads_nonfinite(n, _lib.ptr(buf), _lib.ptr(slots), st), "dwg_grads_nonfinite")
    return L.dwg_grads_nonfinite_slots(n)


def _slot_of(idx, n, nslots):
    """The workgroup that reads element idx: float4 k = idx / 4 goes to workgroup (k mod (nslots * 256)) / 256; the n % 4 tail to workgroup 0."""
    if idx >= n // 4 * 4:
        return 0
    return (idx // 4) % (nslots * 256) // 256


@pytest.fixture(scope="module")
def finite_buffer():
    """BIG floats of finite values with the extremes in them: FLT_MAX, -FLT_MAX, denormals, zeros."""
    g = torch.Generator().manual_seed(3)
    buf = torch.randn(BIG, generator=g)
    fmax = float(np.finfo(f32).max)
    special = torch.tensor([fmax, -fmax, 1e-45, -1e-45, float(np.finfo(f32).tiny) / 2, 0.0, -0.0, 2.0 ** -149])
    buf[:8] = special
    buf[PASS + 13:PASS + 21] = special
    buf[-8:] = special
    return buf.to(DEV)


def test_the_scan_reports_nothing_on_finite_values(finite_buffer):
    slots = torch.full((SLOTS,), 7, dtype=torch.int32, device=DEV)            # garbage: every slot in use is written, 0 or 1
    for n in LENGTHS:
        slots.fill_(7)
        k = _scan(finite_buffer, n, slots)
        assert k == max(1, min(SLOTS, (n // 4 + 255) // 256))
        assert int(slots[:k].abs().sum()) == 0, n
        assert k == SLOTS or int((slots[k:] != 7).sum()) == 0                 # and nothing beyond them
    special = finite_buffer[:8].clone()
    assert _scan(special, 8, slots) == 1 and int(slots[0]) == 0


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_the_scan_finds_a_single_nonfinite_value(finite_buffer, bad):
    slots = torch.zeros(SLOTS, dtype=torch.int32, device=DEV)
    for n in LENGTHS:
        places = {0, n - 1}                                                   # n - 1 lies in the scalar tail unless n % 4 == 0
        if n == BIG:
            places.add(PASS + PASS // 2 + 2)                                  # the middle of the second grid-stride pass
        for idx in sorted(places):
            keep = finite_buffer[idx].clone()
            finite_buffer[idx] = bad
            k = _scan(finite_buffer, n, slots)
            first = slots[:k].clone()
            _scan(finite_buffer, n, slots)                                    # again, nothing cleared in between: the same answer
            assert torch.equal(first, slots[:k])
            want = torch.zeros(k, dtype=torch.int32, device=DEV)
            want[_slot_of(idx, n, k)] = 1
            assert torch.equal(first, want), (n, idx, first.nonzero().flatten().tolist(), _slot_of(idx, n, k))
            finite_buffer[idx] = keep
            _scan(finite_buffer, n, slots)                                    # and no stale 1 once the value is gone
            assert int(slots[:k].sum()) == 0, (n, idx)


def test_the_scan_refuses_bad_arguments():
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    buf, slots = torch.zeros(16, device=DEV), torch.zeros(SLOTS, dtype=torch.int32, device=DEV)
    assert L.dwg_grads_nonfinite(0, _lib.ptr(buf), _lib.ptr(slots), None) != 0
    assert L.dwg_grads_nonfinite(8, None, _lib.ptr(slots), None) != 0 and L.dwg_grads_nonfinite(8, _lib.ptr(buf), None, None) != 0
    assert L.dwg_grads_nonfinite(8, ctypes.c_void_p(buf.data_ptr() + 4), _lib.ptr(slots), None) != 0       # not 16-byte aligned
    assert L.dwg_grads_nonfinite_slots(0) == 0 and L.dwg_grads_nonfinite_slots(1) == 1 and L.dwg_grads_nonfinite_slots(BIG) == SLOTS


# -- the scaled Adam ---------------------------------------------------------------------------------------------------------------------
GROUP_LENGTHS = (4, 1021, 70003)
LRS = (1e-2, 1e-3, 3e-3)
BETAS, EPS = (0.9, 0.99), 1e-15


def _flat_optimizer(seed=0):
    from dreamwaltz_g_amd import optim
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in GROUP_LENGTHS]
    spec = optim.AdamSpec([{'params': [p], 'lr': lr} for p, lr in zip(params, LRS)], betas=BETAS, eps=EPS)
    opts = optim.build_flat_optimizers({'a': spec}, DEV)
    return opts, opts['a'], params


def _host_row(lr, t, scale):
    b1, b2, lr = (struct.unpack("f", struct.pack("f", float(x)))[0] for x in (BETAS[0], BETAS[1], lr))
    return np.asarray([lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), 1.0 / float(f32(scale)), 0.0], np.float64).astype(f32)


def test_the_scaled_adam_against_torch_adam_under_torchs_grad_scaler():
    from dreamwaltz_g_amd.grad_scaler import FlatGradScaler
    opts, o, params = _flat_optimizer()
    buf = opts.buffers
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    topt = torch.optim.Adam([{'params': [r], 'lr': lr} for r, lr in zip(ref, LRS)], betas=BETAS, eps=EPS)
    ts = torch.amp.GradScaler('cuda', growth_interval=2)
    ts.scale(torch.zeros(1, device=DEV))                                     # torch creates its scale lazily
    fs = FlatGradScaler(growth_interval=2, device=DEV)
    g = torch.Generator().manual_seed(17)
    taken, differing, rows = 0, 0, 0
    for step in range(1, 7):
        scale = ts.get_scale()
        assert fs.get_scale() == scale
        grads = [(torch.randn(n, generator=g) * 0.1).to(DEV) * scale for n in GROUP_LENGTHS]
        if step == 3:
            grads[2][GROUP_LENGTHS[2] // 2] = float("inf")
        for p, r, gr in zip(params, ref, grads):
            p.grad.copy_(gr)
            r.grad = gr.clone()
        before = [t.clone() for t in (buf.flat, buf.m, buf.v)]
        steps_before = o.device_step_counts()
        ref_before = [r.detach().clone() for r in ref]
        fs.step(o)
        found = bool(o._dev["found"].item())
        assert float(fs._found_inf) == float(found) and fs.get_scale() == scale          # the old scale until update()
        hyper = o._dev["hyper"].cpu().numpy().copy()
        fs.update()
        ts.step(topt)
        ts.update()
        skipped = all(torch.equal(r.detach(), rb) for r, rb in zip(ref, ref_before))
        assert found == skipped == (step == 3), (step, found, skipped)
        assert fs.get_scale() == ts.get_scale() and fs._get_growth_tracker() == ts._get_growth_tracker(), step
        assert float(fs._found_inf) == 0.0
        if found:
            assert all(torch.equal(a, b) for a, b in zip(before, (buf.flat, buf.m, buf.v)))
            assert o.device_step_counts() == steps_before
            assert (hyper[:3, 3] != 0).all()
            continue
        taken += 1
        assert o.device_step_counts() == [taken] * 3
        for p, r in zip(params, ref):
            assert torch.allclose(p.detach(), r.detach(), rtol=2e-5, atol=2e-6), (step, float((p.detach() - r.detach()).abs().max()))
        for k, lr in enumerate(LRS):
            want = _host_row(lr, taken, scale)
            ulp = np.abs(hyper[k].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            assert ulp.max() <= 1, (step, k, hyper[k], want)
            differing += int((ulp != 0).sum())
            rows += 1
    print("scaled Adam: %d of %d device-computed hyper floats differ from the host statements (each by one ulp)" % (differing, 4 * rows))
    assert taken == 5 and o.t == 6 and fs.get_scale() == ts.get_scale()
    # the gradient stays scaled in the flat buffer, and the host's counts follow at state_dict()
    assert torch.equal(params[0].grad, grads[0])
    assert [pg["t"] for pg in o.state_dict()["param_groups"]] == [5, 5, 5]


def test_a_group_that_took_no_part_keeps_its_parameters_moments_and_step_count():
    from dreamwaltz_g_amd.grad_scaler import FlatGradScaler
    opts, o, params = _flat_optimizer(seed=1)
    buf = opts.buffers
    fs = FlatGradScaler(init_scale=4.0, device=DEV)
    for first in (True, False):
        o.zero_grad()
        for k, p in enumerate(params):
            if k != 1 or first:                                                 # the second round leaves group 1 out of the "backward"
                p.grad.add_(torch.full_like(p, 0.5 * 4.0))
                buf.touch(p)
        sl = slice(o.param_groups[1]["start"], o.param_groups[1]["end"])
        before = [t[sl].clone() for t in (buf.flat, buf.m, buf.v)]
        others = buf.flat.clone()
        fs.step(o)
        fs.update()
        if first:
            assert o.device_step_counts() == [1, 1, 1] and not torch.equal(before[0], buf.flat[sl])
        else:
            assert o.device_step_counts() == [2, 1, 2]
            assert all(torch.equal(a, b[sl]) for a, b in zip(before, (buf.flat, buf.m, buf.v)))
            assert not torch.equal(others[:4], buf.flat[:4])
    # an explicit participation list decides instead of the record, as in step()
    o.zero_grad()
    fs.step(o, participation=[False, True, False])
    assert o.device_step_counts() == [2, 2, 2]
    # the host-counting step() refuses until the counts are synced, then carries on from them
    with pytest.raises(RuntimeError, match="step_scaled"):
        o.step()
    assert [pg["t"] for pg in o.state_dict()["param_groups"]] == [2, 2, 2]
    o.step()
    assert [pg["t"] for pg in o.param_groups] == [3, 3, 3]
    fs.step(o)                                                                  # and the device is re-seeded from the host's counts
    assert o.device_step_counts() == [4, 4, 4]


def test_gradient_hooks_with_a_flat_scaler_as_with_torchs():
    from dreamwaltz_g_amd import pgc
    from dreamwaltz_g_amd.grad_scaler import FlatGradScaler
    fs = FlatGradScaler(init_scale=512.0, device=DEV)
    ts = torch.amp.GradScaler('cuda', init_scale=512.0)
    ts.scale(torch.zeros(1, device=DEV))
    grad = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(5)).to(DEV)
    mask = (torch.rand(2, 1, 16, 16, generator=torch.Generator().manual_seed(6)) > 0.3).float().to(DEV)
    for kw in (dict(grad_clip=False, grad_norm=True, grad_clip_scale=1.0), dict(grad_clip=True, grad_norm=True, grad_clip_scale=2.0, mask=mask)):
        a = pgc.build_grad_hook_func(scaler=fs, **kw)(grad.clone())
        b = pgc.build_grad_hook_func(scaler=ts, **kw)(grad.clone())
        assert torch.equal(a, b) and float(a.abs().max()) > 1.0
    # build_pgc_hook_func has no reference behaviour to mirror: the same refusal with either scaler
    for s in (fs, ts):
        with pytest.raises(NotImplementedError, match="UnboundLocalError"):
            pgc.build_pgc_hook_func(0.5, 0, s)
