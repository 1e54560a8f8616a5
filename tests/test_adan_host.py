"""Host-side tests of the fused Adan (boundary B23): csrc/adan_math.h compiled for the host (gcc -O2 -ffp-contract=off, the statements the
kernels run) against tests/golden/adan.npz -- the reference's own Adan on the CPU --, the float64 restatement of tests/adan_cases.py
pinned to the same golden, the C-ABI's argument checks, and the Python logic of optim.FlatAdan that needs no device.

THE BOUND, after every step, for the parameters and each of the four states: max|err| / max|ref| against the float64 restatement at most
2 x (the fp32 torch statement composition's error against float64) + 1e-7."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import dwg_import  # noqa: F401
from tests import adan_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
f32 = np.float32
GOLDEN = os.path.join(HERE, "golden", "adan.npz")
SIZES = [sum(int(np.prod(s)) for s in group) for group in ac.GOLDEN_SHAPES]            # elements per group: 40, 18


def _hostlib():
    src = os.path.join(HERE, "hostmath", "adan_math_host.c")
    out = os.path.join(HERE, "hostmath", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libadan_math_host.so")
    hdr = os.path.join(ROOT, "dreamwaltz-g_amd", "csrc", "adan_math.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src, "-lm"], check=True)
    L = ctypes.CDLL(so)
    vp, d, i32 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32
    L.host_adan_sumsq.restype = d
    L.host_adan_sumsq.argtypes = [ctypes.c_int64, vp]
    L.host_adan_clip.restype = d
    L.host_adan_clip.argtypes = [d, d, d, d]
    L.host_adan_hyper_row.argtypes = [d, d, d, d, d, d, ctypes.c_int, i32, ctypes.c_int, d, d, vp]
    L.host_adan_update.argtypes = [ctypes.c_int64] + [vp] * 7
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_chain(params, grads, hyper, max_grad_norm, grad_scale=1.0):
    """The optimizer as the device runs it (dwg_adan_sumsq / dwg_adan_prepare / dwg_adan_step_groups_dev), on the host build of
    adan_math.h: -> per step {'p': [G], state: [G]} fp32 arrays."""
    L = _hostlib()
    R = L.host_adan_row_floats()
    p = [np.array(x, f32) for x in params]
    st = {k: [np.zeros_like(x) for x in p] for k in ac.STATES}
    out = []
    for k, step in enumerate(grads):
        gs = [np.ascontiguousarray(x, f32) for x in step]
        clip = 1.0
        if max_grad_norm > 0:
            total = 0.0
            for g in gs:
                total += L.host_adan_sumsq(g.size, _p(g))
            clip = L.host_adan_clip(total, max_grad_norm, grad_scale, hyper[-1]['eps'])
        for i, h in enumerate(hyper):
            row = np.zeros(R, f32)
            L.host_adan_hyper_row(h['lr'], h['betas'][0], h['betas'][1], h['betas'][2], h['eps'], h['weight_decay'], int(h['no_prox']), k + 1,
                                  int(k == 0), clip, grad_scale, _p(row))
            L.host_adan_update(p[i].size, _p(row), _p(gs[i]), _p(p[i]), _p(st['exp_avg'][i]), _p(st['exp_avg_sq'][i]), _p(st['exp_avg_diff'][i]),
                               _p(st['neg_pre_grad'][i]))
        rec = {'p': [x.copy() for x in p]}
        rec.update({key: [x.copy() for x in st[key]] for key in ac.STATES})
        out.append(rec)
    return out


_CACHE = {}


def _case(variant):
    """(golden arrays, inputs, the float64 chain, the fp32 composition) of one variant, computed once."""
    if variant not in _CACHE:
        wd, no_prox, mgn = variant
        d = np.load(GOLDEN)
        off = np.cumsum([0] + SIZES)
        p0 = [d["p0"][off[g]:off[g + 1]] for g in range(len(SIZES))]
        grads = [[d["grads"][k][off[g]:off[g + 1]] for g in range(len(SIZES))] for k in range(ac.K)]
        hyper = ac.hypers(ac.GOLDEN_LRS, wd, no_prox)
        tag = ac.variant_tag(wd, no_prox, mgn)
        gold = {key: d["%s_%s" % (tag, key)] for key in ("p", "step") + ac.STATES}
        _CACHE[variant] = (gold, p0, grads, hyper, ac.chain(p0, grads, hyper, mgn, torch.float64), ac.chain(p0, grads, hyper, mgn, torch.float32), off)
    return _CACHE[variant]


def test_golden_inputs_are_the_cases_and_cover_the_three_kinds_of_step():
    d = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 << 10
    assert np.array_equal(d["p0"], np.concatenate([ac.flat(g) for g in ac.make_params(ac.GOLDEN_SHAPES)]))
    grads = ac.make_grads(ac.GOLDEN_SHAPES)
    assert np.array_equal(d["grads"], np.stack([np.concatenate([ac.flat(g) for g in s]) for s in grads]))
    norms = [ac.global_norm(s) for s in grads]
    assert sum(n > ac.MAX_GRAD_NORM for n in norms) >= 2 and sum(0 < n < ac.MAX_GRAD_NORM for n in norms) >= 2 and norms.count(0.0) == 1
    assert len(ac.VARIANTS) == 8


@pytest.mark.parametrize("variant", ac.VARIANTS, ids=lambda v: ac.variant_tag(*v))
def test_float64_restatement_is_pinned_to_the_golden(variant):
    gold, p0, grads, hyper, r64, r32, off = _case(variant)
    for k in range(ac.K):
        assert list(gold["step"][k]) == [k + 1] * len(SIZES)
        for key in ("p",) + ac.STATES:
            for g in range(len(SIZES)):
                want, comp = r64[k][key][g], r32[k][key][g]
                e = ac.rel_max(gold[key][k][off[g]:off[g + 1]], want)
                assert e <= ac.bound(comp, want), (k, key, g, e, ac.bound(comp, want))
    # the clipping is what the variants say: with max_grad_norm 5 the first step's gradient (norm 12) is scaled by 5 / 12
    if variant[2] > 0:
        assert ac.rel_max(-gold["neg_pre_grad"][0], np.concatenate(grads[0]) * (5.0 / 12.0)) < 1e-6
    else:
        assert np.array_equal(-gold["neg_pre_grad"][0], np.concatenate(grads[0]))


@pytest.mark.parametrize("variant", ac.VARIANTS, ids=lambda v: ac.variant_tag(*v))
def test_adan_math_h_against_the_golden_and_float64(variant):
    gold, p0, grads, hyper, r64, r32, off = _case(variant)
    got = host_chain(p0, grads, hyper, variant[2])
    worst = 0.0
    for k in range(ac.K):
        for key in ("p",) + ac.STATES:
            for g in range(len(SIZES)):
                want, comp = r64[k][key][g], r32[k][key][g]
                b = ac.bound(comp, want)
                e = ac.rel_max(got[k][key][g], want)
                worst = max(worst, e / b)
                assert e <= b, (k, key, g, e, b)
                # and against the reference's own result, at the same bound
                eg = ac.rel_max(got[k][key][g], gold[key][k][off[g]:off[g + 1]])
                assert eg <= b, (k, key, g, eg, b)
    print("adan_math.h %s: worst error / bound %.3f" % (ac.variant_tag(*variant), worst))
    # the first update's difference is exactly zero, and neg_pre_grad holds MINUS the clipped gradient
    assert all(not x.any() for x in got[0]["exp_avg_diff"])
    if variant[2] == 0:
        assert all(np.array_equal(-a, b) for a, b in zip(got[0]["neg_pre_grad"], grads[0]))


def test_scalars_are_formed_in_double_and_rounded_once():
    L = _hostlib()
    row = np.zeros(L.host_adan_row_floats(), f32)
    b1, b2, b3 = ac.BETAS
    for t in (1, 2, 7, 1000):
        for lr, wd, no_prox in ((1e-3, 2e-5, 0), (3e-3, 0.0, 1), (1e-3, 2e-5, 1)):
            L.host_adan_hyper_row(lr, b1, b2, b3, 1e-8, wd, no_prox, t, int(t == 1), 0.25, 0.5, _p(row))
            want = [0.125, lr / (1 - b1 ** t), lr * b2 / (1 - b2 ** t), (1 - b3 ** t) ** 0.5, (1 - lr * wd) if no_prox else (1 + lr * wd),
                    float(t == 1), b1, 1 - b1, b2, 1 - b2, b3, 1 - b3, 1e-8, float(no_prox), 0.0, 0.0]
            assert np.array_equal(row, np.asarray(want, np.float64).astype(f32)), (t, row, want)
    assert L.host_adan_clip(144.0, 5.0, 1.0, 1e-8) == 5.0 / (12.0 + 1e-8)
    assert L.host_adan_clip(144.0, 5.0, 0.5, 1e-8) == 5.0 / (6.0 + 1e-8)                # the norm of the SCALED gradient
    assert L.host_adan_clip(1.0, 5.0, 1.0, 1e-8) == 1.0 and L.host_adan_clip(0.0, 5.0, 1.0, 1e-8) == 1.0
    assert L.host_adan_clip(1e30, 0.0, 1.0, 1e-8) == 1.0                                 # max_grad_norm 0: no clipping


def test_cabi_argument_errors_before_any_launch():
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert L.dwg_adan_sumsq_slots(0) == 0 and L.dwg_adan_sumsq_slots(1) == 1 and L.dwg_adan_sumsq_slots(499) == 1
    assert L.dwg_adan_sumsq_slots(70001) == 69 and L.dwg_adan_sumsq_slots(1 << 20) == 1024 and L.dwg_adan_sumsq_slots(1 << 30) == 1024
    assert _lib.CONSTANTS["DWG_ADAN_MAX_SLOTS"] == 1024 and _lib.CONSTANTS["DWG_ADAN_ROW"] == 16
    for args in ((0, fake, fake), (-1, fake, fake), (8, None, fake), (8, fake, None), (8, odd, fake), (8, fake, odd)):
        assert L.dwg_adan_sumsq(*args, None) != 0, args
    H = _lib.STRUCTS["dwg_adan_hyper"]
    good = (H * 2)()
    for h in good:
        h.lr, h.beta1, h.beta2, h.beta3, h.eps, h.weight_decay = 1e-3, 0.98, 0.92, 0.99, 1e-8, 0.0
    bad = (H * 2)()
    bad[0].lr, bad[0].beta1, bad[0].beta2, bad[0].beta3, bad[0].eps = 1e-3, 1.0, 0.92, 0.99, 1e-8        # beta1 = 1
    prep = L.dwg_adan_prepare
    for args in ((1, None, 2, good, 0, 5.0, 1.0, fake, fake), (1, odd, 2, good, 0, 5.0, 1.0, fake, fake), (2000, fake, 2, good, 0, 5.0, 1.0, fake, fake),
                 (1, fake, 0, good, 0, 5.0, 1.0, fake, fake), (1, fake, 17, good, 0, 5.0, 1.0, fake, fake), (1, fake, 2, None, 0, 5.0, 1.0, fake, fake),
                 (1, fake, 2, good, 4, 5.0, 1.0, fake, fake), (1, fake, 2, good, 0, -1.0, 1.0, fake, fake), (0, None, 2, good, 0, 5.0, 1.0, fake, fake),
                 (1, fake, 2, good, 0, 0.0, 1.0, fake, fake), (1, fake, 2, good, 0, 5.0, 1.0, None, fake), (1, fake, 2, good, 0, 5.0, 1.0, fake, None),
                 (1, fake, 2, good, 0, 5.0, 1.0, fake, odd), (1, fake, 2, bad, 0, 5.0, 1.0, fake, fake)):
        assert prep(*args, None) != 0, args
    Gc = _lib.STRUCTS["dwg_adan_group"]

    def group(n=8, row=0, **ptrs):
        g = Gc()
        for k in ("param", "grad", "exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad"):
            setattr(g, k, ptrs.get(k, 4096))
        g.n, g.hyper_row = n, row
        return g
    step = L.dwg_adan_step_groups_dev
    assert step(0, None, fake, None) == 0                                              # nothing to do
    assert step(1, (Gc * 1)(group(n=0)), fake, None) == 0                              # an empty group is skipped
    for count, groups, rows in ((1, None, fake), (-1, (Gc * 1)(group()), fake), (17, (Gc * 1)(group()), fake), (1, (Gc * 1)(group()), None),
                                (1, (Gc * 1)(group()), odd), (1, (Gc * 1)(group(n=-1)), fake), (1, (Gc * 1)(group(row=-1)), fake),
                                (1, (Gc * 1)(group(row=16)), fake), (1, (Gc * 1)(group(param=None)), fake), (1, (Gc * 1)(group(grad=4100)), fake),
                                (1, (Gc * 1)(group(neg_pre_grad=None)), fake), (1, (Gc * 1)(group(exp_avg_diff=4104)), fake)):
        assert step(count, groups, rows, None) != 0, (count, rows)


# --------------------------------------------------------------------------------------------------------------------------------------
# optim.FlatAdan: the logic that needs no device
# --------------------------------------------------------------------------------------------------------------------------------------
def _flat_adan():
    from dreamwaltz_g_amd import optim
    a = [torch.nn.Parameter(torch.arange(6, dtype=torch.float32).view(2, 3)), torch.nn.Parameter(torch.ones(5))]
    b = [torch.nn.Parameter(torch.full((3,), 2.0))]
    spec = optim.AdanSpec([{'params': a, 'lr': 1e-3}, {'params': b, 'lr': 3e-3, 'no_prox': True}], weight_decay=2e-5, max_grad_norm=5.0)
    return optim, optim.FlatAdan(spec, 'cpu'), a, b


def test_flat_adan_slices_views_and_groups():
    optim, o, a, b = _flat_adan()
    assert o.buf.slices == [(0, 6), (8, 5), (16, 3)] and o.buf.total == 20                # 16-byte aligned slices
    assert [(pg["start"], pg["end"]) for pg in o.param_groups] == [(0, 16), (16, 20)]
    for t in (o.buf.flat, o.buf.grad, o.exp_avg, o.exp_avg_sq, o.exp_avg_diff, o.neg_pre_grad):
        assert t.shape == (20,) and t.dtype == torch.float32
    assert torch.equal(o.buf.flat[:6], torch.arange(6.0)) and torch.equal(o.buf.flat[16:19], torch.full((3,), 2.0))
    assert a[0].data_ptr() == o.buf.flat.data_ptr() and a[1].grad.data_ptr() == o.buf.grad.data_ptr() + 32
    pg = o.param_groups
    assert (pg[0]["lr"], pg[1]["lr"], pg[0]["no_prox"], pg[1]["no_prox"]) == (1e-3, 3e-3, False, True)
    assert all(g["betas"] == (0.98, 0.92, 0.99) and g["eps"] == 1e-8 and g["weight_decay"] == 2e-5 and g["max_grad_norm"] == 5.0 for g in pg)
    assert o.grad_scale == 1.0 and o.owns_buffers
    with pytest.raises(ValueError, match="beta"):
        optim.AdanSpec([{'params': []}], betas=(0.98, 1.0, 0.99))
    with pytest.raises(ValueError, match="grad norm"):
        optim.AdanSpec([{'params': []}], max_grad_norm=-1.0)


def test_flat_adan_participation_follows_the_backward():
    optim, o, a, b = _flat_adan()
    assert o.participating() == [0, 1]                                                  # no backward recorded anything: every group
    (a[1] * 2.0).sum().backward()
    assert o.buf.tracking and o.participating() == [0]
    assert torch.equal(o.buf.grad[8:13], torch.full((5,), 2.0)) and not o.buf.grad[:8].any()
    assert o.participating([False, True]) == [1]                                        # the caller's decision wins
    o.zero_grad()
    assert not o.buf.grad.any() and not o.buf.tracking and o.participating() == [0, 1]
    (b[0] * 3.0).sum().backward()
    assert o.participating() == [1]


def test_flat_adan_state_dict_round_trip_and_step_scaled_refusal():
    optim, o, a, b = _flat_adan()
    o.exp_avg.copy_(torch.arange(20.0)); o.exp_avg_sq.fill_(2.0); o.exp_avg_diff.fill_(-1.0); o.neg_pre_grad.copy_(-torch.arange(20.0))
    o._steps.copy_(torch.tensor([7, 7], dtype=torch.int32))
    o.param_groups[0]["has_prev"] = True
    o.param_groups[1]["lr"] = 5e-3
    sd = o.state_dict()
    assert sorted(sd) == sorted(["max_grad_norm", "param_groups", "exp_avg", "exp_avg_sq", "exp_avg_diff", "neg_pre_grad"])
    assert [g["step"] for g in sd["param_groups"]] == [7, 7] and all("params" not in g for g in sd["param_groups"])
    assert {"lr", "betas", "eps", "weight_decay", "no_prox", "step", "max_grad_norm"} <= set(sd["param_groups"][0])
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    _, o2, _, _ = _flat_adan()
    o2.load_state_dict(sd)
    assert o2.device_step_counts() == [7, 7] and o2.param_groups[1]["lr"] == 5e-3
    assert [g["has_prev"] for g in o2.param_groups] == [True, False]
    for key in ac.STATES:
        assert torch.equal(getattr(o2, key), getattr(o, key)), key
    back = o2.state_dict()
    assert back["param_groups"] == sd["param_groups"] and all(torch.equal(back[k], sd[k]) for k in ac.STATES)
    with pytest.raises(NotImplementedError, match="step_scaled"):
        o.step_scaled(None)
