"""GPU tests of the fused Adan (boundary B23, dreamwaltz_g_amd.optim.FlatAdan on csrc/adan.hip): six steps -- the clip active, inactive
and an all-zero gradient among them (tests/adan_cases.NORMS) -- against the float64 restatement of tests/adan_cases.py.

THE BOUND, after every step, for the parameters and each of the four states: max|err| / max|ref| at most 2 x (the fp32 torch statement
composition's error against float64) + 1e-7.  Two runs are bit-identical, and the three launches replayed from a captured graph give the
eager bits.

Sizes: 1; 3; the learned background's four tensors (499 parameters, one group); 70 001 in two groups (several slots of the scan, a tail
that is no multiple of four); 1 050 001 -- past DWG_ADAN_MAX_SLOTS x 1024 = 1 048 576 elements, where every workgroup of the scan strides
over the buffer."""
import numpy as np
import pytest
import torch

from tests import adan_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = {
    "n1": ([[(1,)]], [1e-3]),
    "n3": ([[(3,)]], [1e-3]),
    "background499": (ac.BACKGROUND_SHAPES, [1e-3]),
    "n70001": ([[(50000,)], [(20001,)]], [1e-3, 3e-3]),
    "n1050001": ([[(1050001,)]], [1e-3]),
}


def _build(shapes, lrs, wd, no_prox, mgn, p0):
    from dreamwaltz_g_amd import optim
    params = [[torch.nn.Parameter(torch.from_numpy(t.copy()).to(DEV)) for t in group] for group in p0]
    spec = optim.AdanSpec([{'params': group, 'lr': lr} for group, lr in zip(params, lrs)], betas=ac.BETAS, eps=ac.EPS, weight_decay=wd,
                          max_grad_norm=mgn, no_prox=no_prox)
    return optim.FlatAdan(spec, DEV), params


def _set_grads(params, step):
    for group, gg in zip(params, step):
        for p, t in zip(group, gg):
            p.grad.copy_(torch.from_numpy(t).to(DEV))


def _snapshot(o, params):
    """{'p': [G] 1-D tensors (the group's tensors, no padding), state: [G]} read through the parameters' slices of the flat buffers."""
    rec = {}
    for key, buf in (("p", o.buf.flat), ("exp_avg", o.exp_avg), ("exp_avg_sq", o.exp_avg_sq), ("exp_avg_diff", o.exp_avg_diff),
                     ("neg_pre_grad", o.neg_pre_grad)):
        rec[key], i = [], 0
        for group in params:
            parts = []
            for _ in group:
                off, n = o.buf.slices[i]
                parts.append(buf[off:off + n].clone())
                i += 1
            rec[key].append(torch.cat(parts))
    return rec


def _run(shapes, lrs, wd, no_prox, mgn, p0, grads):
    o, params = _build(shapes, lrs, wd, no_prox, mgn, p0)
    out = []
    for step in grads:
        o.zero_grad()
        _set_grads(params, step)
        o.step()
        out.append(_snapshot(o, params))
    return o, params, out


SETTINGS = {"reference": (2e-5, False, 5.0), "noprox": (2e-5, True, 5.0), "noclip": (0.0, False, 0.0)}
# every size under every setting, but the large one under the reference's only (the kernels take no other path for the settings)
RUNS = [(c, s) for c in CASES for s in SETTINGS if c != "n1050001" or s == "reference"]


@pytest.mark.parametrize("case,setting", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_six_steps_against_float64(case, setting):
    shapes, lrs = CASES[case]
    wd, no_prox, mgn = SETTINGS[setting]
    p0, grads = ac.make_params(shapes, seed=3), ac.make_grads(shapes, seed=4)
    norms = [ac.global_norm(s) for s in grads]
    assert sum(n > 5 for n in norms) >= 2 and sum(0 < n < 5 for n in norms) >= 2 and norms.count(0.0) == 1
    hyper = ac.hypers(lrs, wd, no_prox)
    fp, fg = [ac.flat(g) for g in p0], [[ac.flat(g) for g in s] for s in grads]
    r64, r32 = ac.chain(fp, fg, hyper, mgn, torch.float64), ac.chain(fp, fg, hyper, mgn, torch.float32)
    o, params, got = _run(shapes, lrs, wd, no_prox, mgn, p0, grads)
    worst = 0.0
    for k in range(ac.K):
        for key in ("p",) + ac.STATES:
            for g in range(len(shapes)):
                want, comp = r64[k][key][g], r32[k][key][g]
                e, b = ac.rel_max(got[k][key][g].cpu(), want), ac.bound(comp, want)
                worst = max(worst, e / b)
                assert e <= b, (case, k, key, g, e, b)
    print("FlatAdan %s wd=%g no_prox=%s clip=%g: worst error / bound %.3f" % (case, wd, no_prox, mgn, worst))
    assert o.device_step_counts() == [ac.K] * len(shapes)
    # the gradient buffer is left as it was written, and the padding between the slices stays zero
    assert torch.equal(params[0][0].grad.cpu(), torch.from_numpy(grads[-1][0][0]))
    used = torch.zeros(o.buf.total, dtype=torch.bool)
    for off, n in o.buf.slices:
        used[off:off + n] = True
    for buf in (o.buf.flat, o.exp_avg, o.exp_avg_sq, o.exp_avg_diff, o.neg_pre_grad):
        assert not buf.cpu()[~used].any()


@pytest.mark.parametrize("case", ["background499", "n70001"])
def test_two_runs_are_bit_identical_and_a_captured_step_equals_the_eager_one(case):
    shapes, lrs = CASES[case]
    p0, grads = ac.make_params(shapes, seed=3), ac.make_grads(shapes, seed=4)
    _, _, a = _run(shapes, lrs, 2e-5, False, 5.0, p0, grads)
    _, _, b = _run(shapes, lrs, 2e-5, False, 5.0, p0, grads)
    for k in range(ac.K):
        for key in a[k]:
            assert all(torch.equal(x, y) for x, y in zip(a[k][key], b[k][key])), (k, key)
    # the three launches captured once (sequential, no branches) and replayed for every later step: the step counts live on the device
    o, params = _build(shapes, lrs, 2e-5, False, 5.0, p0)
    o.zero_grad()
    _set_grads(params, grads[0])
    o.step()                                            # eager: the group's first update (the host flag of the capture is then "not first")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _set_grads(params, grads[1])
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            o.step()
    torch.cuda.current_stream().wait_stream(side)
    for k in range(1, ac.K):
        _set_grads(params, grads[k])
        graph.replay()
        got = _snapshot(o, params)
        for key in got:
            assert all(torch.equal(x, y) for x, y in zip(got[key], a[k][key])), (k, key)
    assert o.device_step_counts() == [ac.K] * len(shapes)


def test_a_group_that_took_no_part_ages_and_is_otherwise_untouched():
    shapes, lrs = CASES["n70001"]
    p0, grads = ac.make_params(shapes, seed=3), ac.make_grads(shapes, seed=4)
    o, params = _build(shapes, lrs, 2e-5, False, 5.0, p0)
    o.zero_grad()
    _set_grads(params, grads[0])
    before = _snapshot(o, params)
    o.step(participation=[True, False])
    after = _snapshot(o, params)
    assert o.device_step_counts() == [1, 1]
    for key in after:
        assert torch.equal(after[key][1], before[key][1]), key
    assert not torch.equal(after["p"][0], before["p"][0])
    assert [pg["has_prev"] for pg in o.param_groups] == [True, False]
    # its first update comes at step 2: the difference is zero there, as for a parameter whose state the reference creates late
    o.zero_grad()
    _set_grads(params, grads[1])
    o.step()
    assert not o.exp_avg_diff[o.param_groups[1]["start"]:o.param_groups[1]["end"]].any()
    assert o.exp_avg_diff[:o.param_groups[0]["end"]].any()
    from dreamwaltz_g_amd import optim
    epoch = optim.PARAM_EPOCH[0]
    o.step()
    assert optim.PARAM_EPOCH[0] == epoch + 1
