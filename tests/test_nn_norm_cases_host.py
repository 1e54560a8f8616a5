"""Proves the checker of nn_norm_cases.py on the CPU, without a GPU: the formulas of csrc/nn_norm.hip emulated in torch float32 and rounded
to each element type

  * meet the per-element bound on every shape of the GPU tables (smaller batch where that keeps the run short) and on both offset cases --
    the bound is reachable by a correct fp32 implementation (the worst err / bound per op and element type is printed; the 16-bit types sit
    near 1 by construction: a half-ulp store IS the bound), and
  * miss it, in every element type, bf16 included, as soon as one of eight subtle faults is seeded -- where the max-norm measure of
    test_nn_gpu.py is blind.

The emulations follow the kernels' formulas (one-pass variance E[x^2] - m^2, rsqrt(max(var, 0) + eps), z / (1 + exp(-z)), the two-step
residual add, two-pass LayerNorm, the Abramowitz-Stegun erf of dwg_common.h), not their summation order."""
import math

import pytest
import torch

from tests import nn_norm_cases as nc

DT = pytest.mark.parametrize("dt", nc.DTYPES, ids=nc.DT_IDS)


def _small_batch(shape):
    B, HW, C, G = shape
    return (min(B, 2) if HW < 1024 else 1, HW, C, G)


# ------------------------------------------------------------------------------------------------------------------ fp32 emulations
def _silu(z):
    return z / (1 + torch.exp(-z))


def _silu_grad(z):
    s = 1 / (1 + torch.exp(-z))
    return s * (1 + z * (1 - s))


def emu_gn_stats(x, G, fault=None):
    B, HW, C = x.shape
    xs = torch.roll(x, -1, 2) if fault == "groupshift" else x          # group g = channels g cg + 1 .. (g + 1) cg
    if fault == "lastpix":
        xs = xs[:, :-1]
    xg = xs.reshape(B, xs.shape[1], G, C // G)
    return torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1)     # fp32 [B, G, 2]


def _mean_rstd(stats, n, eps, C, G):
    inv_n = torch.tensor(1.0 / n, dtype=torch.float32)
    m = stats[..., 0] * inv_n
    var = stats[..., 1] * inv_n - m * m
    rs = torch.rsqrt(var.clamp_min(0) + eps)
    ex = lambda t: t.repeat_interleave(C // G, 1)[:, None, :]          # noqa: E731  [B, G] -> [B, 1, C]
    return ex(m), ex(rs)


def emu_gn_forward(d, shape, dt, eps, silu, form, fault=None):
    """-> (y float64 as stored in `dt`, stats fp32).  form 'apply': ((x - m) rs) gamma + beta (k_gn_apply); 'small': x sc + sh with
    sc = gamma rs, sh = beta - m sc (k_gn_small)."""
    B, HW, C, G = shape
    x = d["x"].float()
    gamma, beta = d["gamma"].clone(), d["beta"]
    if fault == "gamma1":
        gamma[int((gamma - 1).abs().argmax())] = 1.0
    stats = emu_gn_stats(x, G, fault)
    m, rs = _mean_rstd(stats, HW * (C // G), 0.0 if fault == "noeps" else eps, C, G)
    if form == "apply":
        z = (x - m) * rs * gamma + beta
    else:
        sc = gamma * rs
        z = x * sc + (beta - m * sc)
    if silu:
        z = _silu(z)
    return nc.round64(z, dt), stats


def emu_gn_backward(d, shape, dt, eps, silu, stats, with_res, fault=None):
    B, HW, C, G = shape
    x, dy, gamma, beta = d["x"].float(), d["dy"].float(), d["gamma"], d["beta"]
    n = HW * (C // G)
    m, rs = _mean_rstd(stats, n, eps, C, G)
    xh = (x - m) * rs
    g = dy.clone()
    if silu:
        g = g * _silu_grad(xh * gamma + beta)
    g = g * gamma
    inv_n = torch.tensor(1.0 / n, dtype=torch.float32)
    ex = lambda t: t.repeat_interleave(C // G, 1)[:, None, :]          # noqa: E731
    gg = g.view(B, HW, G, C // G)
    m1 = ex(gg.sum((1, 3)) * inv_n)
    m2 = ex((gg * xh.view(B, HW, G, C // G)).sum((1, 3)) * inv_n)
    if fault == "nom2":
        m2 = torch.zeros_like(m2)
    out = nc.round64(rs * (g - m1 - xh * m2), dt)
    if with_res:
        res = d["res"].float()
        if fault == "resrow":
            res = torch.roll(res, 1, 1)
        out = nc.round64(out.float() + res, dt)                        # the kernel's second store
    return out


def emu_layernorm(x, gamma, beta, eps, dt, fault=None):
    x = x.float()
    C = x.shape[-1]
    dlt = x - x.sum(-1, keepdim=True) / C
    rstd = torch.rsqrt((dlt * dlt).sum(-1, keepdim=True) / C + (0.0 if fault == "noeps" else eps))
    return nc.round64(dlt * rstd * gamma + beta, dt)


def _erf_as(x):
    """dwg_erf_fast: Abramowitz-Stegun 7.1.26 in fp32."""
    ax = x.abs()
    t = 1 / (0.3275911 * ax + 1)
    p = 1.061405429 * t - 1.453152027
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + c
    return torch.copysign(1 - p * t * torch.exp(-ax * ax), x)


def emu_geglu(h, dt, fault=None):
    a, g = h.float().chunk(2, dim=-1)
    if fault == "tanh":
        gelu = 0.5 * g * (1 + torch.tanh(math.sqrt(2 / math.pi) * (g + 0.044715 * g ** 3)))
    else:
        gelu = 0.5 * g * (1 + _erf_as(g * 0.70710678118654752))
    return nc.round64(a * gelu, dt)


def emu_softmax(S, scale, dt, fault=None):
    z = S.float() * scale
    e = torch.exp(z - z.max(-1, keepdim=True).values)
    tot = (e[:, :-1] if fault == "nlast" else e).sum(-1, keepdim=True)
    return nc.round64(e * (1 / tot), dt)


def emu_softmax_bwd(P, dP, scale, dt):
    P, dP = P.float(), dP.float()
    return nc.round64(scale * P * (dP - (P * dP).sum(-1, keepdim=True)), dt)


# ------------------------------------------------------------------------------------------------------------------ cases
def _gn_fwd_case(shape, dt, eps, silu, kind="plain", fault=None):
    """-> ([(form, out)], ref y, ref stats, sum|x|, emulated stats, inputs, autograd leaf)"""
    d = nc.gn_inputs(shape, dt, kind)
    ref, leaf = nc.gn_ref(d["x"], d["gamma"], d["beta"], shape[3], eps, silu)
    outs = []
    for form in ("apply", "small"):
        y, st = emu_gn_forward(d, shape, dt, eps, silu, form, fault)
        outs.append((form, y))
    rs, ra = nc.gn_stats_ref(d["x"], shape[3])
    return outs, ref.detach(), rs, ra, st, d, (ref, leaf)


def _bwd_store(gx, res, dt):
    """The store term of the backward: one store without a residual, two with (nn_norm_cases docstring)."""
    return None if res is None else nc.store_term(gx, dt) + nc.store_term(gx + res, dt)


@DT
def test_groupnorm_forward_emulation_meets_the_bound(dt):
    worst = worst_st = 0.0
    for shape, _ in nc.GN_FWD:
        sh = _small_batch(shape)
        for silu in (0, 1):
            outs, ref, rs, ra, st, _, _ = _gn_fwd_case(sh, dt, nc.GN_EPS[shape], silu)
            for form, y in outs:
                worst = max(worst, nc.check(y, ref, dt, "gn fwd %s %s silu=%d" % (form, sh, silu)))
            worst_st = max(worst_st, nc.check_stats(st, rs, ra, "gn stats %s" % (sh,)))
    print("groupnorm forward  %-4s worst err/bound %.3f, statistics %.4f" % (nc.DT_NAME[dt], worst, worst_st))


@DT
def test_groupnorm_backward_emulation_meets_the_bound(dt):
    worst = 0.0
    for shape, _ in nc.GN_BWD:
        sh = _small_batch(shape)
        for silu in (0, 1):
            _, _, _, _, st, d, (ref, leaf) = _gn_fwd_case(sh, dt, nc.GN_EPS[shape], silu)
            gx = nc.gn_bwd_ref(ref, leaf, d["dy"])
            for with_res in (False, True):
                out = emu_gn_backward(d, sh, dt, nc.GN_EPS[shape], silu, st, with_res)
                want = gx + d["res"] if with_res else gx
                worst = max(worst, nc.check(out, want, dt, "gn bwd %s silu=%d res=%d" % (sh, silu, with_res),
                                            _bwd_store(gx, d["res"] if with_res else None, dt)))
    print("groupnorm backward %-4s worst err/bound %.3f" % (nc.DT_NAME[dt], worst))


@DT
def test_offset_and_low_variance_cases_meet_the_bound(dt):
    """mean = 4 sigma forward and 2 sigma backward at (1, 100, 512, 32): the one-pass variance loses m^2 / var of its digits and still
    leaves room in the bound (f32: 0.15 of it with exactly rounded sums, 0.6 forward / 0.16 backward with the fp32 sums of this emulation,
    whose own error of 4e-7 the m^2 / var = 16 then multiplies); the low-variance case is the one where eps carries weight."""
    sh = nc.GN_OFFSET_SHAPE
    w = {}
    for silu in (0, 1):
        outs, ref, rs, ra, st, _, _ = _gn_fwd_case(sh, dt, 1e-5, silu, "fwd4s")
        for form, y in outs:
            w["fwd 4 sigma"] = max(w.get("fwd 4 sigma", 0), nc.check(y, ref, dt, "gn fwd 4 sigma " + form))
        nc.check_stats(st, rs, ra, "gn stats 4 sigma")
        _, _, _, _, st, d, (ref, leaf) = _gn_fwd_case(sh, dt, 1e-5, silu, "bwd2s")
        gx = nc.gn_bwd_ref(ref, leaf, d["dy"])
        for with_res in (False, True):
            out = emu_gn_backward(d, sh, dt, 1e-5, silu, st, with_res)
            r = nc.check(out, gx + d["res"] if with_res else gx, dt, "gn bwd 2 sigma", _bwd_store(gx, d["res"] if with_res else None, dt))
            w["bwd 2 sigma"] = max(w.get("bwd 2 sigma", 0), r)
        outs, ref, rs, ra, st, _, _ = _gn_fwd_case(nc.GN_LOWVAR_SHAPE, dt, 1e-5, silu, "lowvar")
        for form, y in outs:
            w["low variance"] = max(w.get("low variance", 0), nc.check(y, ref, dt, "gn fwd low variance " + form))
        nc.check_stats(st, rs, ra, "gn stats low variance")
    print("groupnorm offsets  %-4s worst err/bound %s" % (nc.DT_NAME[dt], {k: round(v, 3) for k, v in w.items()}))


@DT
def test_layernorm_geglu_softmax_emulations_meet_the_bound(dt):
    w = dict(layernorm=0.0, geglu=0.0, softmax=0.0, softmax_bwd=0.0)
    for M, C in nc.LN_SHAPES:
        x, gamma, beta = nc.ln_draw(M, C)
        _, xr = nc.rounded(x, dt)
        w["layernorm"] = max(w["layernorm"], nc.check(emu_layernorm(xr, gamma, beta, 1e-5, dt), nc.ln_ref(xr, gamma, beta, 1e-5), dt,
                                                      "layernorm %s" % ((M, C),)))
    for M, Fd in nc.GEGLU_SHAPES:
        _, hr = nc.rounded(nc.geglu_draw(min(M, 37), Fd), dt)
        w["geglu"] = max(w["geglu"], nc.check(emu_geglu(hr, dt), nc.geglu_ref(hr), dt, "geglu %s" % ((M, Fd),)))
    for rows, dom in nc.SOFTMAX_CASES:
        for n in nc.SOFTMAX_N:
            S, dP = nc.softmax_draw(rows, n, dom)
            P = emu_softmax(S, nc.SOFTMAX_SCALE, dt)
            w["softmax"] = max(w["softmax"], nc.check(P, nc.softmax_ref(S, nc.SOFTMAX_SCALE), dt, "softmax %s" % ((rows, n),)))
            dS = emu_softmax_bwd(P, dP, nc.SOFTMAX_SCALE, dt)
            w["softmax_bwd"] = max(w["softmax_bwd"], nc.check(dS, nc.softmax_bwd_ref(P, dP, nc.SOFTMAX_SCALE), dt,
                                                              "softmax bwd %s" % ((rows, n),)))
            if n == 1:
                assert float(dS.abs().max()) == 0.0                       # ref == 0, bound == 0: met as 0 <= 0
    print("row ops            %-4s worst err/bound %s" % (nc.DT_NAME[dt], {k: round(v, 3) for k, v in w.items()}))


# ------------------------------------------------------------------------------------------------------------------ seeded faults
@DT
def test_seeded_faults_are_rejected(dt):
    """Each fault on a small-kernel shape and on a three-launch shape (smaller batch), with and without SiLU."""
    for shape in ((1, 64, 320, 32), (2, 100, 512, 32)):
        for silu in (0, 1):
            for fault in ("lastpix", "groupshift", "gamma1"):
                outs, ref, *_ = _gn_fwd_case(shape, dt, 1e-5, silu, fault=fault)
                for form, y in outs:
                    assert not nc.passes(y, ref, dt), (fault, form, shape, silu)
            _, _, _, _, st, d, (ref, leaf) = _gn_fwd_case(shape, dt, 1e-5, silu)
            gx = nc.gn_bwd_ref(ref, leaf, d["dy"])
            for fault, with_res in (("nom2", False), ("nom2", True), ("resrow", True)):
                out = emu_gn_backward(d, shape, dt, 1e-5, silu, st, with_res, fault)
                want = gx + d["res"] if with_res else gx
                assert not nc.passes(out, want, dt, _bwd_store(gx, d["res"] if with_res else None, dt)), (fault, shape, silu)
    # a dropped eps shows where the variance is of eps' size: the low-variance GroupNorm case and row 0 of every LayerNorm case
    for silu in (0, 1):
        outs, ref, *_ = _gn_fwd_case(nc.GN_LOWVAR_SHAPE, dt, 1e-5, silu, "lowvar", fault="noeps")
        for form, y in outs:
            assert not nc.passes(y, ref, dt), ("noeps", form, silu)
    for M, C in nc.LN_SHAPES:
        x, gamma, beta = nc.ln_draw(M, C)
        _, xr = nc.rounded(x, dt)
        assert not nc.passes(emu_layernorm(xr, gamma, beta, 1e-5, dt, "noeps"), nc.ln_ref(xr, gamma, beta, 1e-5), dt), (M, C)
    for M, Fd in nc.GEGLU_SHAPES[1:]:
        _, hr = nc.rounded(nc.geglu_draw(min(M, 37), Fd), dt)
        assert not nc.passes(emu_geglu(hr, dt, "tanh"), nc.geglu_ref(hr), dt), (M, Fd)
    for n in (63, 64, 65, 77):
        S, _ = nc.softmax_draw(5, n)
        assert not nc.passes(emu_softmax(S, nc.SOFTMAX_SCALE, dt, "nlast"), nc.softmax_ref(S, nc.SOFTMAX_SCALE), dt), n


def test_the_max_norm_measure_misses_what_the_bound_rejects():
    """The measure of test_nn_gpu.py, max|a - ref| / max|ref| < 1.2e-2, on the bf16 GroupNorm whose statistics skip the last pixel."""
    shape = (2, 100, 512, 32)
    outs, ref, *_ = _gn_fwd_case(shape, nc.BF16, 1e-5, 1, fault="lastpix")
    y = outs[0][1]
    assert float((y - ref).abs().max() / ref.abs().max()) < 1.2e-2
    assert not nc.passes(y, ref, nc.BF16)


# ------------------------------------------------------------------------------------------------------------------ guards
@DT
@pytest.mark.parametrize("n,ld", [(77, 88), (64, 72), (8, 8)])
def test_guarded_output_sees_a_write_outside_the_row(dt, n, ld):
    g = nc.Guarded(3, n, dt, "cpu", ld=ld)
    assert g.intact()
    vals = torch.randn(3, n)
    enc = nc.encode(vals, dt)                                             # f32x: padded to whole groups ...
    if dt == nc.F32X and n % 8:
        full = g.t[:, :enc.shape[-1]].clone().view(torch.float16).view(3, -1, 2, 8)
        new = enc.view(torch.float16).view(3, -1, 2, 8)
        k = n % 8                                                         # ... of which the last one is written in its first n % 8 lanes only
        full[:, :-1] = new[:, :-1]
        full[:, -1, :, :k] = new[:, -1, :, :k]
        g.t[:, :enc.shape[-1]] = full.view(3, -1).view(torch.int32)
    else:
        g.t[:, :n] = enc[:, :n]
    assert g.intact()
    assert torch.equal(g.values(), nc.round64(vals, dt))
    if ld > n:
        h = nc.Guarded(3, n, dt, "cpu", ld=ld)
        h.t[1, ld - 1] = 0                                                # a column between this row's end and the next row's start
        assert not h.intact()
    if dt == nc.F32X and n % 8:
        h = nc.Guarded(3, n, dt, "cpu", ld=ld)
        h.t.view(torch.float16).view(3, -1, 2, 8)[2, n // 8, 1, n % 8] = 0    # the lo half of the first unused lane of the last group
        assert not h.intact()
    for row in (-1, 3):
        h = nc.Guarded(3, n, dt, "cpu", ld=ld)
        h.raw.view(nc.TORCH_DT[dt]).view(3 + 4, ld)[2 + row, 0] = 0       # the guard rows before and after
        assert not h.intact()
