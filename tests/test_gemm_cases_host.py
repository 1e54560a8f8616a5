"""Proves the checker of gemm_cases.py on the CPU, without a GPU.  For every case of the table and every element type it applies to, fp32
emulations of a correct kernel -- the product formed whole, in the kernel's k-steps, and in the case's split-K slices summed in slice order;
for f32x as hi hi + (hi lo + lo hi) 2^-11 with fp32 sums -- meet the per-element bound with room to spare, and ten deliberately broken
emulations miss it on at least a stated share of the elements.

Headroom.  Before the output store the emulations must sit within 0.25 of the ARITHMETIC part of the bound, ARITH (|ref| + L S) (+ the erf
term of the GEGLU case), on every element, and after the store inside the whole bound.  (The ratio to the whole bound cannot be asserted
below 0.25 for a 16-bit output: a round-to-nearest store alone uses up to all of store(ref); for fp32 and f32x outputs the two figures
coincide.)

Floors of the mutants (share of the elements outside the bound), each from the size of the seeded error against the bound:
  ktail, last_slice  0.5   t dropped terms of K are an error of sqrt(t / K) sigma; against a bf16 store (2^-8 |ref|) at K = 12304 that is
                           4 sigma of the bound, so ~80 % fail; everywhere else nearly all do.  With input dilation d the tail lies in the
                           last tap, which meets a non-zero pixel at 1 / d^2 of the outputs: 0.5 / d^2 there
  bias_group         0.8 x (columns of the last group) / N      a wrong randn bias is never inside the bound, SiLU's flat tail aside
  res_ld             0.9   every row but the first reads other residuals
  alpha_after        0.8   (alpha - 1) bias, through the activation
  img_off            0.9   another image's randn bias
  halo               0.8 x (Ho + Wo - 1) / (Ho Wo)             the bottom row and the right column of the output see unzeroed pixels (the
                           ragged patch cases, and the asymmetric-pad case, whose only padding is below and to the right)
  upsample, cat      0.9   every output reads wrong pixels / channels
  x_drop             0.1   only at K <= 1024 (see the limit in gemm_cases.py): ~ 30 / sqrt(K) sigma of the bound
"""
import ctypes

import pytest
import torch

from tests import gemm_cases as gc

CASE_DT = pytest.mark.parametrize("case,dt", gc.CASE_DT, ids=gc.CASE_DT_IDS)
HEADROOM = 0.25


def _arith(P):
    return P.bound - gc.store_term(P.ref, P.case.out_dt(P.dt))


@CASE_DT
def test_correct_fp32_emulations_meet_the_bound_with_headroom(case, dt):
    P = gc.problem(case.name, dt)
    worst = {}
    for order in ("whole", "ksteps", "slices"):
        pre = gc.emulate(P, order, store=False)
        worst[order] = float(((pre - P.ref).abs() / _arith(P)).max())
        gc.check(gc.stored(P, pre), P, "%s %s" % (case.name, order))
    print("%s [%s] worst err / arithmetic bound before the store: %s" % (case.name, gc.DT_NAME[dt], worst))
    assert max(worst.values()) < HEADROOM, worst


def _is_patch(c):
    return c.symbol.startswith("k_conv3x3_patch2")


def _ragged_image(c):
    return c.pixel_tile is not None and (c.conv["H"] % c.pixel_tile[0] != 0 or c.conv["W"] % c.pixel_tile[1] != 0)


def _last_group(c):
    return c.N - (c.N - 1) // 4 * 4


# mutant -> (applies(case, dt), summation order, floor(case))
MUTANTS = {
    "ktail": (lambda c, dt: c.dims(dt)[2] % gc.KSTEP[dt] != 0, "whole", lambda c: 0.5 / (c.conv["dil"] ** 2 if c.conv else 1)),
    "last_slice": (lambda c, dt: c.slices > 1, "slices", lambda c: 0.5),
    "bias_group": (lambda c, dt: c.bias == "col" and c.act != "geglu_pair", "whole", lambda c: 0.8 * _last_group(c) / c.N),
    "res_ld": (lambda c, dt: c.residual, "whole", lambda c: 0.9),
    "alpha_after": (lambda c, dt: c.alpha != 1.0 and c.bias is not None, "whole", lambda c: 0.8),
    "img_off": (lambda c, dt: c.bias == "img" and c.conv["B"] > 1, "whole", lambda c: 0.9),
    "halo": (lambda c, dt: (_is_patch(c) and _ragged_image(c)) or c.name == "conv_asym_pad", "whole",
             lambda c: 0.8 * (c.conv["out"][0] + c.conv["out"][1] - 1) / (c.conv["out"][0] * c.conv["out"][1])),
    "upsample": (lambda c, dt: c.conv is not None and c.conv["up"] > 1, "whole", lambda c: 0.9),
    "cat": (lambda c, dt: c.conv is not None and c.conv["cin1"] > 0, "whole", lambda c: 0.9),
    "x_drop": (lambda c, dt: dt == gc.F32X and c.K <= 1024, "whole", lambda c: 0.1),
}
MUTANT_CASES = [(m, c, dt) for c, dt in gc.CASE_DT for m in MUTANTS if MUTANTS[m][0](c, dt)]       # by case: one reference serves its mutants


def test_every_mutant_has_cases_in_every_element_type_it_can_touch():
    for m in MUTANTS:
        dts = {dt for mm, c, dt in MUTANT_CASES if mm == m}
        assert dts >= ({gc.F32X} if m == "x_drop" else {gc.BF16, gc.F16, gc.F32X}), (m, dts)
    assert {dt for m, c, dt in MUTANT_CASES if m in ("ktail", "last_slice", "bias_group", "res_ld", "alpha_after")} == set(gc.DTYPES)


@pytest.mark.parametrize("mutant,case,dt", MUTANT_CASES, ids=["%s-%s-%s" % (m, c.name, gc.DT_NAME[dt]) for m, c, dt in MUTANT_CASES])
def test_broken_emulations_miss_the_bound(mutant, case, dt):
    _, order, floor = MUTANTS[mutant]
    P = gc.problem(case.name, dt)
    share = gc.outside(gc.emulate(P, order, mutant), P)
    print("%s %s [%s]: %.3f of the elements outside the bound (floor %.3f)" % (mutant, case.name, gc.DT_NAME[dt], share, floor(case)))
    assert share > floor(case), (mutant, case.name, share)


# ------------------------------------------------------------------------------------------------------------------ the table itself
@pytest.mark.parametrize("case", gc.CASES, ids=[c.name for c in gc.CASES])
def test_table_invariants(case):
    c = case
    bm, bn, bk = c.tile
    ragged = c.M % bm != 0 or c.N % bn != 0 or c.K % bk != 0 or _ragged_image(c)
    assert ragged, "no ragged dimension"
    if _is_patch(c) and _ragged_image(c):
        ph, pw = c.pixel_tile
        wgs = c.conv["B"] * -(-c.conv["H"] // ph) * -(-c.conv["W"] // pw) * -(-c.N // bn) * c.slices
        assert wgs % 8 != 0, wgs
    for dt in c.dts:
        if dt == gc.F32X:               # halves stay whole 8-groups
            M, N, K, Cin, cin1 = c.dims(dt)
            assert c.K % 16 == 0 and K % 8 == 0 and Cin % 8 == 0 and cin1 % 8 == 0
            assert (c.out != "elem" or c.ld_c % 8 == 0) and (not c.residual or c.res != "elem" or c.ld_r % 8 == 0)
            assert c.form != "heads" or (c.batch[1] * K) % 8 == 0
        for what, b in gc.operand_bytes(c, dt).items():
            assert b <= 64 << 20, (what, b)
    assert (c.splitk[0] in ("lib", "ws")) == c.epilogue and (c.slices > 1) == (c.splitk[0] != "none")


def test_the_asymmetric_pad_case_reads_past_the_bottom_and_right_only():
    """No top / left pad, at least one implied row and column of zeros at the bottom and right -- and every conv case's implied pad is
    non-negative (no case crops its input)."""
    pt, pl, pb, pr = gc.implied_pad(gc.BY_NAME["conv_asym_pad"].conv)
    assert pt == 0 and pl == 0 and pb >= 1 and pr >= 1, (pt, pl, pb, pr)
    for c in gc.CASES:
        if c.conv is not None:
            assert min(gc.implied_pad(c.conv)) >= 0, (c.name, gc.implied_pad(c.conv))


def test_output_and_residual_types_rotate_over_both_epilogues():
    """16-bit out + 16-bit residual, fp32 out + 16-bit residual, fp32 out + fp32 residual: each on an N % 4 == 0 case (the float4 epilogue)
    and on an N % 4 != 0 case (the general loop)."""
    for vec in (True, False):
        got = {(c.out, c.res) for c in gc.CASES if c.residual and gc.F32X in c.dts and (c.N % 4 == 0) == vec and c.splitk[0] == "none"}
        assert got >= {("elem", "elem"), ("f32", "elem"), ("f32", "f32")}, (vec, got)


def _fake_desc(c, dt):
    """The descriptor of (case, dt) with never-dereferenced pointers, for the host-only workspace query."""
    from dreamwaltz_g_amd import gemm
    kw = gc.desc_args(c, dt)
    d = gemm.GemmDesc()
    d.A, d.B, d.C = 1 << 20, 2 << 20, 3 << 20
    d.M, d.N, d.K = kw["M"], kw["N"], kw["K"]
    (d.a_row_stride, d.a_k_stride), (d.b_row_stride, d.b_k_stride) = kw["a_strides"], kw["b_strides"]
    d.ldc, d.ldr = kw["ldc"], kw["ldr"]
    d.batch1, d.batch2 = kw.get("batch", (1, 1))
    d.a_batch1_stride, d.a_batch2_stride = kw.get("a_batch", (0, 0))
    d.b_batch1_stride, d.b_batch2_stride = kw.get("b_batch", (0, 0))
    d.c_batch1_stride, d.c_batch2_stride = kw.get("c_batch", (0, 0))
    d.dtype, d.out_dtype, d.residual_dtype = dt, c.out_dt(dt), c.res_dt(dt)
    d.act, d.alpha, d.bias_per_row, d.accumulate, d.plan_m = gemm.ACT[c.act], c.alpha, int(kw["bias_per_row"]), int(c.accumulate), c.plan_m
    if c.bias:
        d.bias = 4 << 20
    if c.residual:
        d.residual = 5 << 20
    if "conv" in kw:
        d.conv_enabled = 1
        (d.conv_cin, d.conv_hin, d.conv_win, d.conv_hout, d.conv_wout, d.conv_kh, d.conv_kw, d.conv_stride, d.conv_pad_t, d.conv_pad_l,
         d.conv_in_dilation) = kw["conv"]
        d.conv_in_upsample = kw["conv_upsample"]
        if kw["cin1"]:
            d.A2, d.conv_cin1 = 6 << 20, kw["cin1"]
    d.bias_row_div, d.bias_ld = kw.get("bias_row_div", 0), kw.get("bias_ld", 0)
    return d


def test_workspace_query_is_positive_exactly_for_the_library_split_cases():
    try:
        from dreamwaltz_g_amd import _lib
        L = _lib.lib()
    except (RuntimeError, OSError) as e:
        pytest.skip("libdwg_hip.so does not load here: %s" % e)
    for c, dt in gc.CASE_DT + gc.REJECTED:
        d = _fake_desc(c, dt)
        d.splitk = 0                                    # "let the library choose"
        need = int(L.dwg_gemm_workspace_bytes(ctypes.byref(d)))
        rows = max(c.M, c.plan_m)
        assert (need > 0) == (c.splitk[0] == "lib" and dt in c.dts), (c.name, gc.DT_NAME[dt], need)
        assert need % (rows * c.N * 4) == 0 and need <= 64 << 20, (c.name, need)


def test_reference_and_emulation_share_nothing_but_the_inputs():
    """The conv reference goes through F.conv2d on NCHW, the emulation through this module's own im2col: on float64 they agree to rounding for
    every conv form of the table (so neither the bound nor the mutants rest on a mistake common to both)."""
    for c in gc.CASES:
        if c.conv is None or c.M * c.K > 1 << 22:
            continue
        dt = c.dts[0]
        P = gc.problem(c.name, dt)
        (a, b), = P.mats("val")
        ref = gc.conv_ref(P.sources("val"), gc.decode(P.b_s, dt), c.conv)
        assert torch.allclose(a @ b.t(), ref, rtol=0, atol=1e-12), c.name
