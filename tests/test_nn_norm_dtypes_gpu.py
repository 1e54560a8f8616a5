"""-m gpu: the six kernel families of csrc/nn_norm.hip, called alone through the C ABI (dwg_*_dt) in all four element types, against
float64 references of the rounded inputs -- per element, with the bound of nn_norm_cases.py (storage roundoff + 1e-5 of the output scale;
test_nn_norm_cases_host.py shows on the CPU that a correct fp32 implementation meets it and subtly wrong ones do not).  Every output sits
between sentinel guards; the GroupNorm tests also assert the saved statistics and WHICH launches ran, so a shape that stops taking the path
it was chosen for fails instead of silently testing another kernel.

GroupNorm forward shapes (B, HW, C, G) and the path each must take:
  (1, 64, 320, 32)    gn_small, bundle of 4 groups, 5 chunks, 51 pixel lanes; tail loop only
  (2, 1024, 640, 32)  gn_small, bundle of 2; 8-wide, 4-wide and tail loops all run
  (1, 9, 96, 32)      gn_small, bundle of 8 (3 channels per group), fewer pixels than pixel lanes
  (1, 50, 32, 32)     gn_small, one channel per group
  (1, 96, 512, 1)     gn_small at both of its limits: 64 chunks per bundle, HW x chunks = 6144
  (4, 1024, 256, 32)  gn_small at B = 4 and HW = 1024, one chunk per bundle (256 pixel lanes)
  (5, 64, 320, 32)    B = 5: gn_stats + gn_apply, partials folded into apply (no gn_finalize)
  (5, 100, 512, 32)   three-launch, folded; the 4-wide loops of both passes run
  (1, 1681, 320, 32)  HW > 1024, 33 partials: gn_finalize
  (5, 64, 512, 64)    G = 64: never folded
  (1, 625, 2560, 32)  6250 > 6144: three-launch; 320 chunks = two channel passes, group 25 straddles the pass boundary; 79 partials: gn_finalize
  (5, 16, 4096, 32)   two full 256-chunk passes, one pixel row per workgroup trip
  (1, 1025, 64, 32)   HW one past the small limit; 32 pixel rows in parallel with 16 pixels per block (idle rows)
plus two input distributions at small shapes: mean = 4 sigma (forward) / 2 sigma (backward), where the one-pass variance cancels, and a
variance of eps' size, where eps itself is visible.  Each test records its worst err / bound in parity_nn_norm.json, in the
measured-output directory of raster_cases.note_parity."""
import ctypes

import pytest
import torch

from tests import nn_norm_cases as nc

GPU = pytest.mark.gpu
DT = pytest.mark.parametrize("dt", nc.DTYPES, ids=nc.DT_IDS)
E_ARG = -1                                          # include/dwg_types.h


def _pp(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _note(name, **figs):
    from tests import raster_cases as rc
    rc.note_parity(name, {k: float(v) for k, v in figs.items()}, file="parity_nn_norm.json")


def _launches(fn):
    """Runs fn() (which returns the entry point's status) with the launch table on -> {name: launches}."""
    from dreamwaltz_g_amd import _lib
    _lib.prof_enable(True)
    try:
        rc = fn()
        torch.cuda.synchronize()
        table = _lib.prof_table()
    finally:
        _lib.prof_enable(False)
    assert rc == 0, rc
    return {k: v[0] for k, v in table.items()}


class _GN:
    """One GroupNorm case on the device: inputs of nn_norm_cases.gn_inputs, parameters, workspace."""

    def __init__(self, shape, dt, kind="plain"):
        from dreamwaltz_g_amd import _lib
        self.L, self.shape, self.dt = _lib.lib(), shape, dt
        B, HW, C, G = shape
        self.d = d = nc.gn_inputs(shape, dt, kind)
        self.x, self.dy, self.res = d["x_s"].cuda(), d["dy_s"].cuda(), d["res_s"].cuda()
        self.gamma, self.beta = d["gamma"].cuda(), d["beta"].cuda()
        self.ws = torch.empty(int(self.L.dwg_groupnorm_workspace_floats(B, G)), device="cuda")

    def forward(self, eps, silu):
        """-> (Guarded y, Guarded stats, launches)"""
        B, HW, C, G = self.shape
        y = nc.Guarded(B * HW, C, self.dt, "cuda")
        stats = nc.Guarded(B * G, 2, nc.F32, "cuda", guard=8)
        n = _launches(lambda: self.L.dwg_groupnorm_forward_dt(self.dt, B, HW, C, G, _pp(self.x), _pp(self.gamma), _pp(self.beta), eps, silu,
                                                              _pp(y.t), _pp(stats.t), _pp(self.ws), _st()))
        return y, stats, n

    def backward(self, eps, silu, stats, with_res):
        """stats: the device tensor the forward wrote -> (Guarded dx, Guarded scratch, launches)"""
        B, HW, C, G = self.shape
        dx = nc.Guarded(B * HW, C, self.dt, "cuda")
        scratch = nc.Guarded(B * G, 2, nc.F32, "cuda", guard=8)
        n = _launches(lambda: self.L.dwg_groupnorm_backward_dt(self.dt, B, HW, C, G, _pp(self.x), _pp(self.dy), _pp(stats), _pp(self.gamma),
                                                               _pp(self.beta), eps, silu, _pp(dx.t), _pp(scratch.t), _pp(self.ws),
                                                               _pp(self.res) if with_res else None, _st()))
        return dx, scratch, n

    def check_forward(self, eps, silu, launches, name):
        B, HW, C, G = self.shape
        y, stats, n = self.forward(eps, silu)
        assert n == {k: 1 for k in launches}, (name, n)
        ref, leaf = nc.gn_ref(self.d["x"], self.d["gamma"], self.d["beta"], G, eps, silu)
        w = nc.check(y.values().view(B, HW, C), ref.detach(), self.dt, name)
        rs, ra = nc.gn_stats_ref(self.d["x"], G)
        ws = nc.check_stats(stats.values().view(B, G, 2), rs, ra, name)
        assert y.intact() and stats.intact(), (name, "a write outside the output")
        _note(name, err_over_bound=w, stats_err_over_bound=ws)
        return stats, ref, leaf

    def check_backward(self, eps, silu, with_res, launches, name):
        """Forward first (its saved statistics are the backward's input, whichever kernel wrote them), then the input gradient."""
        B, HW, C, G = self.shape
        _, stats, _ = self.forward(eps, silu)
        ref, leaf = nc.gn_ref(self.d["x"], self.d["gamma"], self.d["beta"], G, eps, silu)
        gx = nc.gn_bwd_ref(ref, leaf, self.d["dy"])
        dx, scratch, n = self.backward(eps, silu, stats.t, with_res)
        assert n == {k: 1 for k in launches}, (name, n)
        # one store without a residual, two with it (nn_norm_cases docstring): the kernel rounds dx, adds the residual, rounds again
        store = nc.store_term(gx, self.dt) + nc.store_term(gx + self.d["res"], self.dt) if with_res else None
        w = nc.check(dx.values().view(B, HW, C), gx + self.d["res"] if with_res else gx, self.dt, name, store)
        assert dx.intact() and scratch.intact() and stats.intact(), (name, "a write outside the output")
        _note(name, err_over_bound=w)


def _id(shape):
    return "x".join(str(s) for s in shape)


@GPU
@DT
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("shape,launches", nc.GN_FWD, ids=[_id(s) for s, _ in nc.GN_FWD])
def test_groupnorm_forward(shape, launches, silu, dt):
    _GN(shape, dt).check_forward(nc.GN_EPS[shape], silu, launches, "gn_fwd %s silu=%d %s" % (_id(shape), silu, nc.DT_NAME[dt]))


@GPU
@DT
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("kind,shape", [("fwd4s", nc.GN_OFFSET_SHAPE), ("lowvar", nc.GN_LOWVAR_SHAPE)], ids=["mean_4_sigma", "low_variance"])
def test_groupnorm_forward_offset_and_low_variance(kind, shape, silu, dt):
    """x = 1.5 randn + 6: E[x^2] - m^2 loses m^2 / var = 16 of its digits and stays inside the bound (the limit is written down in
    nn_norm_cases.py).  x = 2e-3 randn: variance 4e-6 under eps = 1e-5 -- an eps that is dropped or misplaced shows in every element type."""
    _GN(shape, dt, kind).check_forward(1e-5, silu, nc.SMALL, "gn_fwd %s %s silu=%d %s" % (kind, _id(shape), silu, nc.DT_NAME[dt]))


@GPU
@DT
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("shape,launches", nc.GN_BWD, ids=[_id(s) for s, _ in nc.GN_BWD])
def test_groupnorm_backward(shape, launches, silu, with_res, dt):
    _GN(shape, dt).check_backward(nc.GN_EPS[shape], silu, with_res, launches,
                                  "gn_bwd %s silu=%d res=%d %s" % (_id(shape), silu, with_res, nc.DT_NAME[dt]))


@GPU
@DT
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_backward_mean_2_sigma(silu, with_res, dt):
    """x = 1.5 randn + 3; the statistics come from gn_small."""
    _GN(nc.GN_OFFSET_SHAPE, dt, "bwd2s").check_backward(1e-5, silu, with_res, ("gn_bwd_stats", "gn_bwd_apply"),
                                                        "gn_bwd bwd2s silu=%d res=%d %s" % (silu, with_res, nc.DT_NAME[dt]))


@GPU
@DT
@pytest.mark.parametrize("shape", [(1, 64, 320, 32), (1, 1681, 320, 32)], ids=["gn_small", "gn_finalize"])
def test_groupnorm_is_reproducible(shape, dt):
    """Forward and backward twice: outputs, saved statistics and backward sums bit for bit (the kernels document a fixed summation order)."""
    c = _GN(shape, dt)
    runs = []
    for _ in range(2):
        y, stats, _ = c.forward(1e-5, 1)
        dx, scratch, _ = c.backward(1e-5, 1, stats.t, True)
        torch.cuda.synchronize()
        runs.append((y.raw, stats.raw, dx.raw, scratch.raw))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@GPU
@DT
@pytest.mark.parametrize("M,C", nc.LN_SHAPES)
def test_layernorm(M, C, dt):
    """(5, 320): a partial last workgroup of 4 rows; (4, 520): 65 chunks, the second register slot used by one lane; (7, 2048): the maximum
    width.  Row 0 has a variance of eps' size."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    x, gamma, beta = nc.ln_draw(M, C)
    xs, xr = nc.rounded(x, dt)
    xs, gd, bd = xs.cuda(), gamma.cuda(), beta.cuda()
    y = nc.Guarded(M, C, dt, "cuda")
    n = _launches(lambda: L.dwg_layernorm_forward_dt(dt, M, C, _pp(xs), _pp(gd), _pp(bd), 1e-5, _pp(y.t), _st()))
    assert n == {"layernorm": 1}, n
    name = "layernorm %dx%d %s" % (M, C, nc.DT_NAME[dt])
    w = nc.check(y.values(), nc.ln_ref(xr, gamma, beta, 1e-5), dt, name)
    assert y.intact(), name
    _note(name, err_over_bound=w)


@GPU
@DT
@pytest.mark.parametrize("M,Fd", nc.GEGLU_SHAPES)
def test_geglu(M, Fd, dt):
    """(4100, 2048): 1 049 600 chunks, more than the 4096 x 256 threads of the largest grid -- the grid-stride loop takes a second trip."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    hs, hr = nc.rounded(nc.geglu_draw(M, Fd), dt)
    hs = hs.cuda()
    out = nc.Guarded(M, Fd, dt, "cuda")
    n = _launches(lambda: L.dwg_geglu_forward_dt(dt, M, Fd, _pp(hs), _pp(out.t), _st()))
    assert n == {"geglu": 1}, n
    name = "geglu %dx%d %s" % (M, Fd, nc.DT_NAME[dt])
    w = nc.check(out.values(), nc.geglu_ref(hr), dt, name)
    assert out.intact(), name
    _note(name, err_over_bound=w)


@GPU
@DT
@pytest.mark.parametrize("n", nc.SOFTMAX_N)
@pytest.mark.parametrize("rows,dominant", nc.SOFTMAX_CASES, ids=["1row_dominated", "5rows_dominated", "1row"])
def test_softmax_rows_forward_and_backward(rows, dominant, n, dt):
    """Strided rows on every operand (stride >= n + 8, a multiple of 8): the columns n .. ld-1 of P and dS are guards, in f32x with n % 8 != 0
    also the unused lanes of the last 32-byte group.  Row 0 holds a dominating score (S[0, 0] = 400: every other term underflows); the single
    row runs once more without it.  The backward runs on the P the forward stored, and its reference on those stored values.
    n = 1: P == 1, dS == 0 exactly."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    ld = nc.softmax_ld(n)
    S, dP = nc.softmax_draw(rows, n, dominant)
    Sd = torch.full((rows, ld), 1.0e4, device="cuda"); Sd[:, :n] = S.cuda()          # what lies between the rows would win every maximum
    dPd = torch.full((rows, ld), 1.0e4, device="cuda"); dPd[:, :n] = dP.cuda()
    P = nc.Guarded(rows, n, dt, "cuda", ld=ld)
    k = _launches(lambda: L.dwg_softmax_rows_forward_dt(dt, rows, n, nc.SOFTMAX_SCALE, _pp(Sd), ld, _pp(P.t), ld, _st()))
    assert k == {"softmax_rows": 1}, k
    name = "softmax %dx%d%s %s" % (rows, n, " dominated" if dominant else "", nc.DT_NAME[dt])
    Pv = P.values()
    w = nc.check(Pv, nc.softmax_ref(S, nc.SOFTMAX_SCALE), dt, name)
    assert P.intact(), name
    dS = nc.Guarded(rows, n, dt, "cuda", ld=ld)
    k = _launches(lambda: L.dwg_softmax_rows_backward_dt(dt, rows, n, nc.SOFTMAX_SCALE, _pp(P.t), ld, _pp(dPd), ld, _pp(dS.t), ld, _st()))
    assert k == {"softmax_rows_bwd": 1}, k
    wb = nc.check(dS.values(), nc.softmax_bwd_ref(Pv, dP, nc.SOFTMAX_SCALE), dt, name + " bwd")
    assert dS.intact() and P.intact(), name
    if n == 1:
        assert float((Pv - 1).abs().max()) == 0.0 and float(dS.values().abs().max()) == 0.0
    _note(name, err_over_bound=w, bwd_err_over_bound=wb)


def test_arguments_are_checked_on_the_host():
    """Fake non-null pointers: a call that got past the checks would launch on them, so every rejection below happens before any launch.
    Needs no GPU (not marked): it runs wherever the library loads."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)

    def gnf(dt, B=1, HW=64, C=320, G=32):
        return L.dwg_groupnorm_forward_dt(dt, B, HW, C, G, fake, fake, fake, 1e-5, 1, fake, fake, fake, None)

    def gnb(dt, B=1, HW=64, C=320, G=32):
        return L.dwg_groupnorm_backward_dt(dt, B, HW, C, G, fake, fake, fake, fake, fake, 1e-5, 1, fake, fake, fake, None, None)

    def smf(dt, rows=4, n=77, P=fake, ldp=88):
        return L.dwg_softmax_rows_forward_dt(dt, rows, n, 0.5, fake, 88, P, ldp, None)

    def smb(dt, rows=4, n=77, P=fake, ldp=88, dS=fake, ldds=88):
        return L.dwg_softmax_rows_backward_dt(dt, rows, n, 0.5, P, ldp, fake, 88, dS, ldds, None)

    for dt in nc.DTYPES:
        for f in (gnf, gnb):
            assert f(dt, C=324) == E_ARG            # C not a multiple of 8
            assert f(dt, C=328) == E_ARG            # C % G != 0
            assert f(dt, C=520, G=65) == E_ARG      # more than 64 groups
            assert f(dt, B=0) == E_ARG and f(dt, HW=0) == E_ARG
        assert L.dwg_layernorm_forward_dt(dt, 4, 2056, fake, fake, fake, 1e-5, fake, None) == E_ARG
        assert L.dwg_layernorm_forward_dt(dt, 4, 324, fake, fake, fake, 1e-5, fake, None) == E_ARG
        assert L.dwg_geglu_forward_dt(dt, 4, 12, fake, fake, None) == E_ARG
        assert smf(dt, n=0) == E_ARG and smb(dt, n=0) == E_ARG and smf(dt, rows=-1) == E_ARG
        # accepted, and nothing to do
        assert L.dwg_layernorm_forward_dt(dt, 0, 320, fake, fake, fake, 1e-5, fake, None) == 0
        assert L.dwg_geglu_forward_dt(dt, 0, 1280, fake, fake, None) == 0
        assert smf(dt, rows=0) == 0 and smb(dt, rows=0) == 0
    # an element type that does not exist
    assert gnf(4) == E_ARG and gnb(4) == E_ARG and smf(4) == E_ARG and smb(4) == E_ARG
    assert L.dwg_layernorm_forward_dt(4, 4, 320, fake, fake, fake, 1e-5, fake, None) == E_ARG
    assert L.dwg_geglu_forward_dt(4, 4, 1280, fake, fake, None) == E_ARG
    # f32x rows are addressed in 32-byte groups: a row stride that is not a multiple of 8, or a base off a 16-byte boundary, would scatter a
    # row's halves into its neighbours' groups -- rejected (the other element types take any stride)
    for ld in (77, 84, 81):
        assert smf(nc.F32X, ldp=ld) == E_ARG and smb(nc.F32X, ldp=ld) == E_ARG and smb(nc.F32X, ldds=ld) == E_ARG, ld
        assert smf(nc.F32X, rows=0, ldp=ld) == E_ARG
    assert smf(nc.F32X, P=odd) == E_ARG and smb(nc.F32X, P=odd) == E_ARG and smb(nc.F32X, dS=odd) == E_ARG
    for dt in (nc.BF16, nc.F16, nc.F32):
        assert smf(dt, rows=0, ldp=77) == 0 and smb(dt, rows=0, ldp=77, ldds=81) == 0 and smf(dt, rows=0, P=odd) == 0
