"""-m gpu: every kernel instantiation, tail, split and addressing path of the fused attention (csrc/attention.hip, attention_f16.hip,
attention_x.hip), one launch each through the C ABI, in bf16, f16 and f32x, against the float64 reference of the rounded inputs -- per
element, with the bound of attention_cases.py (test_attention_cases_host.py shows on the CPU that correct fp32 implementations of the
kernels' formulas meet it and subtly wrong ones do not).

Each test uploads the case's operands, calls the entry point its layout names -- dwg_attention_forward_dt, dwg_attention_forward_ws with a
NaN-filled workspace for the split cases, dwg_attention_forward_pairs_dt for the two-level batch -- on the current stream with the launch
table on and the output inside sentinel guards, and asserts, in this order:
  1. the workspace query returns exactly what attention_cases.workspace_bytes mirrors (0 where the library would not split);
  2. the set of launched profiler symbols is exactly the instantiation of (d, dtype), plus k_flash_merge_x (`flash_attn_merge`) where the case
     splits its keys and never otherwise -- a too-small or misaligned workspace must run unsplit;
  3. the output is finite, inside the bound on every element, and equal to V[argmax] on the one-key / one-hot rows;
  4. every byte between the rows, between the images and around the output still holds the sentinel;
  5. for the split cases: a second run gives the same bits (include/dwg_nn.h: merged in a fixed order, run-to-run reproducible).
The worst err / bound of each case goes to parity_attention.json in the measured-output directory of raster_cases.note_parity."""
import ctypes

import pytest
import torch

from tests import attention_cases as ac

pytestmark = pytest.mark.gpu


def _note(name, worst):
    from tests import raster_cases as rc
    rc.note_parity(name, {"err_over_bound": float(worst)}, file="parity_attention.json")


def _launch(L, c, dt, P, dev, out, ws, ws_bytes):
    es = ac.nc.ELEM_BYTES[dt]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def op(n):
        t, off, ld, b, o = P.ops[n]
        return ctypes.c_void_p(dev[id(t)].data_ptr() + off * es), ld, b, o
    (q, ldq, bq, _), (k, ldk, bk, ok), (v, ldv, bv, ov) = op("Q"), op("K"), op("V")
    o = ctypes.c_void_p(out.t.data_ptr())
    if c.layout == "pairs":
        assert ws is None
        return L.dwg_attention_forward_pairs_dt(dt, c.R, c.Bq, c.H, c.Nq, c.Nk, c.d, q, ldq, bq, 0, k, ldk, bk, ok, v, ldv, bv, ov, o, c.ldo, c.bo,
                                                c.oo, P.scale, st)
    if ws is not None:
        return L.dwg_attention_forward_ws(dt, c.B, c.H, c.Nq, c.Nk, c.d, q, ldq, bq, k, ldk, bk, v, ldv, bv, o, c.ldo, c.bo, P.scale,
                                          ctypes.c_void_p(ws), ws_bytes, st)
    return L.dwg_attention_forward_dt(dt, c.B, c.H, c.Nq, c.Nk, c.d, q, ldq, bq, k, ldk, bk, v, ldv, bv, o, c.ldo, c.bo, P.scale, st)


@pytest.mark.parametrize("case,dt", ac.CASE_DT, ids=ac.CASE_DT_IDS)
def test_kernel_launches_its_instantiation_and_matches_float64(case, dt):
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    c = case
    name = "%s [%s]" % (c.name, ac.DT_NAME[dt])
    P = ac.problem(c.name, dt)
    need = int(L.dwg_attention_split_workspace_bytes(dt, c.B, c.H, c.Nq, c.Nk, c.d))
    assert need == (ac.workspace_bytes(c.B, c.H, c.Nq, c.Nk, c.d) if dt == ac.F32X else 0), (name, need)
    dev = {id(t): t.cuda() for t, _, _, _, _ in P.ops.values()}
    wsbuf, ws, ws_bytes = None, None, 0
    if c.ws != "none":
        assert need > 0, name
        wsbuf = torch.empty(need // 4 + 8, device="cuda")
        ws, ws_bytes = wsbuf.data_ptr() + (8 if c.ws == "misaligned" else 0), need - (16 if c.ws == "small" else 0)
    nsplit = c.nsplit(dt)
    want = {P.symbol: 1}
    if nsplit > 1:
        want[ac.MERGE_SYMBOL] = 1
    runs = []
    for _ in range(2 if nsplit > 1 else 1):
        out = ac.GuardedO(c, dt, "cuda")
        if wsbuf is not None:
            wsbuf.fill_(float("nan"))
        _lib.prof_enable(True)
        try:
            rc = _launch(L, c, dt, P, dev, out, ws, ws_bytes)
            torch.cuda.synchronize()
            launched, names = {k: v[0] for k, v in _lib.prof_symbols().items()}, _lib.prof_table()
        finally:
            _lib.prof_enable(False)
        assert rc == 0, (name, rc)
        assert launched == want, (name, launched)
        assert (ac.MERGE in names) == (nsplit > 1) and P.pname in names, (name, names)
        runs.append(out)
    out = runs[0]
    worst = ac.check(out.values(), P, name)
    assert out.intact(), (name, "a write outside the output")
    if len(runs) > 1:
        assert torch.equal(runs[0].raw, runs[1].raw), (name, "two runs of a split launch differ")
    _note(name, worst)
