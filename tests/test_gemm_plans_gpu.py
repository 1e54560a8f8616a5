"""-m gpu: every kernel plan of csrc/gemm.hip's make_plan, one launch each through the C ABI, in every element type the plan exists for
(bf16, f16, f32x from the 16-bit kernels; exact f32), against the float64 reference of the rounded inputs -- per element, with the bound of
gemm_cases.py (test_gemm_cases_host.py shows on the CPU that correct fp32 implementations meet it with room and subtly wrong ones do not).

Each test builds the descriptor with gemm.gemm_raw(run=False), attaches the workspace the case asks for (the library's own query, an explicit
slab workspace, or none), runs it once with the launch table on and asserts, in this order:
  1. the set of launched profiler symbols is exactly the case's -- the kernel instantiation, plus k_splitk_epilogue where the split goes
     through slabs and never otherwise -- so a retuned threshold that moves a case onto another plan fails here instead of silently testing
     another kernel;
  2. the output is finite and inside the bound on every element;
  3. every byte around the output (guard rows, the columns N .. ldc - 1 of every row, for plan_m the rows past the launched M) and around the
     slab workspace still holds the sentinel.
The worst err / bound of each case goes to parity_gemm.json in the measured-output directory of raster_cases.note_parity."""
import ctypes
import os

import pytest
import torch

from tests import gemm_cases as gc

pytestmark = pytest.mark.gpu
E_ARG = -1                                          # include/dwg_types.h
EPILOGUE = "k_splitk_epilogue"
WS_GUARD = 4096                                     # sentinel bytes on either side of the slab workspace


def _note(name, worst):
    from tests import raster_cases as rc
    rc.note_parity(name, {"err_over_bound": float(worst)}, file="parity_gemm.json")


def _descriptor(c, dt, P, out):
    """-> (descriptor, the device tensors it points to)"""
    from dreamwaltz_g_amd import gemm
    kw = gc.desc_args(c, dt)
    keep = dict(A=P.a_s.cuda(), B=P.b_s.cuda(), A2=P.a2_s.cuda() if c.conv and P.a2_s is not None else None,
                bias=P.bias.contiguous().cuda() if P.bias is not None else None, res=P.res_s.cuda() if P.res_s is not None else None)
    M, N, K = kw.pop("M"), kw.pop("N"), kw.pop("K")
    d = gemm.gemm_raw(keep["A"], keep["B"], out.t, M, N, K, kw.pop("a_strides"), kw.pop("b_strides"), kw.pop("ldc"), bias=keep["bias"],
                      residual=keep["res"], A2=keep["A2"], run=False, **kw)
    return d, keep


def _workspace(c, d):
    """Sizes and attaches the workspace as the case says -> (raw sentinel-filled allocation or None, bytes)."""
    from dreamwaltz_g_amd import _lib
    mode, n = c.splitk
    if mode == "lib":
        need = int(_lib.lib().dwg_gemm_workspace_bytes(ctypes.byref(d)))
        assert need > 0, "the library would not split this case"
    elif mode == "ws":
        need = n * d.M * d.N * 4
    else:
        return None, 0
    raw = torch.full((need + 2 * WS_GUARD,), gc.nc.SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    d.workspace, d.workspace_bytes = raw.data_ptr() + WS_GUARD, need
    assert d.workspace % 16 == 0
    return raw, need


def _run(c, d):
    """One launch with the launch table on -> {profiler symbol: launches}"""
    from dreamwaltz_g_amd import gemm, _lib
    before = os.environ.pop("DWG_CONV_PATCH_MINM", None)          # the case's threshold (none: the library's default) for this launch only
    if c.minm is not None:
        os.environ["DWG_CONV_PATCH_MINM"] = str(c.minm)
    try:
        _lib.prof_enable(True)
        try:
            gemm.run_desc(d, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            syms = _lib.prof_symbols()
        finally:
            _lib.prof_enable(False)
    finally:
        os.environ.pop("DWG_CONV_PATCH_MINM", None)
        if before is not None:
            os.environ["DWG_CONV_PATCH_MINM"] = before
    return {k: v[0] for k, v in syms.items()}


@pytest.mark.parametrize("case,dt", gc.CASE_DT, ids=gc.CASE_DT_IDS)
def test_plan_launches_its_kernel_and_matches_float64(case, dt):
    c = case
    name = "%s [%s]" % (c.name, gc.DT_NAME[dt])
    P = gc.problem(c.name, dt)
    guard = 2 if not c.plan_m else c.plan_m - c.M + 8          # plan_m: every row a launch sized for plan_m rows could reach
    out = gc.Guarded(c.rows, c.ncols, c.out_dt(dt), "cuda", ld=c.ld_c, guard=guard)
    if c.splitk[0] == "atomic":
        out.t[:, :c.ncols] = 0                                  # the slices add into a zeroed fp32 C
    if c.accumulate:
        out.t[:, :c.ncols] = P.prior.cuda()
    d, keep = _descriptor(c, dt, P, out)
    ws, need = _workspace(c, d)
    launched = _run(c, d)
    want = {c.symbol_of(dt): 1}
    if c.epilogue:
        want[EPILOGUE] = 1
    assert launched == want, (name, launched)
    worst = gc.check(out.values(), P, name)
    assert out.intact(), (name, "a write outside the output")
    if ws is not None:
        edge = torch.cat([ws[:WS_GUARD], ws[WS_GUARD + need:]]).cpu()
        assert bool((edge == gc.nc.SENTINEL_BYTE).all()), (name, "a write outside the slab workspace")
    _note(name, worst)
    del keep


@pytest.mark.parametrize("case,dt", gc.REJECTED, ids=["%s-%s" % (c.name, gc.DT_NAME[dt]) for c, dt in gc.REJECTED])
def test_shapes_the_format_cannot_express_are_argument_errors(case, dt):
    """The register-staged kernels' shapes (K % 8 != 0) have no split-precision form: DWG_E_ARG, nothing launched, nothing written."""
    from dreamwaltz_g_amd import _lib, gemm
    c = case
    M, N, K, _, _ = c.dims(dt)
    Kp = (K + 7) // 8 * 8
    A, B = torch.zeros(M, Kp, dtype=torch.int32, device="cuda"), torch.zeros(N, Kp, dtype=torch.int32, device="cuda")
    out = gc.Guarded(M, N, dt, "cuda", ld=c.ld_c)
    d = gemm.gemm_raw(A, B, out.t, M, N, K, (Kp, 1), (Kp, 1), c.ld_c, run=False)
    _lib.prof_enable(True)
    try:
        rc = _lib.lib().dwg_gemm(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        syms = _lib.prof_symbols()
    finally:
        _lib.prof_enable(False)
    assert rc == E_ARG and not syms, (rc, syms)
    written = out.raw.cpu()
    assert bool((written == gc.nc.SENTINEL_BYTE).all())
