"""The two-level batch of the fused attention (include/dwg_nn.h dwg_attention_forward_pairs_dt / _ws) and the broadcast channel concat
(include/dwg_elementwise.h dwg_concat_channels_bcast): what a shared-prefix denoiser plan (sd15.DenoiserPlan) uses where its V-row stream
widens to the 2 V entries of the CFG batch.

Both only change ADDRESSES: image (r, v) of R x Bq reads the queries of view v (outer Q stride 0) and batch row r Bq + v of K, V and O; grid,
key split and per-workgroup arithmetic are the plain entry point's over B = R Bq images.  So the bar is bit equality with the plain entry point
on Q materialised R times (and with the plain concat on the second operand repeated R times).  The argument checks run on the host before any
device call and need no GPU."""
import ctypes

import pytest
import torch

F32, BF16, F16, F32X = 0, 1, 2, 3
E_ARG = -1                                          # include/dwg_types.h
R, BQ, H = 2, 2, 2


def _pp(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to_dev(x, dt):
    from dreamwaltz_g_amd import xfmt
    if dt == F32X:
        return xfmt.pack(x).cuda()
    return x.to(torch.float16 if dt == F16 else torch.bfloat16).cuda()


def _draw(Nq, Nk, d, dt):
    """Q [Bq, Nq, H d] (a different draw per view, so that a wrong b mod Bq shows), K / V [R Bq, Nk, H d] (different per batch row)."""
    g = torch.Generator().manual_seed(1000 * Nq + 10 * Nk + d)
    q = torch.randn(BQ, Nq, H * d, generator=g)
    k = torch.randn(R * BQ, Nk, H * d, generator=g)
    v = torch.randn(R * BQ, Nk, H * d, generator=g)
    assert not torch.equal(q[0], q[1])
    return _to_dev(q, dt), _to_dev(k, dt), _to_dev(v, dt)


def _pairs(L, dt, q, k, v, Nq, Nk, d, ws=None, need=0):
    o = torch.empty(R * BQ, Nq, q.shape[-1], device="cuda", dtype=q.dtype)
    ld = H * d
    rc = L.dwg_attention_forward_pairs_ws(dt, R, BQ, H, Nq, Nk, d, _pp(q), ld, Nq * ld, 0, _pp(k), ld, Nk * ld, BQ * Nk * ld,
                                          _pp(v), ld, Nk * ld, BQ * Nk * ld, _pp(o), ld, Nq * ld, BQ * Nq * ld, float(d) ** -0.5,
                                          _pp(ws) if ws is not None else None, need, _st())
    assert rc == 0, rc
    return o


def _plain(L, dt, q, k, v, Nq, Nk, d, ws=None, need=0):
    qr = q.repeat(R, 1, 1).contiguous()             # rows [q_0, q_1, q_0, q_1]: batch row r Bq + v holds view v's queries
    o = torch.empty(R * BQ, Nq, q.shape[-1], device="cuda", dtype=q.dtype)
    ld = H * d
    rc = L.dwg_attention_forward_ws(dt, R * BQ, H, Nq, Nk, d, _pp(qr), ld, Nq * ld, _pp(k), ld, Nk * ld, _pp(v), ld, Nk * ld, _pp(o), ld, Nq * ld,
                                    float(d) ** -0.5, _pp(ws) if ws is not None else None, need, _st())
    assert rc == 0, rc
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32X, F16, BF16], ids=["f32x", "f16", "bf16"])
@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("Nk", [77, 130])
def test_pairs_equal_the_plain_entry_on_repeated_queries_bit_for_bit(dt, d, Nk):
    """Nq = 130: two query blocks, the second ragged; 77 keys (cross-attention, a masked tail tile) and 130."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    Nq = 130
    q, k, v = _draw(Nq, Nk, d, dt)
    a, b = _pairs(L, dt, q, k, v, Nq, Nk, d), _plain(L, dt, q, k, v, Nq, Nk, d)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # the entries are what they should be, not merely equal: view 0's and view 1's outputs differ, and so do the two outer entries of a view
    assert not torch.equal(a[0].view(torch.uint8), a[1].view(torch.uint8)) and not torch.equal(a[0].view(torch.uint8), a[2].view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [40, 160])
def test_pairs_through_the_key_split_and_merge_launches_bit_for_bit(d):
    """A launch small enough in Nq to split its keys over workgroups (one query block per image and head, 330 keys): the partial results
    in the workspace and the merge launch address their outputs through the same two-level batch."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    Nq, Nk = 64, 330
    need = int(L.dwg_attention_split_workspace_bytes(F32X, R * BQ, H, Nq, Nk, d))
    assert need > 0
    q, k, v = _draw(Nq, Nk, d, F32X)
    ws = torch.empty(need // 4, device="cuda")
    outs = []
    for f in (_pairs, _plain):
        ws.fill_(float("nan"))
        _lib.prof_enable(True)
        outs.append(f(L, F32X, q, k, v, Nq, Nk, d, ws, need))
        torch.cuda.synchronize()
        names = _lib.prof_table(); _lib.prof_enable(False)
        assert "flash_attn_merge" in names, names.keys()
    assert torch.equal(outs[0], outs[1])
    assert not torch.equal(outs[0][0], outs[0][1]) and not torch.equal(outs[0][0], outs[0][2])


@pytest.mark.gpu
@pytest.mark.parametrize("Ca,Cb", [(320, 320), (8, 24)])
def test_concat_with_a_broadcast_second_operand_bit_for_bit(Ca, Cb):
    """rows = 2 x 2 x (5 x 7) pixels, the second operand has the 2 x (5 x 7) rows of one outer entry."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    rows_b = 2 * 5 * 7
    rows = 2 * rows_b
    g = torch.Generator().manual_seed(Ca + Cb)
    a = torch.randn(rows, Ca, generator=g).to(torch.bfloat16).cuda()
    b = torch.randn(rows_b, Cb, generator=g).to(torch.bfloat16).cuda()
    got = torch.empty(rows, Ca + Cb, device="cuda", dtype=torch.bfloat16)
    ref = torch.empty_like(got)
    assert L.dwg_concat_channels_bcast(rows, rows_b, Ca, Cb, _pp(a), _pp(b), _pp(got), _st()) == 0
    assert L.dwg_concat_channels(rows, Ca, Cb, _pp(a), _pp(b.repeat(2, 1).contiguous()), _pp(ref), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(got[:, Ca:].view(torch.int16), torch.cat([b, b]).view(torch.int16)) and torch.equal(got[:, :Ca].view(torch.int16), a.view(torch.int16))


def test_pair_arguments_are_checked_on_the_host():
    """Bad strides, counts and null pointers are DWG_E_ARG before any device call: strides in whole 8-element groups, outer stride 0 for the
    queries only."""
    from dreamwaltz_g_amd import _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    Nq, Nk, d = 130, 77, 40
    ld = H * d

    def call(dt=F32X, Rr=R, Bq=BQ, Hh=H, dd=d, Q=fake, K=fake, V=fake, O=fake, oq=0, ok=BQ * Nk * ld, ov=BQ * Nk * ld, oo=BQ * Nq * ld, bq=Nq * ld,
             ldq=ld, ws=False, scale=None):
        args = (dt, Rr, Bq, Hh, Nq, Nk, dd, Q, ldq, bq, oq, K, ld, Nk * ld, ok, V, ld, Nk * ld, ov, O, ld, Nq * ld, oo,
                float(dd) ** -0.5 if scale is None else scale)
        return L.dwg_attention_forward_pairs_ws(*args, None, 0, None) if ws else L.dwg_attention_forward_pairs_dt(*args, None)

    def plain(dt, ws, scale):
        """The one-level entry points: dwg_attention_forward_dt / _ws over B = R Bq images."""
        args = (dt, R * BQ, H, Nq, Nk, d, fake, ld, Nq * ld, fake, ld, Nk * ld, fake, ld, Nk * ld, fake, ld, Nq * ld, scale)
        return L.dwg_attention_forward_ws(*args, None, 0, None) if ws else L.dwg_attention_forward_dt(*args, None)
    for dt in (F32X, F16, BF16):
        for ws in (False, True):
            for bad in (dict(Q=None), dict(K=None), dict(V=None), dict(O=None), dict(Q=odd), dict(O=odd), dict(ok=0), dict(ov=0), dict(oo=0),
                        dict(oq=4), dict(ok=BQ * Nk * ld + 4), dict(ov=12), dict(oo=BQ * Nq * ld + 2), dict(bq=Nq * ld + 4), dict(ldq=ld + 1),
                        dict(Rr=0), dict(Bq=0), dict(Rr=-1), dict(Hh=0), dict(dd=44), dict(dd=168), dict(Rr=300, Bq=300)):
                assert call(dt=dt, ws=ws, **bad) == E_ARG, (dt, ws, bad)
            # the scale is folded into the exponent as a positive factor: 0, negative, NaN and inf are argument errors, on every entry point
            for scale in (0.0, -0.0, -0.158, float("nan"), float("inf"), -float("inf")):
                assert call(dt=dt, ws=ws, scale=scale) == E_ARG, (dt, ws, scale)
                assert plain(dt, ws, scale) == E_ARG, (dt, ws, scale)
    for scale in (0.0, -0.158, float("nan"), float("inf")):
        assert L.dwg_attention_forward(R * BQ, H, Nq, Nk, d, fake, ld, Nq * ld, fake, ld, Nk * ld, fake, ld, Nk * ld, fake, ld, Nq * ld, scale, None) == E_ARG
    assert call(dt=F32) == E_ARG and call(dt=7, ws=True) == E_ARG          # the exact-f32 plans run attention on dwg_gemm
    fn = L.dwg_concat_channels_bcast
    assert fn(0, 70, 320, 320, fake, fake, fake, None) == 0
    for bad in ((140, 0, 320, 320, fake, fake, fake), (140, 60, 320, 320, fake, fake, fake), (140, 70, 4, 320, fake, fake, fake),
                (140, 70, 320, 12, fake, fake, fake), (140, 70, 320, 320, None, fake, fake), (140, 70, 320, 320, fake, None, fake),
                (140, 70, 320, 320, fake, fake, None), (-1, 70, 320, 320, fake, fake, fake)):
        assert fn(*bad, None) == E_ARG, bad
