"""Shared pieces of the kernel-level parity tests of the fused attention (csrc/attention.hip: bf16, attention_f16.hip: f16, attention_x.hip:
split-precision f32x): the case table -- every kernel instantiation, tail, split and addressing path the launchers can take -- the inputs, the
float64 reference, the per-element bound and fp32 emulations of correct kernels and of subtly wrong ones.  Used by
test_attention_kernels_gpu.py (the kernels, called through the C ABI with the output between sentinel guards and the launched profiler symbols
asserted) and test_attention_cases_host.py (the proof, on the CPU, that the bound is met by correct fp32 implementations of the kernels'
formulas and missed by the mutants).

Storage.  As in nn_norm_cases.py: inputs are drawn in fp32 with a seeded generator, rounded to the element type, and the float64 reference is
computed from the ROUNDED values (the scale, too, is the fp32 number the entry point receives).

Reference, per (image, head), float64:   P = softmax(scale Q K^T),   O = P V,   and two products of absolute values
        S[q, c] = sum_k P[q, k] |V[k, c]|                 T[q] = scale max_k sum_i |Q[q, i]| |K[k, i]|

The bound, per element, never a global maximum:

        |out - ref| <= store(ref) + (U_P + ARITH + 2 U_S T[q]) S[q, c] + F16_SUB[q, c]

Derivation.  A kernel computes O' = sum_k P'_k V_k / sum_k P'_k with P'_k = P_k (1 + e_k) up to a common factor (the running maximum, exact
or rounded up, cancels).  With |e_k| <= e:  |O' - O| <= 2 e S / (1 - e)  -- numerator and denominator each move by at most e, relative to S
and to 1.  The sources of e:
  * U_P, the rounding of P to the operand type of the PV product: bf16 2^-9 and f16 2^-12 per rounding, once in the numerator and once in the
    denominator (the ones-row instantiations sum the rounded P; the others sum the fp32 P, which only removes the second half), so
    U_P = 2^-8 / 2^-11 as a whole.  f32x splits P into hi + lo 2^-11 (22 bits): U_P = 0, the split is inside ARITH.
  * U_S, the relative error of one score product, against T: a score off by U_S T changes every probability by at most exp(2 U_S T) (one
    factor for the score, one for the maximum), hence 2 U_S T S.  bf16 / f16: the inputs are exact and the sum is fp32, U_S = 2^-23.
    f32x: 2^-20, the "4 units of 2^-22" of k_flash_fwd_x2's header (the dropped lo lo term, the fp32 sums, the re-split scaled query).
  * ARITH = 1e-5, the project's bar for fp32-grade arithmetic: exp2, the fp32 sums of the PV product and of l, the reciprocal, the merge.
  * F16_SUB, f16 only: probabilities below 2^-14 are subnormal halves with an absolute error of 2^-25 each, which U_P (relative) does not
    cover: F16_SUB = 2^-25 sum_k |V[k, c]| / L[q] with L[q] = sum_k exp(s_k - max s) >= 1.
  * store(ref) is nn_norm_cases.store_term for the output type.
No tolerance is fitted to the kernels; the emulations below (correct fp32 implementations of the kernels' formulas) stay under the bound as
derived, without a correction.

Exact cases, no bound: with one key, and on a row of kind `large` whose best key leads by more than 200, every other probability is 0 and
O == V[argmax] -- bit for bit in bf16 / f16 (P = 1, l = 1), within store(ref) alone in f32x (the hi + lo split of P V and of the output).

Limit of the bound.  A wrong SCORE is seen only through the probabilities it changes: score errors e_k move O by sum_k P_k e_k (V_k - O),
against an allowance of (U_P + ARITH + 2 U_S T) S.  A dropped cross term of the f32x QK^T product is e_k ~ 2^-13 scale |q . k|_2 ~ 6e-5 on
randn inputs, i.e. ~ 6e-5 sqrt(sum P_k^2) |V - O| ~ 1.2e-5 in O at 77 .. 97 keys -- the SIZE of the f32x bound at kind plain
((1e-5 + 2^-19 T) S with T ~ 5 .. 12, S ~ 0.8), so that about half of the elements fall outside it, fewer as d (and with it T) grows.
It is not seen (1) where 2 U_S T exceeds U_P + ARITH by much: `negative`, `large`, `late_max` (T of 150 to several hundred: the f32x bound is
1e-4 .. 1e-3 S); (2) where S is large against |V - O|: `offset_v` (S ~ 100, |V - O| ~ 1); (3) on saturated rows (`large`, `early_max`,
`late_max`: one key holds the mass) and where every key has the same error (`uniform`).  The mutant is therefore asserted at kind plain, at
every head size, and nowhere else.

Mutants the bound cannot see: an EMPTY key range merged with weight 1 instead of 0 -- its partial is exactly (O = 0, l = 0), so any finite
weight gives the same bits (asserted as such); what can go wrong with an empty range is a partial that is not written at all, and that
mutant (`empty_stale`: the NaN fill of the workspace survives) fails on every element.

Worst err / bound over the whole table:
  fp32 emulations (test_attention_cases_host.py, CPU):   bf16 0.54 (keys_d40_nk33)   f16 0.63 (kind_late_max_d160)   f32x 0.35 (kind_late_max_d160)
  the kernels on an MI355X (parity_attention.json):      bf16 0.54 (keys_d40_nk33)   f16 0.56 (kind_large_d48)       f32x 0.17 (kind_late_max_d160)
The 16-bit figures are the two roundings the bound is made of, the output store and the rounding of P, which a correct kernel uses up to
about half; kernel and emulation agree there to the digit.  In f32x the worst cases are the late_max ones, split or not (0.09 .. 0.17),
everything else is below 0.1.
"""
import functools

import torch

from tests.nn_norm_cases import ARITH, DT_NAME, Guarded, decode, encode, rounded, store_term  # noqa: F401 (re-exported to both tests)
from tests import nn_norm_cases as nc
from tests.gemm_cases import component

F32, BF16, F16, F32X = nc.F32, nc.BF16, nc.F16, nc.F32X
ALL3 = (BF16, F16, F32X)
U_P = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32X: 0.0}
U_S = {BF16: 2.0 ** -23, F16: 2.0 ** -23, F32X: 2.0 ** -20}
LOG2E = 1.4426950408889634
KINDS = ("plain", "offset_v", "uniform", "early_max", "late_max", "large", "negative")
MERGE, MERGE_SYMBOL = "flash_attn_merge", "k_flash_merge_x"


# ------------------------------------------------------------------------------------------------------------------ the launchers, mirrored
def kernel_of(d, dt):
    """(profiler name, profiler symbol, keys per tile, 'flash' | 'x' | 'x2', ones row) of head size d in element type dt."""
    if dt == F32X:
        if d in (40, 80):
            return "flash_attn_d%d" % d, "k_flash_fwd_x2<%d, 64, %d>" % (d, 2 if d == 40 else 1), 64, "x2", True
        dk, dv, mb = (32, 32, 2) if d <= 32 else (48, 64, 2) if d <= 48 else (64, 64, 2) if d <= 64 else (96, 96, 1) if d <= 96 else (160, 160, 1)
        return "flash_attn_d%d" % dk, "k_flash_fwd_x<%d, %d, %d>" % (dk, dv, mb), 32, "x", False
    dk, dv = (32, 32) if d <= 32 else (48, 64) if d <= 48 else (64, 64) if d <= 64 else (96, 96) if d <= 96 else (160, 160)
    return "flash_attn_d%d" % dk, "k_flash_fwd<%d, %d, %d>" % (dk, dv, d if d in (40, 80) else 0), 32, "flash", d in (40, 80)


def splits(B, H, Nq, Nk, d):
    """Key ranges an f32x launch with a workspace uses (attn_splits of attention_x.hip): enough for ~512 workgroups, at least two tiles
    per range, at most eight."""
    kt = 64 if d in (40, 80) else 32
    base, ntiles = -(-Nq // 128) * B * H, -(-Nk // kt)
    sp = 1 if base >= 256 else min(-(-512 // base), 8, ntiles // 2)
    return 1 if sp < 2 else sp


def workspace_bytes(B, H, Nq, Nk, d):
    sp = splits(B, H, Nq, Nk, d)
    dv = 32 if d <= 32 else 64 if d <= 64 else 96 if d <= 96 else 160
    return sp * B * H * Nq * (dv + 4) * 4 if sp > 1 else 0


class Case:
    """layout: 'dense' Q / K / V / O tensors of their own, no padding | 'sliced' Q, K, V column slices of one [B, N, 3 H d + 8] tensor, O with
    ldo = H d + 8 and bo = Nq ldo + 16 | 'pairs' the two-level batch R = 2, Bq = 2, oq = 0 (B = 4 images, two query sets), O padded as for
    'sliced'.  ws (f32x only): 'none' no workspace | 'split' the queried workspace, NaN-filled | 'small' 16 bytes short | 'misaligned' 8 bytes
    off a 16-byte boundary -- the last two must run unsplit."""

    def __init__(self, name, d, Nq, Nk, B=1, H=2, kind="plain", layout="dense", ws="none", dts=ALL3):
        self.name, self.d, self.Nq, self.Nk, self.B, self.H, self.kind, self.layout, self.ws, self.dts = name, d, Nq, Nk, B, H, kind, layout, ws, dts
        self.R, self.Bq = (2, B // 2) if layout == "pairs" else (1, B)
        self.ldo = H * d + (0 if layout == "dense" else 8)
        self.bo = Nq * self.ldo + (0 if layout == "dense" else 16)
        self.oo = self.Bq * self.bo

    def __repr__(self):
        return self.name

    def nsplit(self, dt):
        """Key ranges the launch of this case must use."""
        return splits(self.B, self.H, self.Nq, self.Nk, self.d) if dt == F32X and self.ws == "split" else 1


HEAD_SIZES = (8, 24, 32, 40, 48, 56, 64, 72, 80, 96, 104, 128, 160)
SPLIT_SHAPES = (("tail", 130, 64), ("tail", 130, 160), ("empty", 270, 64), ("empty", 520, 40), ("empty", 520, 80), ("cap8", 500, 64),
                ("cap8", 1000, 40))
CASES = (
    # one per instantiation: two query blocks, the second with 2 rows in one wave; a masked tail of 13 keys (f32x d = 40 / 80: of 64)
    [Case("inst_d%d" % d, d, 130, 77, B=2, H=3) for d in HEAD_SIZES]
    # key-count edges: f32x d = 40: second 32-key block of the 64-key tile all masked (65 .. 96) or holding one key (97)
    + [Case("keys_d%d_nk%d" % (d, nk), d, 33, nk) for d in (40, 64) for nk in (1, 31, 32, 33, 64, 65, 96, 97, 128)]
    + [Case("queries_nq%d" % nq, 80, nq, 33) for nq in (1, 32, 33, 128, 129)]
    + [Case("sliced_d%d" % d, d, 77, 77, B=2, H=3, layout="sliced") for d in (40, 80)]
    + [Case("pairs_d%d" % d, d, 33, 77, B=4, H=3, layout="pairs") for d in (40, 160)]
    + [Case("split_%s_d%d_%s" % (nm, d, kind), d, 33, nk, kind=kind, ws="split", dts=(F32X,)) for nm, nk, d in SPLIT_SHAPES
       for kind in ("plain", "late_max", "early_max")]
    + [Case("split_ws_%s" % ws, 64, 33, 270, ws=ws, dts=(F32X,)) for ws in ("small", "misaligned")]
    + [Case("kind_%s_d%d" % (kind, d), d, 33, 97, kind=kind) for kind in KINDS for d in (40, 48, 80, 160)]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CASE_DT = [(c, dt) for c in CASES for dt in ALL3 if dt in c.dts]
CASE_DT_IDS = ["%s-%s" % (c.name, DT_NAME[dt]) for c, dt in CASE_DT]


# ------------------------------------------------------------------------------------------------------------------ inputs
def draw(c, g):
    """fp32 Q [Bq, Nq, H, d], K, V [B, Nk, H, d] of the case's kind.  The kinds that shape the scores do it through channel 0 of every head:
    a constant there in Q against a chosen column in K (both exact in every element type or rounded before the reference sees them)."""
    rn = lambda *s: torch.randn(*s, generator=g)                                          # noqa: E731
    q, k, v = rn(c.Bq, c.Nq, c.H, c.d), rn(c.B, c.Nk, c.H, c.d), rn(c.B, c.Nk, c.H, c.d)
    rd = c.d ** 0.5
    kind = c.kind
    if kind == "offset_v":
        v = v + 100.0
    elif kind == "uniform":
        k = k[:, :1].expand(-1, c.Nk, -1, -1).clone()
    elif kind == "early_max":                            # key 0 leads by 12: the maximum of tile 0 stands from then on
        q[..., 0] = 3.0; k[..., 0] = 0.0; k[:, 0, :, 0] = 4.0 * rd
    elif kind == "late_max":                             # + 0.5 per key on a noise of 0.05: the last valid key leads, the maximum rises every tile
        q[..., 0] = 16.0; k = k * 0.05
        k[..., 0] = (0.5 * rd / 16.0) * torch.arange(c.Nk, dtype=torch.float32)[None, :, None]
    elif kind == "large":                                # scores of sigma 80; row 0 of every (image, head): key Nk / 2 leads by hundreds
        k = k * 80.0
        q[:, 0] = 2.0
        k[:, c.Nk // 2] = 500.0 / rd
    elif kind == "negative":
        q[..., 0] = 16.0; k[..., 0] = -150.0 * rd / 16.0
    else:
        assert kind == "plain", kind
    return q, k, v


class Problem:
    """The inputs of (case, dt): storage tensors on the CPU with the addressing of every operand (what the GPU test uploads), the float64
    reference `ref` [B, Nq, H d], S, T and the per-element `bound`."""

    def __init__(self, case, dt):
        c = self.case = case
        self.dt = dt
        self.pname, self.symbol, self.KT, self.kern, self.ones_row = kernel_of(c.d, dt)
        self.scale = float(torch.tensor(c.d ** -0.5, dtype=torch.float32))
        g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) + 7919 * dt)
        q, k, v = draw(c, g)
        Hd = c.H * c.d
        q, k, v = q.reshape(c.Bq, c.Nq, Hd), k.reshape(c.B, c.Nk, Hd), v.reshape(c.B, c.Nk, Hd)
        # operand -> (storage tensor, first element, row stride, image stride, outer stride), strides in logical elements
        if c.layout == "sliced":
            assert c.Nq == c.Nk and c.Bq == c.B
            ld = 3 * Hd + 8
            x = encode(torch.cat([q, k, v, torch.randn(c.B, c.Nq, 8, generator=g)], -1), dt)
            self.ops = {n: (x, i * Hd, ld, c.Nq * ld, 0) for i, n in enumerate("QKV")}
        else:
            self.ops = dict(Q=(encode(q, dt), 0, Hd, c.Nq * Hd, 0), K=(encode(k, dt), 0, Hd, c.Nk * Hd, c.Bq * c.Nk * Hd),
                            V=(encode(v, dt), 0, Hd, c.Nk * Hd, c.Bq * c.Nk * Hd))
        self._reference()

    def comp(self, name, comp):
        """Operand `name` as [images, rows, H, d] in component 'val' (float64) | 'hi' | 'lo' (fp32; lo scaled by 2^11, f32x only)."""
        s, off = self.ops[name][:2]
        Hd = self.case.H * self.case.d
        return component(s, self.dt, comp)[..., off:off + Hd].reshape(s.shape[0], s.shape[1], self.case.H, self.case.d)

    def _reference(self):
        c, dt = self.case, self.dt
        Q, K, V = (self.comp(n, "val") for n in "QKV")
        ref = torch.empty(c.B, c.Nq, c.H, c.d, dtype=torch.float64)
        S, sub = torch.empty_like(ref), torch.zeros_like(ref)
        T, gap = torch.empty(c.B, c.Nq, c.H, dtype=torch.float64), torch.empty(c.B, c.Nq, c.H, dtype=torch.float64)
        arg = torch.empty(c.B, c.Nq, c.H, dtype=torch.long)
        for b in range(c.B):
            for h in range(c.H):
                q, k, v = Q[b % c.Bq, :, h], K[b, :, h], V[b, :, h]
                s = self.scale * (q @ k.t())
                top = s.topk(min(2, c.Nk), dim=1).values
                e = torch.exp(s - top[:, :1])
                L = e.sum(1, keepdim=True)
                p = e / L
                ref[b, :, h], S[b, :, h] = p @ v, p @ v.abs()
                T[b, :, h] = self.scale * (q.abs() @ k.abs().t()).max(1).values
                sub[b, :, h] = 2.0 ** -25 * v.abs().sum(0)[None, :] / L
                gap[b, :, h] = top[:, 0] - top[:, 1] if c.Nk > 1 else float("inf")
                arg[b, :, h] = s.argmax(1)
        flat = lambda t: t.reshape(c.B, c.Nq, c.H * c.d)                                   # noqa: E731
        self.ref, self.S, self.T = flat(ref), flat(S), T
        Tq = T[..., None].expand(-1, -1, -1, c.d).reshape(c.B, c.Nq, c.H * c.d)
        self.bound = store_term(self.ref, dt) + (U_P[dt] + ARITH + 2 * U_S[dt] * Tq) * self.S + (flat(sub) if dt == F16 else 0.0)
        # the exact rows: one key, or (kind large) a lead of more than 200 -- every other probability underflows to 0
        one_hot = (gap > 200.0) if (c.kind == "large" or c.Nk == 1) else torch.zeros_like(gap, dtype=torch.bool)
        self.exact = one_hot[..., None].expand(-1, -1, -1, c.d).reshape(c.B, c.Nq, c.H * c.d)
        self.exact_val = flat(torch.stack([torch.stack([V[b, arg[b, :, h], h] for h in range(c.H)], 1) for b in range(c.B)]))


@functools.lru_cache(maxsize=4)
def problem(name, dt):
    return Problem(BY_NAME[name], dt)


def check(out, P, what):
    """nn_norm_cases.check with the per-element bound of this module (`check` adds ARITH max|ref| to the store term it is given, so that
    constant is taken off first: what is asserted is exactly P.bound); then the exact rows.  Returns the worst err / bound."""
    worst = nc.check(out, P.ref, P.dt, what, store=P.bound - ARITH * P.ref.abs().max())
    if bool(P.exact.any()):
        err = (out.double() - P.exact_val).abs()[P.exact]
        tol = store_term(P.exact_val, P.dt)[P.exact] if P.dt == F32X else torch.zeros_like(err)
        assert bool((err <= tol).all()), "%s: a one-key / one-hot row is not V[argmax] (worst |err| %.3g)" % (what, float(err.max()))
    return worst


def outside(out, P):
    """Share of the elements of `out` outside the bound (a non-finite element is outside)."""
    return float((~((out.double() - P.ref).abs() <= P.bound)).double().mean())


# ------------------------------------------------------------------------------------------------------------------ guarded output
class GuardedO(Guarded):
    """The output of a case -- image b at (b // Bq) oo + (b % Bq) bo, rows of ldo elements, H d of them written -- as ONE guarded row of
    B bo elements: everything between the rows, between the images and a whole row's worth on either side must keep the sentinel."""

    def __init__(self, c, dt, device):
        span = c.B * c.bo
        super().__init__(1, span, dt, device, ld=span, guard=1)
        b, q, j = torch.meshgrid(torch.arange(c.B), torch.arange(c.Nq), torch.arange(c.H * c.d), indexing="ij")
        self.idx = ((b // c.Bq) * c.oo + (b % c.Bq) * c.bo + q * c.ldo + j).reshape(-1)
        self.shape = (c.B, c.Nq, c.H * c.d)

    def values(self):
        return decode(self.t, self.dt)[0][self.idx].reshape(self.shape)

    def written_mask(self):
        es = nc.ELEM_BYTES[self.dt]
        m = torch.zeros(3, self.ld * es, dtype=torch.bool)
        j = self.idx
        if self.dt == F32X:
            b = (j // 8) * 32 + (j % 8) * 2
            cols = torch.cat([b, b + 1, b + 16, b + 17])
        else:
            cols = (j[:, None] * es + torch.arange(es)[None, :]).reshape(-1)
        m[1, cols] = True
        return m


# ------------------------------------------------------------------------------------------------------------------ fp32 emulations
MUTANTS = ("mask_drop", "mask_admit", "skip_rescale", "l_only", "no_log2e", "ones_next_head", "merge_skip", "merge_unshifted", "empty_w1",
           "empty_stale", "x_drop", "ragged_row")
_f = torch.float32


def _half_rtz(p):
    """fp32 p >= 0 -> the fp16 value v_cvt_pkrtz leaves (toward zero), as fp32."""
    h = p.half()
    bits = h.view(torch.int16) - (h.float() > p).to(torch.int16)
    return bits.view(torch.float16).float()


def _split(x):
    hi = x.half().float()
    return hi, ((x - hi) * 2048.0).half().float()


def _tile(x, k0, KT, repeat_last):
    """rows k0 .. k0 + KT of x, past the end: zeros (the register-staged kernels) or the last row again (k_flash_fwd_x2)."""
    t = x[k0:k0 + KT]
    if t.shape[0] < KT:
        pad = x[-1:].expand(KT - t.shape[0], -1) if repeat_last else x.new_zeros(KT - t.shape[0], x.shape[1])
        t = torch.cat([t, pad])
    return t


def _range(P, q, k, v, vnext, tiles, mutant):
    """One workgroup's walk over `tiles` for one (image, head): q, k, v tuples of components (hi[, lo]) [rows, d], vnext the components of
    the next head's channel 0 [Nk].  -> (unnormalised O [Nq, d], running maximum [Nq], denominator [Nq]), fp32."""
    c, KT, kern = P.case, P.KT, P.kern
    Nq, Nk, d = q[0].shape[0], c.Nk, c.d
    sl = torch.tensor(P.scale, dtype=_f) * (1.0 if mutant == "no_log2e" else torch.tensor(LOG2E, dtype=_f))
    x = len(q) == 2
    if kern == "x2":
        q = _split((q[0] + q[1] * (1.0 / 2048.0)) * sl)                     # the query scaled into the exponent's domain and re-split
    m_run, base = torch.full((Nq,), -3.0e38, dtype=_f), torch.zeros(Nq, dtype=_f)
    acc, acx, l, lx = torch.zeros(Nq, d, dtype=_f), torch.zeros(Nq, d, dtype=_f), torch.zeros(Nq, dtype=_f), torch.zeros(Nq, dtype=_f)
    nvalid = Nk + (mutant == "mask_admit") - (mutant == "mask_drop")
    for t in tiles:
        k0 = t * KT
        kt = [_tile(a, k0, KT, kern == "x2") for a in k]
        vt = [_tile(a, k0, KT, kern == "x2") for a in v]
        vn = [_tile(a[:, None], k0, KT, kern == "x2")[:, 0] for a in vnext]
        s = q[0] @ kt[0].t()
        if x:
            cross = q[0] @ kt[1].t()
            if mutant != "x_drop":
                cross = cross + q[1] @ kt[0].t()
            s = s + cross * (1.0 / 2048.0)
        masked = (k0 + torch.arange(KT)) >= nvalid
        skip = mutant == "skip_rescale" and t == tiles[-1] and t != tiles[0]      # the last tile: what it fails to scale down stays dominant
        if kern == "x2":
            s = s - base[:, None]
            s[:, masked] = -3.0e38
            mx = s.max(1).values
            up = (mx > 0) | (m_run < -1.0e37)
            m = (base + mx).clamp(-60000.0, 60000.0)
            m_new = torch.where(up, (m + m.abs() * 0.001 + 0.001).half().float(), m_run)
            s = s - (m_new - base)[:, None]
            alpha = torch.exp2(m_run - m_new)
            p = torch.exp2(s)
        else:
            s[:, masked] = -3.0e38
            m_new = torch.maximum(m_run, s.max(1).values * sl)
            p = torch.exp2(s * sl - m_new[:, None])
            alpha = torch.exp2(m_run - m_new)
        if not skip:
            l, lx = l * alpha, lx * alpha
            if mutant != "l_only":
                acc, acx = acc * alpha[:, None], acx * alpha[:, None]
        m_run = base = m_new
        if kern == "flash":
            pr = p.to(nc.TORCH_DT[P.dt]).float()
            acc = acc + pr @ vt[0]
            if mutant == "ones_next_head" and P.ones_row:
                l = l + pr @ vn[0]
            else:
                l = l + (pr if P.ones_row else p).sum(1)
        else:
            ph = _half_rtz(p) if kern == "x2" else p.half().float()
            pl = ((p - ph) * 2048.0).half().float()
            acc = acc + ph @ vt[0]
            acx = acx + (ph @ vt[1] + pl @ vt[0])
            if kern == "x":
                l = l + p.sum(1)
            elif mutant == "ones_next_head":
                l, lx = l + ph @ vn[0], lx + (ph @ vn[1] + pl @ vn[0])
            else:
                l, lx = l + ph.sum(1), lx + pl.sum(1)                         # the ones column of V hi, through the same three products
    return acc + acx * (1.0 / 2048.0), m_run, l + lx * (1.0 / 2048.0)


def emulate(P, mutant=None, nsplit=None):
    """An fp32 implementation of the kernel that serves (case, dt) -> float64 of what it stores, [B, Nq, H d].  nsplit: the key ranges
    (default: the case's own)."""
    c, dt = P.case, P.dt
    comps = ("hi", "lo") if dt == F32X else ("hi",)
    Q, K, V = ([P.comp(n, cp) for cp in comps] for n in "QKV")
    sp = c.nsplit(dt) if nsplit is None else nsplit
    ntiles = -(-c.Nk // P.KT)
    tper = -(-ntiles // sp)
    out = torch.empty(c.B, c.Nq, c.H, c.d, dtype=torch.float64)
    for b in range(c.B):
        for h in range(c.H):
            q, k, v = [a[b % c.Bq, :, h] for a in Q], [a[b, :, h] for a in K], [a[b, :, h] for a in V]
            vnext = [a[b, :, (h + 1) % c.H, 0] for a in V]
            parts = [_range(P, q, k, v, vnext, range(min(ntiles, i * tper), min(ntiles, (i + 1) * tper)), mutant) for i in range(sp)]
            if sp == 1:
                o, _, L = parts[0]
            else:
                empty = [min(ntiles, i * tper) >= ntiles for i in range(sp)]
                if mutant == "merge_skip":
                    parts, empty = parts[:1] + parts[2:], empty[:1] + empty[2:]
                m = torch.stack([p_[1] for p_ in parts]).max(0).values
                o, L = torch.zeros(c.Nq, c.d, dtype=_f), torch.zeros(c.Nq, dtype=_f)
                for (oi, mi, li), e in zip(parts, empty):
                    w = torch.exp2(mi - m)
                    if mutant == "merge_unshifted" or (mutant == "empty_w1" and e):
                        w = torch.ones_like(w)
                    if mutant == "empty_stale" and e:
                        oi, li = oi + float("nan"), li + float("nan")
                    L, o = L + w * li, o + w[:, None] * oi
            inv = torch.where(L > 0, 1.0 / L, torch.zeros_like(L))
            out[b, :, h] = nc.round64(o * inv[:, None], dt)
    if mutant == "ragged_row":
        out[:, c.Nq - 1] = float("nan")                                      # the row keeps the sentinel
    return out.reshape(c.B, c.Nq, c.H * c.d)
