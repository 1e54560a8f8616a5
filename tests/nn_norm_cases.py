"""Shared pieces of the kernel-level parity tests of csrc/nn_norm.hip (GroupNorm forward / input gradient, LayerNorm, GEGLU, row softmax
forward / backward) in all four element types: storage helpers, float64 references, the per-element bound, guarded outputs, the shape tables.
Used by test_nn_norm_dtypes_gpu.py (the kernels) and test_nn_norm_cases_host.py (fp32 emulations of the kernels' formulas: the proof that
the bound is met by a correct implementation and missed by subtly wrong ones).

Storage.  Inputs are drawn in fp32, rounded to the element type (`encode`), and the float64 reference is computed from the ROUNDED values
(`decode`), so what is left is the kernel's arithmetic and its output store.  F32X goes through xfmt.pack; its float64 value is hi + lo 2^-11
exactly.

The bound, per element, never a ratio (softmax backward with n = 1 has ref == 0 and must give 0 <= 0):

        |out - ref| <= store(ref) + 1e-5 max|ref|

store(ref) is the unit roundoff of the element type: bf16 2^-8 |ref|, f16 2^-11 max(|ref|, 2^-14), f32 2^-24 |ref|, f32x 5e-7 max(|ref|, 1e-4)
(the figure test_gemm_x_gpu.py asserts for the format).  1e-5 of the output scale is the project's bar for fp32-grade arithmetic (TOL of
test_gemm_x_gpu.py, the f32 cases of test_gemm_gpu.py); it covers the fp32 statistics, __expf, rsqrtf and dwg_erf_fast (6e-7 absolute).
The sum is rigorous: a value within d of ref before the store is within u |ref| + (1 + u) d after it.

GroupNorm backward with `residual` stores TWICE: the kernel rounds dx to the element type, adds the residual to that rounded value and rounds
again.  Its store term is therefore store(dx_ref) + store(dx_ref + residual).  (An observation for a later change -- one rounding would do.)

Saved statistics stats[b][g] = (sum x, sum x^2): |stats - ref| <= 1e-5 sum|x| and <= 1e-5 sum x^2, in every element type (they are fp32 even
when the tensor is bf16).

Limit of the bound.  The kernels form the variance as E[x^2] - m^2 in fp32, whose error grows with m^2 / var.  Emulated in fp32 on the CPU
(test_nn_norm_cases_host.py), the forward case with mean = 4 sigma and the backward case with mean = 2 sigma, both at
(B, HW, C, G) = (1, 100, 512, 32), use 0.15 of the f32 bound when the two sums are exactly rounded and up to 0.6 with fp32 sums that are
themselves 4e-7 off, and are asserted; at 8 sigma forward, or at 2 sigma backward with 50 000 elements per group, the FORMULA no longer
meets the bound.  Those are not asserted anywhere: it is the known limit of the one-pass variance, not a defect of a kernel.  (The kernels
themselves, measured on an MI355X: 0.33 of the f32 bound at 4 sigma forward, 0.08 at 2 sigma backward.)
"""
import functools

import torch
import torch.nn.functional as F

F32, BF16, F16, F32X = 0, 1, 2, 3                      # DWG_DTYPE_* (include/dwg_types.h)
DTYPES = [BF16, F16, F32, F32X]
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16", F32X: "f32x"}
DT_IDS = [DT_NAME[d] for d in DTYPES]
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16, F32X: torch.int32}
ELEM_BYTES = {F32: 4, BF16: 2, F16: 2, F32X: 4}
ARITH = 1e-5                                           # fp32-grade arithmetic, relative to the output scale
SENTINEL_BYTE = 0x5A                                   # every guard byte; as bf16 / f32 1.5e16, as f16 (and both f32x halves) 203.25


# ------------------------------------------------------------------------------------------------------------------ storage
def encode(x, dt):
    """fp32 CPU tensor [..., n] -> CPU tensor in the storage type of `dt` (f32x: int32 words, the last dimension padded to whole groups
    of 8 and sliced back, so callers may pass any n as long as THEY keep rows on group boundaries)."""
    x = x.float()
    if dt != F32X:
        return x.to(TORCH_DT[dt]).contiguous()
    from dreamwaltz_g_amd import xfmt
    n = x.shape[-1]
    if n % 8:
        x = F.pad(x, (0, 8 - n % 8))
    return xfmt.pack(x)


def decode(t, dt):
    """stored tensor (any device) -> the values it holds, float64 on the CPU.  f32x: [..., n] int32 with n % 8 == 0."""
    t = t.detach().cpu().contiguous()
    if dt != F32X:
        return t.double()
    h = t.view(torch.float16).view(t.shape[:-1] + (t.shape[-1] // 8, 2, 8)).double()
    return (h[..., 0, :] + h[..., 1, :] / 2048.0).reshape(t.shape)


def rounded(x, dt):
    """fp32 CPU tensor -> (storage tensor on the CPU, float64 values it holds), sliced back to x's last dimension."""
    s = encode(x, dt)
    return s, decode(s, dt)[..., :x.shape[-1]]


def round64(x, dt):
    """What a store of the fp32 values x to element type `dt` leaves, as float64 (the output rounding of the host emulations)."""
    return rounded(x, dt)[1]


# ------------------------------------------------------------------------------------------------------------------ the bound
def store_term(ref, dt):
    a = ref.abs()
    if dt == BF16:
        return a * 2.0 ** -8
    if dt == F16:
        return a.clamp_min(2.0 ** -14) * 2.0 ** -11
    if dt == F32:
        return a * 2.0 ** -24
    return a.clamp_min(1e-4) * 5e-7


def check(out, ref, dt, what, store=None):
    """Asserts |out - ref| <= store + 1e-5 max|ref| on every element; returns the worst err / bound (0 / 0 counts as 0) for the report."""
    out, ref = out.double(), ref.double()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert bool(torch.isfinite(out).all()), (what, "non-finite output")
    err = (out - ref).abs()
    bound = (store_term(ref, dt) if store is None else store) + ARITH * ref.abs().max()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    ok = err <= bound
    if not bool(ok.all()):
        i = int(ratio.argmax())
        raise AssertionError("%s [%s]: %d of %d elements outside the bound; worst err/bound %.3g at flat index %d (out %.9g, ref %.9g, bound %.3g)"
                             % (what, DT_NAME[dt], int((~ok).sum()), ok.numel(), worst, i, float(out.reshape(-1)[i]),
                                float(ref.reshape(-1)[i]), float(bound.reshape(-1)[i])))
    return worst


def passes(out, ref, dt, store=None):
    try:
        check(out, ref, dt, "probe", store)
    except AssertionError:
        return False
    return True


def check_stats(stats, ref_stats, ref_abs, what):
    """stats / ref_stats [B, G, 2] = (sum x, sum x^2); ref_abs [B, G] = sum |x|.  Returns the worst error relative to its bound."""
    stats, ref_stats = stats.double().cpu(), ref_stats.double()
    assert stats.shape == ref_stats.shape, (what, stats.shape, ref_stats.shape)
    e1 = (stats[..., 0] - ref_stats[..., 0]).abs(); b1 = ARITH * ref_abs
    e2 = (stats[..., 1] - ref_stats[..., 1]).abs(); b2 = ARITH * ref_stats[..., 1]
    worst = max(float((e1 / b1).max()), float((e2 / b2).max()))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), (what, "saved statistics, worst err/bound", worst)
    return worst


# ------------------------------------------------------------------------------------------------------------------ references (float64)
def gn_ref(x, gamma, beta, G, eps, silu):
    """x [B, HW, C] float64 (the rounded input) -> y [B, HW, C], leaf for gn_bwd_ref."""
    xd = x.clone().requires_grad_(True)
    y = F.group_norm(xd.permute(0, 2, 1), G, gamma.double(), beta.double(), eps)
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1), xd


def gn_bwd_ref(y, xd, dy):
    (gx,) = torch.autograd.grad(y, xd, dy, retain_graph=True)
    return gx


def gn_stats_ref(x, G):
    """-> stats [B, G, 2] = (sum x, sum x^2) and sum |x| [B, G], float64."""
    B, HW, C = x.shape
    xg = x.view(B, HW, G, C // G)
    return torch.stack([xg.sum((1, 3)), (xg * xg).sum((1, 3))], -1), xg.abs().sum((1, 3))


def ln_ref(x, gamma, beta, eps):
    return F.layer_norm(x, (x.shape[-1],), gamma.double(), beta.double(), eps)


def geglu_ref(h):
    a, b = h.chunk(2, dim=-1)
    return a * F.gelu(b)


def softmax_ref(S, scale):
    return torch.softmax(S.double() * scale, -1)


def softmax_bwd_ref(P, dP, scale):
    """On the STORED probabilities P (float64 of what the forward left)."""
    dP = dP.double()
    return scale * P * (dP - (P * dP).sum(-1, keepdim=True))


# ------------------------------------------------------------------------------------------------------------------ draws (cached, read-only)
@functools.lru_cache(maxsize=4)
def gn_draw(B, HW, C, G, offset=0.3, spread=1.5):
    """fp32 x, dy, residual [B, HW, C]; gamma, beta [C].  The same numbers for every element type and flag of a shape."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * HW + 7 * C + G)
    x = torch.randn(B, HW, C, generator=g) * spread + offset
    gamma = torch.randn(C, generator=g) * 0.5 + 1.0
    beta = torch.randn(C, generator=g) * 0.2
    dy = torch.randn(B, HW, C, generator=g)
    res = torch.randn(B, HW, C, generator=g)
    return x, gamma, beta, dy, res


@functools.lru_cache(maxsize=2)
def ln_draw(M, C):
    """Row 0 is scaled to a variance of 1.6e-5, where eps = 1e-5 matters (a dropped eps shows in every element type)."""
    g = torch.Generator().manual_seed(31 * M + C)
    x = torch.randn(M, C, generator=g) * 2 + 0.5
    x[0] *= 2e-3
    return x, torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.1


@functools.lru_cache(maxsize=1)
def geglu_draw(M, Fd):
    """[M, 2 F]: values ~ randn, gates ~ 2 randn (both erf tails and the region around 0)."""
    g = torch.Generator().manual_seed(17 * M + Fd)
    h = torch.randn(M, 2 * Fd, generator=g)
    h[:, Fd:] *= 2
    return h


@functools.lru_cache(maxsize=2)
def softmax_draw(rows, n, dominant=True):
    """S, dP fp32 [rows, n].  dominant: row 0 holds a dominating score (S[0, 0] = 400), every other term of that row underflows.  With a
    single row that leaves nothing else to look at, so the one-row cases run a second time on an ordinary row (SOFTMAX_CASES)."""
    g = torch.Generator().manual_seed(101 * rows + n)
    S = torch.randn(rows, n, generator=g) * 3
    if dominant:
        S[0, 0] = 400.0
    return S, torch.randn(rows, n, generator=g)


SOFTMAX_SCALE = 0.158


def softmax_ld(n):
    """Row stride of the strided softmax operands: a multiple of 8, at least n + 8."""
    return (n + 8 + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------------------------ guarded outputs
class Guarded:
    """An output of `rows` x `n` elements of type `dt` with row stride `ld` inside a larger allocation filled with SENTINEL_BYTE: `guard`
    whole rows before and after, and the columns n .. ld-1 of every row (for f32x with n % 8 != 0 also the unused lanes of the last group's hi
    and lo halves).  `intact()` is true when every byte the kernel had no business writing still holds the sentinel -- a write outside the
    row shows without ever leaving the allocation."""

    def __init__(self, rows, n, dt, device, ld=None, guard=2):
        self.rows, self.n, self.dt, self.ld, self.guard = rows, n, dt, (n if ld is None else ld), guard
        assert self.ld >= n and (dt != F32X or self.ld % 8 == 0)
        es = ELEM_BYTES[dt]
        self.raw = torch.full(((rows + 2 * guard) * self.ld * es,), SENTINEL_BYTE, dtype=torch.uint8, device=device)
        self.t = self.raw.view(TORCH_DT[dt]).view(rows + 2 * guard, self.ld)[guard:guard + rows]      # what the kernel is given
        assert self.t.data_ptr() % 16 == 0

    def values(self):
        """float64 [rows, n] on the CPU."""
        return decode(self.t, self.dt)[:, :self.n]

    def written_mask(self):
        """bool [rows + 2 guard, ld * elem bytes]: the bytes that belong to the rows x n output."""
        es = ELEM_BYTES[self.dt]
        m = torch.zeros(self.rows + 2 * self.guard, self.ld * es, dtype=torch.bool)
        j = torch.arange(self.n)
        if self.dt == F32X:
            b = (j // 8) * 32 + (j % 8) * 2                    # dwg_x_byte: the hi half; the lo half 16 bytes on
            cols = torch.cat([b, b + 1, b + 16, b + 17])
        else:
            cols = (j[:, None] * es + torch.arange(es)[None, :]).reshape(-1)
        m[self.guard:self.guard + self.rows, cols] = True
        return m

    def intact(self):
        raw = self.raw.cpu().view(self.rows + 2 * self.guard, -1)
        return bool((raw[~self.written_mask()] == SENTINEL_BYTE).all())


# ------------------------------------------------------------------------------------------------------------------ shape tables
SMALL = ("gn_small",)
FOLDED = ("gn_stats", "gn_apply")
FINAL = ("gn_stats", "gn_finalize", "gn_apply")
# (B, HW, C, G), the launches the forward must make -- why each shape is here: see the table in test_nn_norm_dtypes_gpu.py
GN_FWD = [
    ((1, 64, 320, 32), SMALL),
    ((2, 1024, 640, 32), SMALL),
    ((1, 9, 96, 32), SMALL),
    ((1, 50, 32, 32), SMALL),
    ((1, 96, 512, 1), SMALL),
    ((4, 1024, 256, 32), SMALL),
    ((5, 64, 320, 32), FOLDED),
    ((5, 100, 512, 32), FOLDED),
    ((1, 1681, 320, 32), FINAL),
    ((5, 64, 512, 64), FINAL),
    ((1, 625, 2560, 32), FINAL),
    ((5, 16, 4096, 32), FOLDED),
    ((1, 1025, 64, 32), FOLDED),
]
GN_EPS = {s: (1e-5, 1e-6)[i % 2] for i, (s, _) in enumerate(GN_FWD)}
# backward: always the three-launch path; gn_finalize exactly where the forward table shows it (and never for the one gn_small shape: 2 partials)
GN_BWD = [(s, ("gn_bwd_stats",) + (("gn_finalize",) if "gn_finalize" in l else ()) + ("gn_bwd_apply",)) for s, l in GN_FWD[6:]]
GN_BWD.append(((1, 64, 320, 32), ("gn_bwd_stats", "gn_bwd_apply")))
GN_OFFSET_SHAPE = (1, 100, 512, 32)                    # mean = 4 sigma forward (x = 1.5 randn + 6), 2 sigma backward (+ 3)
GN_LOWVAR_SHAPE = (1, 64, 320, 32)                     # x = 2e-3 randn: variance 4e-6 next to eps = 1e-5, so that eps itself is checked
LN_SHAPES = [(1, 8), (5, 320), (4, 520), (7, 2048)]
GEGLU_SHAPES = [(1, 8), (5, 1280), (4100, 2048)]
SOFTMAX_ROWS = [1, 5]
SOFTMAX_CASES = [(1, True), (5, True), (1, False)]     # (rows, row 0 dominated by one score)
SOFTMAX_N = [1, 63, 64, 65, 77, 4096, 8200]


def gn_inputs(shape, dt, kind="plain"):
    """-> dict of the fp32 draws of a GroupNorm case rounded to `dt`: storage tensors (x_s, dy_s, res_s) and float64 values (x, dy, res),
    fp32 gamma / beta.  kind: 'plain' 1.5 randn + 0.3, 'fwd4s' + 6.0, 'bwd2s' + 3.0, 'lowvar' 2e-3 randn."""
    off, spread = {"plain": (0.3, 1.5), "fwd4s": (6.0, 1.5), "bwd2s": (3.0, 1.5), "lowvar": (0.0, 2e-3)}[kind]
    x, gamma, beta, dy, res = gn_draw(*shape, offset=off, spread=spread)
    d = dict(gamma=gamma, beta=beta)
    for k, v in (("x", x), ("dy", dy), ("res", res)):
        d[k + "_s"], d[k] = rounded(v, dt)
    return d
