"""Shared pieces of the kernel-level parity tests of csrc/gemm.hip (the bf16 + exact-f32 unit, the f16 unit and the split-precision f32x unit
that build from it): the case table -- one case per kernel plan of make_plan -- the inputs, the float64 reference, the per-element bound and
fp32 emulations of a correct kernel and of subtly wrong ones.  Used by test_gemm_plans_gpu.py (the kernels, called alone through the C ABI
between sentinel guards, with the launched profiler symbols asserted) and test_gemm_cases_host.py (the proof, on the CPU, that the bound is
met by a correct fp32 implementation and missed by the mutants).

Storage.  As in nn_norm_cases.py: inputs are drawn in fp32 with a seeded generator, rounded to the element type, and the float64 reference is
computed from the ROUNDED values.  Weights are randn / sqrt(K), activations randn, bias / residual / prior contents of C randn.

Shapes are what make_plan sees.  The f32x entry point doubles K, Cin, cin1 and every operand stride (a 2-byte tensor with two K columns), so
an f32x case passes K / 2, Cin / 2 and cin1 / 2 of the table's numbers and lands on the same plan as the 16-bit types.

The reference is plain torch in float64: matmul, or conv2d with F.interpolate(mode="nearest") for the fused upsample, zero insertion for the
input dilation, F.pad for the (asymmetric) padding and torch.cat for the two-source form; then alpha, bias (per column, per row, or per image
through bias_row_div), activation, residual, and the prior contents of C for `accumulate`.

The bound, per element, never a global maximum:

        |out - ref| <= store(ref) + ARITH (|ref| + L S),    S = |alpha| sum_k |a_ik| |b_jk| + |bias| + |residual| + |prior C|

S is a second float64 product, of the absolute values.  L = 1.2 covers the slope of SiLU / GELU (at most 1.13) and is 1 otherwise.  store(ref)
is nn_norm_cases.store_term for the OUTPUT type, ARITH = 1e-5 the project's bar for fp32-grade arithmetic; no new tolerance.  The GEGLU-pair
case has S = S_hidden |gelu(gate)| + |hidden| S_gate and adds the 6e-7 absolute of dwg_erf_fast (as test_gemm_x_gpu.py does).

Limit of the bound.  An f32x product is hi hi + hi lo + lo hi.  A kernel that drops one cross term is off by about 2^-12 |a| |b| per
product with a random sign, i.e. about 2e-4 sqrt(K) |a| |b| in the sum, against ARITH S = 1e-5 K |a| |b|: the ratio is ~ 30 / sqrt(K) in
logical elements.  The mutant is therefore asserted to fail only at the cases whose K (as make_plan sees it) is <= 1024; at K = 12304 an
error of that size is inside ARITH S and no per-element bound of this form can see it.

Worst err / bound of the kernels over the whole table, measured on an MI355X (parity_gemm.json of test_gemm_plans_gpu.py): bf16 0.98
(conv_upsample), f16 0.92 (reg_scalar), f32 0.018 (f32_wide_batch), f32x 0.010 (wide_batch).  The 16-bit figures are the output store -- a
round-to-nearest bf16 / f16 store alone uses up to all of store(ref); over the cases of those types that write fp32 the worst is 0.010 (bf16,
big256_unsplit) and 0.011 (f16, patch4_wide), so ARITH leaves a factor of ~ 50 on the arithmetic of every plan.
"""
import functools

import torch
import torch.nn.functional as F

from tests.nn_norm_cases import ARITH, DT_NAME, DTYPES, Guarded, decode, encode, store_term  # noqa: F401 (Guarded: for the GPU test)
from tests import nn_norm_cases as nc

F32, BF16, F16, F32X = nc.F32, nc.BF16, nc.F16, nc.F32X
HALF = (BF16, F16, F32X)          # the units that build from the 16-bit kernels (f32x: physical fp16 halves)
HALF16 = (BF16, F16)
ERF_FAST = 6e-7                   # dwg_erf_fast, absolute (dwg_common.h)

SYM_H = {BF16: "k_gemm<bf16>", F16: "k_gemm<f16>"}
G64_0, G64_1, G64_2, G64_3 = ("k_gemm_glds<64, %d, %d>" % (a, s) for a, s in ((0, 3), (1, 2), (2, 3), (3, 3)))
G128_0 = "k_gemm_glds<128, 0, 2>"
G8_256_0, G8_256_2, G8_128_0 = "k_gemm_glds8<256, 128, 0, 3>", "k_gemm_glds8<256, 128, 2, 3>", "k_gemm_glds8<128, 256, 0, 3>"
P4_64, P4_64S, P4_128 = "k_conv3x3_patch2<64, false, 4, 4>", "k_conv3x3_patch2<64, true, 4, 4>", "k_conv3x3_patch2<128, false, 4, 2>"
P8, P8S = "k_conv3x3_patch2<128, false, 8, 4>", "k_conv3x3_patch2<128, true, 8, 4>"
KF32 = "k_gemm<f32>"


class Case:
    """One descriptor of the table.  form: 'nt' C = A[M,K] B[N,K]^T | 'heads' batch (images, heads) addressed in place in [img, rows, heads * K]
    projections | 'wgrad' A and B stored [K, M] / [K, N] (row stride 1) | 'conv' NHWC implicit GEMM.  splitk: ('none', 1) | ('lib', 0) the
    library's choice with the queried workspace | ('ws', n) explicit with a workspace of n slabs | ('atomic', n) explicit without one.
    out / res: 'elem' (the operand type) | 'f32'.  symbol: the profiler symbol it must launch ('H': k_gemm<bf16> / k_gemm<f16>), epilogue:
    whether a splitk_epilogue launch must come with it.  slices / patch_split: the emulation's slice count and whether the slices are 64-channel
    slabs (the patch kernels) rather than k-ranges -- emulation parameters, nothing the GPU test asserts."""

    def __init__(self, name, dts, symbol, M=0, N=0, K=0, form="nt", batch=(1, 1), conv=None, bias=None, act=None, residual=False, alpha=1.0,
                 out="elem", res="elem", ldc=None, splitk=("none", 1), minm=None, plan_m=0, accumulate=False, epilogue=False, rejects=(),
                 slices=1, patch_split=False, tile=(128, 64, 64), pixel_tile=None):
        self.name, self.dts, self.symbol = name, dts, symbol
        self.M, self.N, self.K, self.form, self.batch, self.conv = M, N, K, form, batch, conv
        self.bias, self.act, self.residual, self.alpha, self.accumulate = bias, act, residual, alpha, accumulate
        self.out, self.res, self.ldc = out, res, ldc
        self.splitk, self.minm, self.plan_m, self.epilogue, self.rejects = splitk, minm, plan_m, epilogue, rejects
        self.slices, self.patch_split, self.tile, self.pixel_tile = slices, patch_split, tile, pixel_tile
        if conv is not None:
            cv = dict(stride=1, pad=(1, 1), dil=1, up=1, cin1=0, k=3)
            cv.update(conv)
            Hv, Wv = (cv["H"] * cv["up"] - 1) * cv["dil"] + 1, (cv["W"] * cv["up"] - 1) * cv["dil"] + 1
            if "out" not in cv:
                cv["out"] = ((Hv + 2 * cv["pad"][0] - cv["k"]) // cv["stride"] + 1, (Wv + 2 * cv["pad"][1] - cv["k"]) // cv["stride"] + 1)
            self.conv, self.form = cv, "conv"
            self.M, self.N, self.K = cv["B"] * cv["out"][0] * cv["out"][1], cv["Cout"], cv["k"] * cv["k"] * cv["Cin"]

    def __repr__(self):
        return self.name

    def symbol_of(self, dt):
        return SYM_H[dt] if self.symbol == "H" else self.symbol

    def dims(self, dt):
        """(M, N, K, Cin, cin1) in the LOGICAL elements of `dt` (f32x: half the table's K / Cin / cin1)."""
        h = 2 if dt == F32X else 1
        cv = self.conv or {}
        return self.M, self.N, self.K // h, cv.get("Cin", 0) // h, cv.get("cin1", 0) // h

    @property
    def ncols(self):
        return self.N // 2 if self.act == "geglu_pair" else self.N

    @property
    def ld_c(self):
        return self.ldc if self.ldc is not None else self.ncols + 8

    @property
    def ld_r(self):
        return (self.ncols + 16 + 7) // 8 * 8

    @property
    def rows(self):
        return self.batch[0] * self.batch[1] * self.M

    def out_dt(self, dt):
        return dt if self.out == "elem" else F32

    def res_dt(self, dt):
        return dt if self.res == "elem" else F32


def _conv(B, H, W, Cin, Cout, **kw):
    return dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, **kw)


BAR = dict(bias="col", act="silu", residual=True)          # bias, SiLU, residual
T8_256, T8_128 = (256, 128, 64), (128, 256, 64)
CASES = [
    # ---- 16-bit and f32x: plain rows
    Case("narrow_ktail", HALF, G64_0, 130, 72, 208, **BAR),
    Case("narrow_n70", HALF, G64_0, 130, 70, 208, ldc=72, alpha=0.7, **BAR),
    Case("narrow_n70_f32out", HALF, G64_0, 130, 70, 208, ldc=72, out="f32", **BAR),
    Case("narrow_n70_f32res", HALF, G64_0, 130, 70, 208, ldc=72, out="f32", res="f32", **BAR),
    Case("narrow_rowbias_acc", HALF, G64_0, 130, 72, 208, bias="row", accumulate=True, out="f32", alpha=0.5),
    Case("wide_batch", HALF, G128_0, 130, 136, 80, form="heads", batch=(4, 16), alpha=80 ** -0.5, out="f32", tile=(128, 128, 64)),
    Case("reg_scalar", HALF16, "H", 130, 72, 52, bias="col", act="gelu", residual=True, rejects=(F32X,)),
    Case("reg_rvec_atomic", HALF16, "H", 64, 40, 300, form="wgrad", splitk=("atomic", 3), out="f32", slices=3),
    Case("lib_split_slabs", HALF, G64_0, 130, 200, 8016, splitk=("lib", 0), epilogue=True, out="f32", slices=10, **BAR),
    Case("explicit_slabs_n202", HALF, G64_0, 130, 202, 208, ldc=208, splitk=("ws", 3), epilogue=True, slices=3, **BAR),
    Case("explicit_atomic", HALF, G64_0, 130, 72, 208, splitk=("atomic", 3), out="f32", slices=3),
    Case("big256_split", HALF, G8_256_0, 300, 648, 9232, splitk=("lib", 0), epilogue=True, bias="col", residual=True, slices=18, tile=T8_256),
    Case("big256_unsplit", HALF, G8_256_0, 2049, 2944, 1296, out="f32", res="f32", tile=T8_256, **BAR),
    Case("big256_plan_m", HALF, G8_256_0, 1025, 2944, 1296, plan_m=2049, out="f32", tile=T8_256, **BAR),
    Case("big128x256_split", HALF, G8_128_0, 130, 2056, 12304, splitk=("lib", 0), epilogue=True, slices=14, tile=T8_128, **BAR),
    Case("geglu_tail", HALF, G64_0, 130, 192, 208, bias="col", act="geglu_pair"),
    # ---- 16-bit and f32x: convolutions through the im2col loaders
    Case("conv_generic", HALF, G64_1, conv=_conv(2, 9, 11, 48, 72, stride=2), bias="col", act="silu"),
    # the Downsample form: no top / left pad, one implied row and column of zeros at the bottom and right (F.pad (0, 1, 0, 1) + stride 2)
    Case("conv_asym_pad", HALF, G64_1, conv=_conv(2, 10, 12, 48, 72, stride=2, pad=(0, 0), out=(5, 6)), out="f32", bias="col"),
    Case("conv_in_dilation", HALF, G64_1, conv=_conv(2, 5, 6, 48, 72, pad=(2, 2), dil=2, out=(10, 12)), out="f32"),
    Case("conv_upsample", HALF, G64_1, conv=_conv(2, 9, 11, 48, 72, up=2), bias="col", residual=True),
    Case("conv_fast", HALF, G64_2, conv=_conv(2, 9, 11, 64, 72), **BAR),
    Case("conv_cat_fast", HALF, G64_3, conv=_conv(2, 9, 11, 192, 72, cin1=64), out="f32", res="f32", **BAR),
    Case("conv_cat_generic", HALF, G64_1, conv=_conv(2, 9, 11, 96, 72, cin1=64), bias="col"),
    Case("conv_1x1_rows", HALF, G64_0, conv=_conv(2, 9, 11, 64, 72, k=1, pad=(0, 0)), out="f32", **BAR),
    Case("conv_big256", HALF, G8_256_2, conv=_conv(3, 20, 20, 1024, 768, stride=2), splitk=("lib", 0), epilogue=True, bias="img",
         residual=True, out="f32", slices=18, tile=T8_256),
    # ---- 16-bit and f32x: the LDS-patch kernels
    Case("patch4_ragged", HALF, P4_64, conv=_conv(1, 12, 20, 128, 136), minm=128, bias="img", act="silu", residual=True, pixel_tile=(8, 16)),
    Case("patch4_gelu_rerouted", HALF, G64_2, conv=_conv(1, 12, 20, 128, 136), minm=128, bias="img", act="gelu", residual=True,
         pixel_tile=(8, 16)),
    Case("patch4_split", HALF, P4_64S, conv=_conv(1, 12, 20, 1152, 136), minm=128, splitk=("lib", 0), epilogue=True, bias="img", act="silu",
         residual=True, out="f32", slices=9, patch_split=True, pixel_tile=(8, 16)),
    Case("patch4_wide", HALF, P4_128, conv=_conv(7, 24, 40, 64, 520), minm=128, bias="col", out="f32", pixel_tile=(8, 16), tile=(128, 128, 64)),
    Case("patch8_unsplit", HALF, P8, conv=_conv(2, 32, 32, 64, 3208), bias="col", act="silu", pixel_tile=(16, 16), tile=(256, 128, 64)),
    Case("patch8_split", HALF, P8S, conv=_conv(2, 16, 32, 1536, 776), splitk=("lib", 0), epilogue=True, bias="img", residual=True, slices=8,
         patch_split=True, pixel_tile=(16, 16), tile=(256, 128, 64)),
    # ---- exact f32 (k_gemm<f32>: BK = 16, 4-wide vectors)
    Case("f32_scalar", (F32,), KF32, 130, 70, 50, bias="col", act="leaky_relu", alpha=1.3, tile=(128, 64, 16)),
    Case("f32_kvec_rowbias_acc", (F32,), KF32, 129, 72, 52, bias="row", accumulate=True, tile=(128, 64, 16)),
    Case("f32_wgrad_atomic", (F32,), KF32, 64, 40, 300, form="wgrad", splitk=("atomic", 5), slices=5, tile=(128, 64, 16)),
    Case("f32_slabs", (F32,), KF32, 130, 72, 100, splitk=("ws", 3), epilogue=True, slices=3, tile=(128, 64, 16), **BAR),
    Case("f32_conv_stride2", (F32,), KF32, conv=_conv(2, 9, 11, 4, 10, stride=2), bias="col", tile=(128, 64, 16)),
    Case("f32_conv_in_dilation", (F32,), KF32, conv=_conv(2, 5, 6, 12, 10, pad=(2, 2), dil=2, out=(10, 12)), tile=(128, 64, 16)),
    Case("f32_wide_batch", (F32,), KF32, 130, 136, 20, form="heads", batch=(4, 16), alpha=20 ** -0.5, tile=(128, 128, 16)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CASE_DT = [(c, dt) for c in CASES for dt in DTYPES if dt in c.dts]
CASE_DT_IDS = ["%s-%s" % (c.name, DT_NAME[dt]) for c, dt in CASE_DT]
REJECTED = [(c, dt) for c in CASES for dt in c.rejects]


# ------------------------------------------------------------------------------------------------------------------ storage components
def component(s, dt, comp):
    """A stored operand as 'val' (float64 values), 'hi' (fp32: the values, for f32x the hi half) or 'lo' (f32x: the lo half, scaled by 2^11)."""
    if comp == "val":
        return decode(s, dt)
    if dt != F32X:
        assert comp == "hi"
        return decode(s, dt).float()
    h = s.contiguous().view(torch.float16).view(s.shape[:-1] + (s.shape[-1] // 8, 2, 8)).float()
    return h[..., 0 if comp == "hi" else 1, :].reshape(s.shape)


# ------------------------------------------------------------------------------------------------------------------ im2col (the emulations' A)
def im2col(x, cv, mutant=None):
    """x [B, H, W, Cin] (sources already concatenated) -> [B Ho Wo, KH KW Cin] in the kernels' k order (ky, kx, ci).  Mutants: 'upsample'
    reads the source at y instead of y / 2; 'halo' leaves the pixels past the bottom / right image edge unzeroed (they repeat the edge)."""
    B, H, W, C = x.shape
    k, s, (pt, pl), (Ho, Wo) = cv["k"], cv["stride"], cv["pad"], cv["out"]
    if cv["up"] > 1:
        if mutant == "upsample":
            z = x.new_zeros(B, H * 2, W * 2, C); z[:, :H, :W] = x; x = z
        else:
            x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    if cv["dil"] > 1:
        d = cv["dil"]
        z = x.new_zeros(B, (x.shape[1] - 1) * d + 1, (x.shape[2] - 1) * d + 1, C); z[:, ::d, ::d] = x; x = z
    Hv, Wv = x.shape[1], x.shape[2]
    pb, pr = (Ho - 1) * s + k - Hv - pt, (Wo - 1) * s + k - Wv - pl
    xp = F.pad(x, (0, 0, pl, max(pr, 0), pt, max(pb, 0)))
    if mutant == "halo":
        xp[:, pt + Hv:, :, :] = xp[:, pt + Hv - 1:pt + Hv, :, :]
        xp[:, :, pl + Wv:, :] = xp[:, :, pl + Wv - 1:pl + Wv, :]
    cols = [xp[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s, :] for ky in range(k) for kx in range(k)]
    return torch.stack(cols, 3).reshape(B * Ho * Wo, k * k * C)


def implied_pad(cv):
    """(top, left, bottom, right) zero rows / columns around the virtual (upsampled, dilated) input that the output size implies."""
    k, s, (pt, pl), (Ho, Wo) = cv["k"], cv["stride"], cv["pad"], cv["out"]
    Hv, Wv = (cv["H"] * cv["up"] - 1) * cv["dil"] + 1, (cv["W"] * cv["up"] - 1) * cv["dil"] + 1
    return pt, pl, (Ho - 1) * s + k - Hv - pt, (Wo - 1) * s + k - Wv - pl


def conv_ref(x, w, cv):
    """float64 x [B, H, W, Cin], w [N, KH, KW, Cin] -> [B Ho Wo, N] through F.interpolate / zero insertion / F.pad / conv2d."""
    k, s, (pt, pl), (Ho, Wo) = cv["k"], cv["stride"], cv["pad"], cv["out"]
    x = x.permute(0, 3, 1, 2)
    if cv["up"] > 1:
        x = F.interpolate(x, scale_factor=cv["up"], mode="nearest")
    if cv["dil"] > 1:
        d = cv["dil"]
        z = x.new_zeros(x.shape[0], x.shape[1], (x.shape[2] - 1) * d + 1, (x.shape[3] - 1) * d + 1); z[..., ::d, ::d] = x; x = z
    pb, pr = (Ho - 1) * s + k - x.shape[2] - pt, (Wo - 1) * s + k - x.shape[3] - pl
    y = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w.permute(0, 3, 1, 2).contiguous(), stride=s)
    assert y.shape[2:] == (Ho, Wo), (y.shape, Ho, Wo)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


# ------------------------------------------------------------------------------------------------------------------ a case's inputs and reference
class Problem:
    """The inputs of (case, dt): storage tensors on the CPU (what the GPU test uploads), the float64 reference `ref`, the sensitivity `S`
    and the per-element `bound` [rows, ncols]."""

    def __init__(self, case, dt):
        c = self.case = case
        self.dt = dt
        M, N, K, Cin, cin1 = c.dims(dt)
        self.K = K
        g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) + 7919 * dt)
        rn = lambda *s: torch.randn(*s, generator=g)                                      # noqa: E731
        wscale = K ** -0.5
        if c.form == "nt":
            self.a_s, self.b_s = encode(rn(M, K), dt), encode(rn(N, K) * wscale, dt)
        elif c.form == "heads":
            Bn, Hh = c.batch
            self.a_s, self.b_s = encode(rn(Bn, M, Hh * K), dt), encode(rn(Bn, N, Hh * K), dt)
        elif c.form == "wgrad":
            self.a_s, self.b_s = encode(rn(K, M), dt), encode(rn(K, N), dt)
        else:
            cv = c.conv
            c1 = cin1 if cin1 else Cin
            self.a_s = encode(rn(cv["B"], cv["H"], cv["W"], c1), dt)
            self.a2_s = encode(rn(cv["B"], cv["H"], cv["W"], Cin - c1), dt) if cin1 else None
            self.b_s = encode(rn(N, cv["k"], cv["k"], Cin) * wscale, dt)
        R, nc_ = c.rows, c.ncols
        self.nimg = c.conv["B"] if c.conv else 1
        self.bias_ld = N + 8
        self.bias = {None: None, "col": rn(N), "row": rn(M), "img": rn(self.nimg, self.bias_ld)}[c.bias]
        self.res_s = encode(rn(R, c.ld_r), c.res_dt(dt)) if c.residual else None            # the whole [rows, ldr] buffer, padding included
        self.prior = rn(R, nc_) if c.accumulate else None
        self._reference()

    # -- operands as matrices: [(A [rows_z, K], B [N, K])] per batch entry, in component `comp`
    def mats(self, comp, mutant=None):
        c, dt = self.case, self.dt
        a, b = component(self.a_s, dt, comp), component(self.b_s, dt, comp)
        if c.form == "nt":
            return [(a, b)]
        if c.form == "wgrad":
            return [(a.t(), b.t())]
        if c.form == "heads":
            K = self.K
            return [(a[z1][:, z2 * K:(z2 + 1) * K], b[z1][:, z2 * K:(z2 + 1) * K]) for z1 in range(c.batch[0]) for z2 in range(c.batch[1])]
        return [(im2col(self.sources(comp, mutant), c.conv, mutant), b.reshape(b.shape[0], -1))]

    def sources(self, comp, mutant=None):
        """The NHWC input [B, H, W, Cin] of a conv case (both sources concatenated).  Mutant 'cat': the second source is read at channel ci
        instead of ci - cin1 (its flat buffer indexed cin1 elements too far; the last pixel's overrun reads zeros)."""
        x = component(self.a_s, self.dt, comp)
        if self.a2_s is None:
            return x
        x2 = component(self.a2_s, self.dt, comp)
        if mutant == "cat":
            flat = torch.cat([x2.reshape(-1), x2.new_zeros(x.shape[-1])])
            x2 = flat[x.shape[-1]:].reshape(x2.shape)
        return torch.cat([x, x2], -1)

    def residual(self, mutant=None):
        """float64 [rows, ncols].  Mutant 'res_ld': read with a leading dimension of ncols instead of ldr."""
        c = self.case
        full = decode(self.res_s, c.res_dt(self.dt))
        if mutant == "res_ld":
            return full.reshape(-1)[:c.rows * c.ncols].reshape(c.rows, c.ncols)
        return full[:, :c.ncols]

    def bias_rows(self, R, mutant=None):
        """The bias as something that broadcasts against [R, N] (fp32 values)."""
        c, b = self.case, self.bias
        if c.bias == "col":
            if mutant == "bias_group":          # the last group of four columns takes the previous group's values
                b = b.clone(); g0 = (c.N - 1) // 4 * 4; b[g0:] = self.bias[g0 - 4:g0 - 4 + c.N - g0]
            return b[None, :]
        if c.bias == "row":
            return b.repeat(R // c.M)[:, None]
        img = torch.arange(R) // (c.conv["out"][0] * c.conv["out"][1])
        if mutant == "img_off":
            img = (img + 1) % self.nimg
        return b[img][:, :c.N]

    def _reference(self):
        c, dt = self.case, self.dt
        if c.form == "conv":
            x, w = self.sources("val"), decode(self.b_s, dt)
            prod, aprod = conv_ref(x, w, c.conv), conv_ref(x.abs(), w.abs(), c.conv)
        else:
            ms = self.mats("val")
            prod = torch.cat([a @ b.t() for a, b in ms]); aprod = torch.cat([a.abs() @ b.abs().t() for a, b in ms])
        R = prod.shape[0]
        assert R == c.rows and prod.shape[1] == c.N
        v, S = c.alpha * prod, abs(c.alpha) * aprod
        if c.bias:
            bb = self.bias_rows(R).double(); v = v + bb; S = S + bb.abs()
        L, extra = 1.0, 0.0
        if c.act == "geglu_pair":
            hv, hs = v.view(R, -1, 2, 32), S.view(R, -1, 2, 32)
            gate = F.gelu(hv[:, :, 1])
            v = (hv[:, :, 0] * gate).reshape(R, -1)
            S = (hs[:, :, 0] * gate.abs() + hv[:, :, 0].abs() * hs[:, :, 1]).reshape(R, -1)
            L, extra = 1.2, ERF_FAST
        elif c.act is not None:
            v = {"silu": F.silu, "gelu": F.gelu, "leaky_relu": lambda t: F.leaky_relu(t, 0.01), "relu": F.relu, "sigmoid": torch.sigmoid}[c.act](v)
            L = 1.2 if c.act in ("silu", "gelu") else 1.0
        if c.residual:
            r = self.residual(); v = v + r; S = S + r.abs()
        if c.accumulate:
            v = v + self.prior.double(); S = S + self.prior.double().abs()
        self.ref, self.S = v, S
        self.bound = store_term(v, c.out_dt(dt)) + ARITH * (v.abs() + L * S) + extra


@functools.lru_cache(maxsize=2)
def problem(name, dt):
    return Problem(BY_NAME[name], dt)


def check(out, P, what):
    """nn_norm_cases.check with the per-element bound of this module: `check` adds ARITH max|ref| to the store term it is given, so that
    constant is taken off first and what is asserted is exactly P.bound.  Returns the worst err / bound."""
    return nc.check(out, P.ref, P.case.out_dt(P.dt), what, store=P.bound - ARITH * P.ref.abs().max())


def outside(out, P):
    """Share of the elements of `out` outside the bound."""
    return float(((out.double() - P.ref).abs() > P.bound).double().mean())


# ------------------------------------------------------------------------------------------------------------------ fp32 emulations
KSTEP = {BF16: 64, F16: 64, F32X: 32, F32: 16}       # the kernels' k-step in logical elements: 64 halves (32 f32x elements), 16 floats


def kstep(P):
    return KSTEP[P.dt]


def slice_ranges(P):
    """The k-ranges (in logical elements) of the case's slices, by the kernels' rule: ceil(K / slices) rounded up to whole k-steps."""
    n, bk, K = P.case.slices, kstep(P), P.K
    per = ((K + n - 1) // n + bk - 1) // bk * bk
    return [(min(K, i * per), min(K, (i + 1) * per)) for i in range(n)]


def _partial(As, Bs, sel, mutant):
    """fp32 product over the k-selection `sel` (a slice, or an index tensor): (main, cross / 2^11 still to apply).  f32x: hi hi, and the two
    cross products hi lo + lo hi summed in fp32 (mutant 'x_drop': lo hi missing)."""
    ah, bh = As[0][:, sel], Bs[0][:, sel]
    main = ah @ bh.t()
    if len(As) == 1:
        return main, None
    al, bl = As[1][:, sel], Bs[1][:, sel]
    cross = ah @ bl.t()
    if mutant != "x_drop":
        cross = cross + al @ bh.t()
    return main, cross


def _combine(main, cross):
    return main if cross is None else main + cross * (1.0 / 2048.0)


def _accumulate(As, Bs, order, P, mutant):
    c, K, bk = P.case, P.K, kstep(P)
    if mutant == "ktail":
        assert K % bk, "no k tail to drop"
        K = K - K % bk
    if order == "whole":
        return _combine(*_partial(As, Bs, slice(0, K), mutant))
    if order == "ksteps":
        main = cross = None
        for k0 in range(0, K, bk):
            m, x = _partial(As, Bs, slice(k0, min(K, k0 + bk)), mutant)
            main = m if main is None else main + m
            cross = x if cross is None or x is None else cross + x
        return _combine(main, cross)
    assert order == "slices"
    if c.patch_split:                       # slices of whole 64-channel slabs (physical halves), every tap of them
        Cin = P.case.dims(P.dt)[3]
        slab = 32 if P.dt == F32X else 64
        ncc, n = Cin // slab, c.slices
        per = (ncc + n - 1) // n
        kidx = torch.arange(9 * Cin).view(9, Cin)
        sels = [kidx[:, i * per * slab:min(ncc, (i + 1) * per) * slab].reshape(-1) for i in range(n)]
        sels = [s for s in sels if s.numel()]
    else:
        sels = [slice(a, b) for a, b in slice_ranges(P) if b > a]
    if mutant == "last_slice":
        sels = sels[:-1]
    acc = None
    for s in sels:
        v = _combine(*_partial(As, Bs, s, mutant))
        acc = v if acc is None else acc + v
    return acc


def emulate(P, order="whole", mutant=None, store=True):
    """An fp32 implementation of the case -> float64 of what it stores [rows, ncols] (store=False: of the fp32 value it is about to store).
    order: 'whole' | 'ksteps' | 'slices'.  mutant: None, or one of ktail, last_slice, bias_group, res_ld, alpha_after, img_off, halo, upsample,
    cat, x_drop."""
    c, dt = P.case, P.dt
    comps = ("hi", "lo") if dt == F32X else ("hi",)
    per_comp = [P.mats(cp, mutant) for cp in comps]
    acc = torch.cat([_accumulate([m[z][0] for m in per_comp], [m[z][1] for m in per_comp], order, P, mutant) for z in range(len(per_comp[0]))])
    R = acc.shape[0]
    alpha = torch.tensor(c.alpha, dtype=torch.float32)
    bias = P.bias_rows(R, mutant) if c.bias else None
    if mutant == "alpha_after":
        v = (acc + bias) * alpha
    else:
        v = acc * alpha
        if bias is not None:
            v = v + bias
    if c.act == "geglu_pair":
        h = v.view(R, -1, 2, 32)
        v = (h[:, :, 0] * (0.5 * h[:, :, 1] * (1.0 + torch.erf(h[:, :, 1] * 0.70710678118654752)))).reshape(R, -1)
    elif c.act == "silu":
        v = v / (1.0 + torch.exp(-v))
    elif c.act == "gelu":
        v = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
    elif c.act == "leaky_relu":
        v = torch.where(v > 0, v, 0.01 * v)
    elif c.act is not None:
        raise NotImplementedError(c.act)
    if c.residual:
        v = v + P.residual(mutant).float()
    if c.accumulate:
        v = v + P.prior
    return stored(P, v) if store else v.double()


def stored(P, v):
    """What the output store of the case leaves of the fp32 values v, as float64."""
    od = P.case.out_dt(P.dt)
    return v.double() if od == F32 else nc.round64(v.float(), od)


# ------------------------------------------------------------------------------------------------------------------ the descriptor
def desc_args(c, dt):
    """The keyword arguments of gemm.gemm_raw for (case, dt), tensors and workspace excepted.  Strides in logical elements."""
    M, N, K, Cin, cin1 = c.dims(dt)
    kw = dict(M=M, N=N, K=K, ldc=c.ld_c, ldr=c.ld_r if c.residual else 0, act=c.act, alpha=c.alpha, bias_per_row=c.bias == "row",
              accumulate=c.accumulate, plan_m=c.plan_m, splitk={"none": 1, "lib": 0}.get(c.splitk[0], c.splitk[1]))
    if c.form == "nt":
        kw.update(a_strides=(K, 1), b_strides=(K, 1))
    elif c.form == "wgrad":
        kw.update(a_strides=(1, M), b_strides=(1, N))
    elif c.form == "heads":
        Bn, Hh = c.batch
        kw.update(a_strides=(Hh * K, 1), b_strides=(Hh * K, 1), batch=c.batch, a_batch=(M * Hh * K, K), b_batch=(N * Hh * K, K),
                  c_batch=(Hh * M * c.ld_c, M * c.ld_c))
    else:
        cv = c.conv
        kw.update(a_strides=(0, 1), b_strides=(K, 1), conv_upsample=cv["up"], cin1=cin1,
                  conv=(Cin, cv["H"], cv["W"], cv["out"][0], cv["out"][1], cv["k"], cv["k"], cv["stride"], cv["pad"][0], cv["pad"][1], cv["dil"]))
    if c.bias == "img":
        kw.update(bias_row_div=c.conv["out"][0] * c.conv["out"][1], bias_ld=N + 8)
    return kw


def operand_bytes(c, dt):
    """Bytes of every buffer of (case, dt): A (both sources), B, C with its leading dimension, residual, slab workspace."""
    M, N, K, Cin, cin1 = c.dims(dt)
    es = nc.ELEM_BYTES[dt]
    nb = c.batch[0] * c.batch[1]
    a = c.conv["B"] * c.conv["H"] * c.conv["W"] * Cin * es if c.conv else nb * M * K * es
    return dict(A=a, B=nb * N * K * es if c.form == "heads" else N * K * es, C=c.rows * c.ld_c * nc.ELEM_BYTES[c.out_dt(dt)],
                R=c.rows * c.ld_r * nc.ELEM_BYTES[c.res_dt(dt)] if c.residual else 0,
                W=c.slices * max(M, c.plan_m) * N * 4 if c.splitk[0] in ("lib", "ws") else 0)    # (library split: at least; the query test has the rest)
