"""MI355X-native learned background of the NeRF stage (boundary B22, bg_mode 'nerf'): frequency encoding of the ray direction ->
bg_net -> sigmoid / identity in one kernel, on csrc/nerf_background.hip through include/dwg_nerf_background.h.

  freq_encode(x, degree)             the reference FreqEncoder's forward (core/nerf/freqencoder/freq.py): [..., 3] -> [..., 3 + 6 degree]
  FreqEncoder(input_dim, degree)     the module with the reference's attributes; no parameters
  learned_background(rays_d, encoder_bg, bg_net, sigmoid, precision)
                                     what _NeRFNetwork.background computes for 'nerf' (core/nerf/nerf_model.py:134-139): [N, C], one
                                     autograd function, one launch forward and two backward, gradients for bg_net's weights and biases
  unsupported_reason(encoder_bg, bg_net)   None when the kernels take this pair, else why not

The encoding is sin / cos proper of the exactly scaled input (the reference's kernel takes a fast-intrinsic sine of x + phase: not
restated).  Precision follows autocast as nerf.nerf_field does.  No CPU fallback; every tensor is checked (CUDA, fp32, shape, contiguity,
one device) and a violation raises RuntimeError before any launch.
"""
import ctypes

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from . import nerf

MAX_DEGREE, MAX_LAYERS = _lib.CONSTANTS["DWG_NERF_BG_MAX_DEGREE"], _lib.CONSTANTS["DWG_NERF_BG_MAX_LAYERS"]
HIDDEN, OUT_DIMS = (16, 32, 64), (3, 4)


def _check_dirs(name, x):
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise RuntimeError("%s must not require grad: the frequency encoding is not differentiated (encoder_bg has no parameters)" % name)
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.shape[-1] != 3:
        raise RuntimeError("%s must be a tensor [..., 3]" % name)
    _lib.check_tensor(name, x)
    if x.numel() // 3 >= 1 << 31:
        raise RuntimeError("%s holds %d directions: fewer than 2^31" % (name, x.numel() // 3))


def _check_degree(degree):
    if not isinstance(degree, int) or isinstance(degree, bool) or not 1 <= degree <= MAX_DEGREE:
        raise RuntimeError("the frequency encoding takes degree 1..%d, got %r" % (MAX_DEGREE, degree))


def freq_encode(x, degree=6):
    """x [..., 3] fp32 on the device -> [..., 3 + 6 degree]: column c < 3 is x[c]; c = 3 + (2 f + s) * 3 + d is sin(2^f x[d]) for s = 0 and
    cos(2^f x[d]) for s = 1.  Not differentiable."""
    _check_degree(degree)
    _check_dirs("x", x)
    N = x.numel() // 3
    out = torch.empty(tuple(x.shape[:-1]) + (3 + 6 * degree,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().dwg_nerf_freq_encode(N, _lib.ptr(x), degree, _lib.ptr(out), _lib.stream(x)), "dwg_nerf_freq_encode")
    return out


class FreqEncoder(nn.Module):
    """core/nerf/freqencoder/freq.py:60-82: input_dim, degree, output_dim; no parameters."""

    def __init__(self, input_dim=3, degree=6):
        super().__init__()
        if input_dim != 3:
            raise NotImplementedError("FreqEncoder input_dim %r is not built natively (3: a direction)" % (input_dim,))
        self.input_dim = input_dim
        self.degree = degree
        self.output_dim = input_dim + input_dim * 2 * degree

    def __repr__(self):
        return f"FreqEncoder: input_dim={self.input_dim} degree={self.degree} output_dim={self.output_dim}"

    def forward(self, inputs, **kwargs):
        return freq_encode(inputs, self.degree)


def unsupported_reason(encoder_bg, bg_net, device=None):
    """None when learned_background takes this encoder and network (device: where the parameters must live), else why not."""
    if encoder_bg is None or getattr(encoder_bg, "input_dim", None) != 3:
        return "encoder_bg is not a frequency encoder of 3 inputs"
    degree = getattr(encoder_bg, "degree", None)
    if not isinstance(degree, int) or isinstance(degree, bool) or not 1 <= degree <= MAX_DEGREE:
        return "encoder_bg degree %r (the kernels take 1..%d)" % (degree, MAX_DEGREE)
    if getattr(encoder_bg, "output_dim", 3 + 6 * degree) != 3 + 6 * degree:
        return "encoder_bg output_dim %r is not 3 + 6 degree" % (encoder_bg.output_dim,)
    net = getattr(bg_net, "net", None)
    try:
        lins = list(net) if net is not None else None
    except TypeError:
        lins = None
    if not lins or not 1 <= len(lins) <= MAX_LAYERS:
        return "bg_net with %s layers (the kernels take 1..%d)" % (None if not lins else len(lins), MAX_LAYERS)
    if any(not isinstance(l, nn.Linear) or l.bias is None for l in lins):
        return "bg_net layers are not biased nn.Linear"
    if lins[-1].out_features not in OUT_DIMS:
        return "bg_net output width %d (the kernels take 3 or 4)" % lins[-1].out_features
    if len(lins) > 1 and lins[0].out_features not in HIDDEN:
        return "bg_net hidden width %d (the kernels take 16, 32 or 64)" % lins[0].out_features
    for l, lin in enumerate(lins):
        k = 3 + 6 * degree if l == 0 else lins[0].out_features
        n = lins[-1].out_features if l == len(lins) - 1 else lins[0].out_features
        if (lin.in_features, lin.out_features) != (k, n):
            return "bg_net.net[%d] is %d -> %d, expected %d -> %d" % (l, lin.in_features, lin.out_features, k, n)
        if device is not None and (lin.weight.device != device or lin.bias.device != device):
            return "bg_net.net[%d] is not on %s" % (l, device)
    return None


class _Spec:
    """Everything of the background that is not a tensor autograd differentiates."""

    def __init__(self, degree, widths, sigmoid, precision):
        self.degree, self.widths, self.sigmoid, self.precision = degree, widths, int(bool(sigmoid)), int(precision)
        self.num_layers = len(widths)
        self.hidden = widths[0][0] if len(widths) > 1 else 0
        self.out_dim = widths[-1][0]

    def desc(self, wb):
        d = _lib.NerfBgDescC()
        d.degree, d.num_layers, d.hidden, d.out_dim = self.degree, self.num_layers, self.hidden, self.out_dim
        for l in range(self.num_layers):
            d.weight[l] = wb[2 * l].data_ptr()
            d.bias[l] = wb[2 * l + 1].data_ptr()
        d.sigmoid, d.precision = self.sigmoid, self.precision
        return d


class _LearnedBackground(Function):
    @staticmethod
    def forward(ctx, spec, keep, dirs, *wb):
        N = dirs.shape[0]
        out = torch.empty((N, spec.out_dim), dtype=torch.float32, device=dirs.device)
        if N:
            d = spec.desc(wb)
            with torch.cuda.device(dirs.device):
                _lib.check(_lib.lib().dwg_nerf_bg_forward(N, _lib.ptr(dirs), ctypes.byref(d), _lib.ptr(out), _lib.stream(dirs)), "dwg_nerf_bg_forward")
        ctx.spec, ctx.keep = spec, keep
        if keep:
            ctx.save_for_backward(dirs, *wb)
        return out

    @staticmethod
    def backward(ctx, d_out):
        if not ctx.keep:
            raise RuntimeError("learned_background was called with gradients off: nothing was saved for a backward")
        dirs, *wb = ctx.saved_tensors
        spec = ctx.spec
        need = ctx.needs_input_grad[3:]
        g_wb = [torch.empty_like(t) if need[i] else None for i, t in enumerate(wb)]
        if all(g is None for g in g_wb):
            return (None,) * (3 + len(wb))
        N = dirs.shape[0]
        if N == 0:
            return (None, None, None, *[None if g is None else g.zero_() for g in g_wb])
        d_out = d_out.float().contiguous()
        g = _lib.NerfBgGradsC()
        for l in range(spec.num_layers):
            g.weight[l] = None if g_wb[2 * l] is None else g_wb[2 * l].data_ptr()
            g.bias[l] = None if g_wb[2 * l + 1] is None else g_wb[2 * l + 1].data_ptr()
        d = spec.desc(wb)
        L = _lib.lib()
        nbytes = int(L.dwg_nerf_bg_backward_workspace_bytes(ctypes.byref(d)))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dirs.device)
        with torch.cuda.device(dirs.device):
            _lib.check(L.dwg_nerf_bg_backward(N, _lib.ptr(dirs), _lib.ptr(d_out), ctypes.byref(d), ctypes.byref(g), _lib.ptr(ws), nbytes,
                                              _lib.stream(dirs)), "dwg_nerf_bg_backward")
        return (None, None, None, *g_wb)


def learned_background(rays_d, encoder_bg, bg_net, sigmoid=True, precision=None):
    """rays_d [N, 3] fp32 on the device -> [N, C] fp32: epilogue(bg_net(encoder_bg(rays_d))), C = bg_net's output width (3 or 4),
    sigmoid for rgb, identity (sigmoid=False) in latent mode.

    precision: None follows autocast (nerf.autocast_precision), 0 f32, 1 f16 -- under f16 the result holds fp16 values in an fp32
    buffer (nerf_view.view_compose reads it in place; the reference's image_bg is half there).  The gradients of bg_net's weights and
    biases go back to autograd, only those it asks for; rays_d gets none and must not require one.  Under no_grad, or when no parameter
    requires grad, nothing is saved."""
    if precision is None:
        precision = nerf.autocast_precision()
    if precision not in (0, 1):
        raise RuntimeError("precision must be None, 0 (f32) or 1 (f16), got %r" % (precision,))
    _check_dirs("rays_d", rays_d)
    if rays_d.dim() != 2:
        raise RuntimeError("rays_d must have shape [N, 3], got %s" % (tuple(rays_d.shape),))
    reason = unsupported_reason(encoder_bg, bg_net)
    if reason is not None:
        raise RuntimeError("learned_background does not take this background: %s" % reason)
    wb, widths = [], []
    for l, lin in enumerate(bg_net.net):
        _lib.check_tensor("bg_net.net[%d].weight" % l, lin.weight, shape=(lin.out_features, lin.in_features), device=rays_d.device)
        _lib.check_tensor("bg_net.net[%d].bias" % l, lin.bias, shape=(lin.out_features,), device=rays_d.device)
        wb += [lin.weight, lin.bias]
        widths.append((lin.out_features, lin.in_features))
    spec = _Spec(int(encoder_bg.degree), widths, sigmoid, precision)
    # the saved state follows the CALLER's grad mode (inside Function.forward gradients are always off)
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in wb)
    return _LearnedBackground.apply(spec, keep, rays_d, *wb)
