"""MI355X-native field network of the NeRF stage (boundary B7): grid encoding -> sigma_net -> density / albedo in one kernel.

  nerf_field(x, encoder, sigma_net, sigma_scale, bound, ...)   autograd function over dwg_nerf_field_forward / _backward
                                 (include/dwg_nerf.h): what _NeRFNetwork.common_forward / local_geometry_forward compute
                                 (core/nerf/nerf_model.py:268-295) for the grid backbone, with gradients for the table, every
                                 sigma_net weight and bias and sigma_scale -- only those autograd asks for.
  bind_nerf_network(ref)         rebinds common_forward and local_geometry_forward of a constructed reference _NeRFNetwork to
                                 nerf_field; the reference's own Parameters are read in place (optimizer, checkpoints untouched).
                                 With cuda_ray it also rebinds update_extra_state to the native occupancy update (occupancy.py, B13)
                                 and run_cuda to the one-launch inference render (nerf_render.py, B14; with shaded_render=True
                                 also for the shaded views, B15; with train_render=True also the training view, B18).
Precision follows autocast: under torch.autocast(fp16) the kernels mirror the reference's fp16 rounding points (f16 MFMA, fp32
accumulation), otherwise they compute in exact f32.  The arithmetic is csrc/nerf_field.hip; no CPU fallback.  Every buffer is checked
(CUDA, contiguous, dtype, size) and a violation raises RuntimeError before any launch.
"""
import ctypes

import numpy as np
import torch
from torch.autograd import Function

from . import _lib

ACTIVATIONS = {'exp': 0, 'softplus': 1, 'scaling': 2}
PRIORS = {'none': 0, 'gaussian': 1, 'sqrt': 2}
MAX_LAYERS, MAX_HIDDEN, MAX_OUT, MAX_LEVELS = _lib.CONSTANTS["DWG_NERF_MAX_LAYERS"], 64, 16, 32


def _autocast_dtype():
    """The CUDA autocast dtype, None without autocast."""
    if not torch.is_autocast_enabled():
        return None
    return torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()


def autocast_precision():
    """1 (f16) under CUDA autocast to float16, 0 (f32) without autocast; other autocast dtypes are not covered."""
    dt = _autocast_dtype()
    if dt not in (None, torch.float16):
        raise RuntimeError("the fused NeRF field covers fp16 autocast only, got %s" % dt)
    return int(dt is not None)


def autocast_covered():
    """autocast_precision() would not raise: autocast is off or to float16."""
    return _autocast_dtype() in (None, torch.float16)


def _host_offsets(encoder):
    """ctypes int32 copy of encoder.offsets, cached on the encoder by the buffer's address and version."""
    off = encoder.offsets
    key = (off.data_ptr(), off._version, off.numel())
    c = getattr(encoder, "_dwg_nerf_host_offsets", None)
    if c is None or c[0] != key:
        vals = [int(v) for v in off.detach().cpu().tolist()]
        c = (key, (ctypes.c_int32 * len(vals))(*vals))
        encoder._dwg_nerf_host_offsets = c
    return c[1]


class FieldSpec:
    """Everything of the field that is not a tensor autograd differentiates."""

    def __init__(self, encoder, sigma_net, bound, density_activation, density_prior, albedo_sigmoid, raw, precision):
        lins = list(sigma_net.net)
        self.L = int(encoder.num_levels)
        self.S = float(np.log2(encoder.per_level_scale))
        self.H = int(encoder.base_resolution)
        self.gridtype = int(encoder.gridtype_id)
        self.align_corners = int(bool(encoder.align_corners))
        self.interp = int(encoder.interp_id)
        self.offsets = encoder.offsets
        self.host_offsets = _host_offsets(encoder)
        self.bound = float(bound)
        self.num_layers = len(lins)
        self.hidden = int(lins[0].out_features) if len(lins) > 1 else 0
        self.out_dim = int(lins[-1].out_features)
        if density_activation not in ACTIVATIONS:
            raise RuntimeError("density_activation must be one of %s, got %r" % (sorted(ACTIVATIONS), density_activation))
        if density_prior not in PRIORS:
            raise RuntimeError("density_prior must be one of %s, got %r" % (sorted(PRIORS), density_prior))
        self.act = ACTIVATIONS[density_activation]
        self.prior = PRIORS[density_prior]
        self.albedo_sigmoid = int(bool(albedo_sigmoid))
        self.raw = int(bool(raw))
        self.precision = int(precision)

    def desc(self, embeddings, sigma_scale, wb):
        d = _lib.NerfFieldDescC()
        d.embeddings, d.offsets = embeddings.data_ptr(), self.offsets.data_ptr()
        d.host_offsets = ctypes.cast(self.host_offsets, ctypes.c_void_p)
        d.num_levels, d.log2_per_level_scale, d.base_resolution = self.L, self.S, self.H
        d.gridtype, d.align_corners, d.interp, d.bound = self.gridtype, self.align_corners, self.interp, self.bound
        d.num_layers, d.hidden, d.out_dim = self.num_layers, self.hidden, self.out_dim
        for l in range(self.num_layers):
            d.weight[l] = wb[2 * l].data_ptr()
            d.bias[l] = wb[2 * l + 1].data_ptr()
        d.density_activation, d.density_prior, d.albedo_sigmoid, d.raw = self.act, self.prior, self.albedo_sigmoid, self.raw
        d.sigma_scale = sigma_scale.data_ptr()
        d.precision = self.precision
        return d

    def check(self, x, embeddings, sigma_scale, wb):
        _lib.check_tensor("x", x, torch.float32)
        if x.dim() != 2 or x.shape[1] != 3:
            raise RuntimeError("x must be [M, 3], got %s" % (tuple(x.shape),))
        _lib.check_tensor("embeddings", embeddings, torch.float32)
        if embeddings.dim() != 2 or embeddings.shape[1] != 2:
            raise RuntimeError("embeddings must be [entries, 2] (level_dim 2), got %s" % (tuple(embeddings.shape),))
        _lib.check_tensor("offsets", self.offsets, torch.int32, numel=self.L + 1)
        if not 1 <= self.L <= MAX_LEVELS:
            raise RuntimeError("the fused field takes 1..%d levels, got %d" % (MAX_LEVELS, self.L))
        if int(self.host_offsets[self.L]) != embeddings.shape[0]:
            raise RuntimeError("embeddings has %d entries, offsets say %d" % (embeddings.shape[0], int(self.host_offsets[self.L])))
        _lib.check_tensor("sigma_scale", sigma_scale, torch.float32, numel=1)
        if not 1 <= self.num_layers <= MAX_LAYERS:
            raise RuntimeError("sigma_net must have 1..%d layers, got %d" % (MAX_LAYERS, self.num_layers))
        if self.num_layers > 1 and not 1 <= self.hidden <= MAX_HIDDEN:
            raise RuntimeError("sigma_net hidden width must be 1..%d, got %d" % (MAX_HIDDEN, self.hidden))
        if not 2 <= self.out_dim <= MAX_OUT:
            raise RuntimeError("sigma_net output width must be 2..%d, got %d" % (MAX_OUT, self.out_dim))
        for l in range(self.num_layers):
            k = 2 * self.L if l == 0 else self.hidden
            n = self.out_dim if l == self.num_layers - 1 else self.hidden
            _lib.check_tensor("sigma_net.net[%d].weight" % l, wb[2 * l], torch.float32, numel=n * k)
            _lib.check_tensor("sigma_net.net[%d].bias" % l, wb[2 * l + 1], torch.float32, numel=n)


def field_forward(spec, embeddings, sigma_scale, wb, x):
    """(sigma [M] fp32, albedo [M, out_dim - 1] in the spec's precision) of dwg_nerf_field_forward at x [M, 3]; the caller has checked."""
    M = x.shape[0]
    sigma = torch.empty(M, device=x.device, dtype=torch.float32)
    albedo = torch.empty(M, spec.out_dim - 1, device=x.device, dtype=torch.float16 if spec.precision else torch.float32)
    d = spec.desc(embeddings, sigma_scale, wb)
    _lib.check(_lib.lib().dwg_nerf_field_forward(ctypes.byref(d), _lib.ptr(x), M, _lib.ptr(sigma), _lib.ptr(albedo), _lib.stream(x)),
               "dwg_nerf_field_forward")
    return sigma, albedo


def field_backward(spec, embeddings, sigma_scale, wb, x, dsigma, dalbedo, g_emb, g_ss, g_wb, fd=None, accumulate=0):
    """dwg_nerf_field_backward over the M rows of x into the wanted gradient tensors (g_emb, g_ss and each of g_wb: None when not
    wanted); with fd = (eps, dsigma_fd [M, 6]) dwg_nerf_field_backward_fd, which also takes the six shifted point sets.  The table
    gradient is added into; the others are overwritten unless accumulate."""
    g = _lib.NerfFieldGradsC()
    g.embeddings = None if g_emb is None else g_emb.data_ptr()
    for l in range(spec.num_layers):
        g.weight[l] = None if g_wb[2 * l] is None else g_wb[2 * l].data_ptr()
        g.bias[l] = None if g_wb[2 * l + 1] is None else g_wb[2 * l + 1].data_ptr()
    g.sigma_scale = None if g_ss is None else g_ss.data_ptr()
    g.accumulate = accumulate
    d = spec.desc(embeddings, sigma_scale, wb)
    L, M = _lib.lib(), x.shape[0]
    nbytes = int(L.dwg_nerf_field_backward_workspace_bytes(ctypes.byref(d), M))
    ws = torch.empty(max(nbytes, 1), device=x.device, dtype=torch.uint8)
    tail = (ctypes.byref(g), _lib.ptr(ws), nbytes, _lib.stream(x))
    if fd is None:
        _lib.check(L.dwg_nerf_field_backward(ctypes.byref(d), _lib.ptr(x), M, _lib.ptr(dsigma), _lib.ptr(dalbedo), *tail), "dwg_nerf_field_backward")
    else:
        _lib.check(L.dwg_nerf_field_backward_fd(ctypes.byref(d), _lib.ptr(x), M, ctypes.c_float(fd[0]), _lib.ptr(dsigma), _lib.ptr(dalbedo),
                                                _lib.ptr(fd[1]), *tail), "dwg_nerf_field_backward_fd")


class _NerfField(Function):
    @staticmethod
    def forward(ctx, spec, x, embeddings, sigma_scale, *wb):
        spec.check(x, embeddings, sigma_scale, wb)
        sigma, albedo = field_forward(spec, embeddings, sigma_scale, wb, x)
        ctx.spec = spec
        ctx.save_for_backward(x, embeddings, sigma_scale, *wb)
        ctx.albedo_dtype = albedo.dtype
        return sigma, albedo

    @staticmethod
    def backward(ctx, dsigma, dalbedo):
        x, embeddings, sigma_scale, *wb = ctx.saved_tensors
        spec = ctx.spec
        need = ctx.needs_input_grad
        M = x.shape[0]
        dsigma = torch.zeros(M, device=x.device, dtype=torch.float32) if dsigma is None else dsigma.float().contiguous()
        dalbedo = (torch.zeros(M, spec.out_dim - 1, device=x.device, dtype=ctx.albedo_dtype) if dalbedo is None
                   else dalbedo.to(ctx.albedo_dtype).contiguous())
        g_emb = torch.zeros_like(embeddings) if need[2] else None
        g_ss = torch.empty_like(sigma_scale) if (need[3] and spec.act == ACTIVATIONS['scaling']) else None
        g_wb = [torch.empty_like(t) if need[4 + i] else None for i, t in enumerate(wb)]
        if g_emb is None and g_ss is None and all(t is None for t in g_wb):
            return (None,) * (4 + len(wb))
        field_backward(spec, embeddings, sigma_scale, wb, x, dsigma, dalbedo, g_emb, g_ss, g_wb)
        return (None, None, g_emb, g_ss if need[3] else None, *g_wb)


def nerf_field(x, encoder, sigma_net, sigma_scale, bound, density_activation='exp', density_prior='none', albedo_sigmoid=True, raw=False,
               mlp_no_grad=False, precision=None):
    """(sigma, albedo) of the field at x [..., 3] in [-bound, bound].

    raw: sigma is the last layer's output (no activation, no prior); albedo_sigmoid: the rgb postprocess (False in latent mode).
    mlp_no_grad: sigma_net's parameters get no gradient (local_geometry_forward(mlp_no_grad=True)).  precision: None follows autocast,
    0 f32, 1 f16.  Returns sigma fp32 (fp16 when raw under f16, as the reference's h[..., 0]) and albedo fp16 under f16, else fp32.
    The gradient with respect to x is not computed: x must not require it."""
    if precision is None:
        precision = autocast_precision()
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise RuntimeError("nerf_field does not compute the gradient with respect to x (use the reference's path for it)")
    if not isinstance(x, torch.Tensor) or x.shape[-1] != 3:
        raise RuntimeError("x must be a tensor [..., 3]")
    spec = FieldSpec(encoder, sigma_net, bound, density_activation, density_prior, albedo_sigmoid, raw, precision)
    prefix = list(x.shape[:-1])
    wb = []
    for lin in sigma_net.net:
        if lin.bias is None:
            raise RuntimeError("sigma_net layers must have a bias")
        wb += [lin.weight.detach(), lin.bias.detach()] if mlp_no_grad else [lin.weight, lin.bias]
    ss = sigma_scale.reshape(1) if isinstance(sigma_scale, torch.Tensor) else None
    if ss is None:
        raise RuntimeError("sigma_scale must be a tensor")
    sigma, albedo = _NerfField.apply(spec, x.reshape(-1, 3), encoder.embeddings, ss, *wb)
    if raw and precision:
        sigma = sigma.half()
    return sigma.view(prefix), albedo.view(prefix + [spec.out_dim - 1])


# ------------------------------------------------------------------------------------------------------------------------------------
# binding a constructed reference network
# ------------------------------------------------------------------------------------------------------------------------------------
def unbound_reason(ref):
    """None when the kernels cover this reference network, else why not."""
    name = type(ref).__name__
    if name != "_NeRFNetwork":
        return "structure %s (dual_mlp / dual_enc) is not the shared-MLP network" % name
    if getattr(ref, "density_prior_type", None) not in PRIORS:
        return "density_prior %r is not covered (none, gaussian, sqrt)" % (getattr(ref, "density_prior_type", None),)
    if getattr(ref, "decoder_layer", None) is not None:
        return "nerf_type with a decoder_layer (latent_tune / latent_approx) is not covered"
    enc = getattr(ref, "encoder", None)
    if enc is None or not all(hasattr(enc, a) for a in ("embeddings", "offsets", "per_level_scale", "base_resolution", "gridtype_id",
                                                        "interp_id", "align_corners", "num_levels")):
        return "backbone %s is not a grid encoder" % type(enc).__name__
    if getattr(enc, "input_dim", 3) != 3 or getattr(enc, "level_dim", 2) != 2:
        return "grid encoder input_dim %s / level_dim %s (the kernels take 3 / 2)" % (getattr(enc, "input_dim", None), getattr(enc, "level_dim", None))
    if not 1 <= int(enc.num_levels) <= MAX_LEVELS:
        return "num_levels %d beyond the kernel's %d" % (int(enc.num_levels), MAX_LEVELS)
    net = getattr(getattr(ref, "sigma_net", None), "net", None)
    if net is None or not 1 <= len(net) <= MAX_LAYERS:
        return "sigma_net with %s layers (the kernels take 1..%d)" % (None if net is None else len(net), MAX_LAYERS)
    if any(not isinstance(l, torch.nn.Linear) or l.bias is None for l in net):
        return "sigma_net layers are not biased nn.Linear"
    if len(net) > 1 and net[0].out_features > MAX_HIDDEN:
        return "sigma_net hidden width %d beyond the kernel's %d" % (net[0].out_features, MAX_HIDDEN)
    if not 2 <= net[-1].out_features <= MAX_OUT:
        return "sigma_net output width %d beyond the kernel's %d" % (net[-1].out_features, MAX_OUT)
    act = getattr(getattr(ref, "opt", None), "density_activation", None)
    if act not in ACTIVATIONS:
        return "density_activation %r is not covered" % (act,)
    if not isinstance(getattr(ref, "sigma_scale", None), torch.Tensor):
        return "the network has no sigma_scale parameter"
    return None


def _covered_call(x):
    """The kernels take this call: a CUDA fp32 x that needs no gradient, and no autocast dtype but fp16."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.requires_grad:
        return False
    return autocast_covered()


def bind_nerf_network(ref, shaded_render=False, train_render=False):
    """Rebind ref.common_forward / ref.local_geometry_forward to the fused kernels.  Returns None when bound, else the reason it was
    left unbound (also kept as ref._dwg_nerf_unbound).  Calls the kernels do not take (x requiring a gradient -- the autograd normal --,
    a CPU x, bf16 autocast) go to the original methods.  shaded_render: the installed run_cuda also takes the evaluation views with
    shading 'normal', 'textureless' and 'lambertian' (nerf_render.covered_call, B15); off, they stay on the original method.
    train_render: the installed run_cuda also takes the training view with shading 'albedo' (nerf_render.render_rays_train, B18: the
    backward runs over the samples the composite used); off, training calls stay on the original method.  train_render='shaded': also
    the training views with shading 'normal', 'textureless' and 'lambertian' (B19, nerf_render.covered_train_call); with True they stay
    on the original method.  render() itself is bound by bind_nerf_view (B20), on request."""
    reason = unbound_reason(ref)
    if reason is not None:
        ref._dwg_nerf_unbound = reason
        return reason
    ref._dwg_shaded_render = bool(shaded_render)
    ref._dwg_train_render = bool(train_render)
    ref._dwg_train_shaded = isinstance(train_render, str) and train_render == 'shaded'
    if getattr(ref, "_dwg_nerf_bound", False):
        return None
    orig_common, orig_local = ref.common_forward, ref.local_geometry_forward
    latent = bool(getattr(ref, "latent_mode", False))

    def _field(x, raw, sigmoid, mlp_no_grad=False):
        return nerf_field(x, ref.encoder, ref.sigma_net, ref.sigma_scale, ref.bound, density_activation=ref.opt.density_activation,
                          density_prior=ref.density_prior_type, albedo_sigmoid=sigmoid, raw=raw, mlp_no_grad=mlp_no_grad)

    def common_forward(x, mask=None, return_raw=False, **kwargs):
        if not _covered_call(x):
            return orig_common(x, mask=mask, return_raw=return_raw, **kwargs)
        if return_raw:
            return _field(x, raw=True, sigmoid=False)
        sigma, albedo = _field(x, raw=False, sigmoid=not latent)
        if mask is not None:
            sigma = sigma * mask
        return sigma, albedo

    def local_geometry_forward(x, mlp_no_grad=False):
        if not _covered_call(x):
            return orig_local(x, mlp_no_grad=mlp_no_grad)
        return _field(x, raw=True, sigmoid=not latent, mlp_no_grad=mlp_no_grad)

    common_forward.__wrapped__ = orig_common
    local_geometry_forward.__wrapped__ = orig_local
    ref.common_forward = common_forward
    ref.local_geometry_forward = local_geometry_forward
    _bind_update_extra_state(ref)
    _bind_run_cuda(ref)
    ref._dwg_nerf_bound = True
    ref._dwg_nerf_unbound = None
    return None


def _occupancy_covered(ref):
    """The native occupancy update (boundary B13, occupancy.py) takes this network's render state: cuda_ray with density_grid /
    density_bitfield buffers within dwg_occupancy.h's limits."""
    from . import occupancy
    if not getattr(ref, "cuda_ray", False) or not hasattr(type(ref), "update_extra_state"):
        return False
    grid, bits = getattr(ref, "density_grid", None), getattr(ref, "density_bitfield", None)
    H, C = getattr(ref, "grid_size", None), getattr(ref, "cascade", None)
    if not isinstance(grid, torch.Tensor) or not isinstance(bits, torch.Tensor) or not isinstance(H, int) or not isinstance(C, int):
        return False
    if not occupancy.within_limits(C, H) or not float(ref.bound) > 0 or C != occupancy.cascades(float(ref.bound)):
        return False
    return (grid.dtype == torch.float32 and tuple(grid.shape) == (C, H ** 3) and bits.dtype == torch.uint8 and bits.numel() == C * H ** 3 // 8)


def _bind_update_extra_state(ref):
    """Install update_extra_state(decay, S, random_sigmas) on a bound network: occupancy.OccupancyGrid.update on the reference's own
    buffers (state_dict and checkpoints untouched), then mean_density / min_density / max_density / iter_density from one stats() read
    and the reference's step-counter statements as they are (nerf_renderer.py:149-153; mean_count's .item() is the second, 4-byte,
    read).  The original method takes the calls the kernels do not: not cuda_ray, a chunked update (S below grid_size: the chunked order
    of the draws is not restated), buffers or parameters on the CPU, bf16 autocast."""
    if "update_extra_state" in ref.__dict__ or not _occupancy_covered(ref):
        return
    from . import occupancy
    orig_update = ref.update_extra_state

    def _grid():
        g = getattr(ref, "_dwg_occupancy", None)
        if (g is None or g.density_grid.data_ptr() != ref.density_grid.data_ptr() or g.density_bitfield.data_ptr() != ref.density_bitfield.data_ptr()
                or g.density_thresh != float(ref.density_thresh)):
            g = occupancy.OccupancyGrid(ref.grid_size, ref.bound, ref.density_thresh, density_grid=ref.density_grid,
                                        density_bitfield=ref.density_bitfield)
            object.__setattr__(ref, "_dwg_occupancy", g)
        return g

    def _native(S):
        if not ref.cuda_ray or (S is not None and S < ref.grid_size):
            return False
        grid, bits = ref.density_grid, ref.density_bitfield
        if not (grid.is_cuda and bits.is_cuda and grid.is_contiguous() and bits.is_contiguous() and grid.data_ptr() % 16 == 0):
            return False
        if not (ref.encoder.embeddings.is_cuda and ref.sigma_scale.is_cuda):
            return False
        return autocast_covered()

    def update_extra_state(decay=0.95, S=None, random_sigmas=False):
        if not _native(S):
            return orig_update(decay=decay, S=S, random_sigmas=random_sigmas)
        g = _grid()
        g.update(ref.encoder, ref.sigma_net, ref.sigma_scale, density_activation=ref.opt.density_activation,
                 density_prior=ref.density_prior_type, decay=decay, random_sigmas=random_sigmas)
        st = g.stats()
        ref.mean_density, ref.min_density, ref.max_density = st["mean_density"], st["min_density"], st["max_density"]
        ref.iter_density += 1
        ### update step counter
        total_step = min(16, ref.local_step)
        if total_step > 0:
            ref.mean_count = int(ref.step_counter[:total_step, 0].sum().item() / total_step)
        ref.local_step = 0

    update_extra_state.__wrapped__ = orig_update
    ref.update_extra_state = update_extra_state


def _bind_run_cuda(ref):
    """Install run_cuda on a bound network with cuda_ray: nerf_render.run_cuda, which renders an evaluation view (not training, shading
    'albedo' -- or a shaded view when ref._dwg_shaded_render --, no perturbation, CUDA fp32 rays, no autocast or fp16 autocast) in one
    launch, takes the training view with shading 'albedo' through nerf_render.render_rays_train when ref._dwg_train_render (the shaded
    training views too when ref._dwg_train_shaded), and hands every other call to the original method unchanged."""
    if "run_cuda" in ref.__dict__ or not getattr(ref, "cuda_ray", False) or not hasattr(type(ref), "run_cuda"):
        return
    from . import nerf_render
    orig_run = ref.run_cuda

    def run_cuda(rays_o, rays_d, *args, **kwargs):
        return nerf_render.run_cuda(ref, orig_run, rays_o, rays_d, *args, **kwargs)

    run_cuda.__wrapped__ = orig_run
    ref.run_cuda = run_cuda


def bind_nerf_view(ref):
    """Opt-in, on a network bind_nerf_network has bound (boundary B20): ref.render becomes nerf_view.render_view for the calls
    nerf_view.covered_view takes -- rays, run_cuda's native branches and the background mix with the planar image, one launch each
    around the render.  The learned 'nerf' background is rendered natively too (boundary B22, nerf_background.learned_background) when
    the network has a bg_net of supported biased nn.Linear layers on the camera's device, an encoder_bg of 3 inputs with a supported
    degree and no decoder_layer -- a reference _NeRFNetwork built with bg_mode='nerf' has them.  dmtet, a network without cuda_ray,
    staged, several cameras, a camera that is not fp32 on the device, a 'nerf' background on a network without such a bg_net and the
    run_cuda calls the native renders do not take (a training view needs train_render) go to the original render, decided before anything
    is drawn.  Returns None when bound, else the reason.  unbind_nerf_network removes it."""
    if not getattr(ref, "_dwg_nerf_bound", False):
        return "the network is not bound (bind_nerf_network first)"
    if not hasattr(type(ref), "render"):
        return "%s has no render method" % type(ref).__name__
    _bind_render(ref)
    return None


def _bind_render(ref):
    if "render" in ref.__dict__:
        return
    from . import nerf_view
    orig_render = ref.render

    def render(data, shading='albedo', bg_mode=None, staged=False, **kwargs):
        if set(kwargs) - {"light_d", "ambient_ratio", "dt_gamma", "max_steps", "T_thresh"} or not nerf_view.covered_view(
                ref, data, shading, bg_mode, staged, kwargs.get("light_d"), kwargs.get("ambient_ratio", 1.0)):
            return orig_render(data, shading=shading, bg_mode=bg_mode, staged=staged, **kwargs)
        return nerf_view.render_view(ref, data, shading=shading, bg_mode=bg_mode, **kwargs)

    render.__wrapped__ = orig_render
    ref.render = render


def unbind_nerf_network(ref):
    """Undo bind_nerf_network (the instance attributes go; the class methods show through again)."""
    for name in ("common_forward", "local_geometry_forward", "update_extra_state", "run_cuda", "render", "_dwg_occupancy", "_dwg_shaded_render",
                 "_dwg_train_render", "_dwg_train_shaded"):
        if name in ref.__dict__:
            del ref.__dict__[name]
    ref._dwg_nerf_bound = False
