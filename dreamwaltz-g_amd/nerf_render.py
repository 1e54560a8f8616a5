"""MI355X-native inference render of the NeRF stage (boundaries B14 and B15): what the evaluation branch of the reference's
_NeRFRenderer.run_cuda (core/nerf/nerf_renderer.py:351-385) computes for perturb False, in ONE launch of csrc/nerf_field.hip's
k_nf_render (shading 'albedo') or k_nf_render_shaded ('normal', 'textureless', 'lambertian': seven field evaluations per sample, the
finite-difference normal and the shading in the kernel) instead of a Python loop of march_rays -> field -> composite_rays with three
zeroed buffers and one host wait per iteration.

  render_rays(rays_o, rays_d, nears, fars, density_bitfield, cascade, grid_size, encoder, sigma_net, sigma_scale, bound, ...)
                                 (weights_sum [N], depth [N], image [N, out_dim - 1][, counts [N]]) through dwg_nerf_render_infer
                                 or, with shading=..., dwg_nerf_render_shaded (include/dwg_nerf_render.h)
  render_rays_train(...)         the training render (boundary B18): march_rays_train -> field -> composite_rays_train as one autograd
                                 function whose backward runs over the samples the composite used (include/dwg_nerf_train.h); with
                                 shading=... the shaded one (B19): the backward also goes through the shading and the normal
  run_cuda(ref, orig, ...)       the statements of run_cuda around them, for a bound reference network (nerf.bind_nerf_network installs it)

A ray's samples, and everything composited from them, are the loop's: the marching rule is the shared csrc/raymarch_common.h, the field
is the fused kernel's field_tile, the composite is composite_rays' statements in their order.  The one difference: a ray stops after
exactly max_steps composited samples, where the loop's budget (n_step per iteration) lets a ray still alive at the end take between
max_steps and max_steps + 7; rays that end at far or by T_thresh are unaffected.  Precision follows autocast like nerf.nerf_field.
No CPU fallback, no host synchronisation (after the encoder's offsets have been read once); every buffer is checked (CUDA, dtype, shape,
contiguity) and a violation raises RuntimeError before any launch.  render_rays records no autograd state; render_rays_train is the one
autograd function here (its host reads: the march's M and 4 bytes of M_live)."""
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import nerf
from . import pointcloud
from . import raymarch



SHADINGS = {'albedo': 0, 'normal': 1, 'textureless': 2, 'lambertian': 3}


def _grid_shape(cascade, grid_size):
    """(C, H) as integers when the renders take an occupancy grid of this shape, else None."""
    C, H = int(cascade), int(grid_size)
    if C != cascade or H != grid_size or not (1 <= C <= 8 and 2 <= H <= 1024 and C * H ** 3 < 1 << 32) or H & (H - 1):
        return None
    return C, H


def _check_render(rays_o, rays_d, nears, fars, density_bitfield, cascade, grid_size, max_steps, shading, light_d, ambient_ratio, epsilon,
                  epsilon_name, *field):
    """What render_rays and render_rays_train both check of a call, before any launch: the shading's name, the field (`field`:
    pointcloud.field_spec's arguments), the rays, nears / fars, the occupancy grid, max_steps, the shading's arguments (a given light_d,
    the epsilon under the caller's name for it, ambient_ratio, latent 'lambertian') and that everything is on rays_o's device.
    -> (spec, embeddings, sigma_scale [1], [w0, b0, ...] detached, N, C, H)."""
    if shading not in SHADINGS:
        raise RuntimeError("shading must be one of %s, got %r" % (", ".join(sorted(SHADINGS)), shading))
    try:
        spec, emb, ss, wb = pointcloud.field_spec(*field)
    except ValueError as e:
        raise RuntimeError(str(e)) from None
    _lib.check_tensor("rays_o", rays_o, torch.float32, (None, 3))
    N = rays_o.shape[0]
    _lib.check_tensor("rays_d", rays_d, torch.float32, (N, 3))
    _lib.check_tensor("nears", nears, torch.float32, (N,))
    _lib.check_tensor("fars", fars, torch.float32, (N,))
    grid = _grid_shape(cascade, grid_size)
    if grid is None:
        raise RuntimeError("bad occupancy grid shape: cascade %r, grid_size %r (a power of two: a cell's Morton index must stay below "
                           "grid_size^3)" % (cascade, grid_size))
    C, H = grid
    _lib.check_tensor("density_bitfield", density_bitfield, torch.uint8, (C * H ** 3 // 8,))
    if int(max_steps) != max_steps or not 1 <= max_steps < 1 << 31:
        raise RuntimeError("max_steps must be an integer >= 1, got %r" % (max_steps,))
    others = []
    if SHADINGS[shading]:
        if light_d is not None:
            _lib.check_tensor("light_d", light_d, torch.float32, (3,))
            others.append(("light_d", light_d))
        elif SHADINGS[shading] >= 2:
            raise RuntimeError("shading %r needs light_d" % shading)
        if SHADINGS[shading] == 3 and spec.out_dim == 5:
            raise RuntimeError("shading 'lambertian' with four albedo channels (latent mode) is ill-formed in the reference: five channels "
                               "into a four-channel image")
        if not float(epsilon) > 0:
            raise RuntimeError("%s must be positive, got %r" % (epsilon_name, epsilon))
        if float(ambient_ratio) != float(ambient_ratio):
            raise RuntimeError("ambient_ratio is NaN")
    _same_device(rays_o.device, [("rays_d", rays_d), ("nears", nears), ("fars", fars), ("density_bitfield", density_bitfield),
                                 ("embeddings", emb)] + others)
    return spec, emb, ss, wb, N, C, H


def _same_device(dev, named):
    for name, t in named:
        if t.device != dev:
            raise RuntimeError("%s is on %s, rays_o on %s" % (name, t.device, dev))


@torch.no_grad()
def render_rays(rays_o, rays_d, nears, fars, density_bitfield, cascade, grid_size, encoder, sigma_net, sigma_scale, bound, *,
                density_activation, density_prior, albedo_sigmoid, dt_gamma=0, max_steps=1024, T_thresh=1e-4, binarize=False, contract=False,
                precision=None, return_counts=False, max_workgroups=0, shading='albedo', light_d=None, ambient_ratio=1.0, normal_epsilon=1e-3):
    """rays_o / rays_d [N, 3], nears / fars [N] fp32 on the device; density_bitfield [cascade * grid_size^3 / 8] uint8.  Returns
    (weights_sum [N], depth [N], image [N, out_dim - 1]) fp32, and counts [N] int32 (samples composited per ray) with return_counts.
    precision: None follows autocast, 0 f32, 1 f16.  max_workgroups: the number of persistent workgroups (0: the default).
    shading: 'albedo', or 'normal' / 'textureless' / 'lambertian' from the finite-difference normal with step normal_epsilon; light_d
    [3] fp32 on the device (needed by 'textureless' and 'lambertian', never read on the host) and ambient_ratio as forward() takes them.
    'lambertian' with four albedo channels is ill-formed in the reference and refused."""
    spec, emb, ss, wb, N, C, H = _check_render(
        rays_o, rays_d, nears, fars, density_bitfield, cascade, grid_size, max_steps, shading, light_d, ambient_ratio, normal_epsilon,
        "normal_epsilon", encoder, sigma_net, sigma_scale, bound, density_activation, density_prior, albedo_sigmoid, precision)
    if N >= 1 << 32:
        raise RuntimeError("render_rays takes fewer than 2^32 rays")
    if int(max_workgroups) != max_workgroups or not 0 <= max_workgroups < 1 << 31:
        raise RuntimeError("max_workgroups must be a non-negative integer, got %r" % (max_workgroups,))
    dev = rays_o.device
    weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    image = torch.empty((N, spec.out_dim - 1), dtype=torch.float32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev) if return_counts else None
    if N:
        d = spec.desc(emb, ss, wb)
        head = (ctypes.byref(d), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(nears), _lib.ptr(fars), N, _lib.ptr(density_bitfield),
                ctypes.c_float(bound), int(bool(contract)), ctypes.c_float(dt_gamma), int(max_steps), C, H, ctypes.c_float(T_thresh),
                int(bool(binarize)))
        tail = (_lib.ptr(weights_sum), _lib.ptr(depth), _lib.ptr(image), _lib.ptr(counts), int(max_workgroups), _lib.stream(rays_o))
        with torch.cuda.device(dev):
            if SHADINGS[shading]:
                _lib.check(_lib.lib().dwg_nerf_render_shaded(*head, SHADINGS[shading], _lib.ptr(light_d), ctypes.c_float(ambient_ratio),
                                                             ctypes.c_float(normal_epsilon), *tail), "dwg_nerf_render_shaded")
            else:
                _lib.check(_lib.lib().dwg_nerf_render_infer(*head, *tail), "dwg_nerf_render_infer")
    return (weights_sum, depth, image, counts) if return_counts else (weights_sum, depth, image)


# ------------------------------------------------------------------------------------------------------------------------------------
# training render (boundary B18)
# ------------------------------------------------------------------------------------------------------------------------------------
def _shade_train(L, st, sigma_fd, albedo, M, ch, rgbs, stream):
    """dwg_nerf_train_shade_forward of the call's shading over M rows into rgbs [M, ch] fp32."""
    _lib.check(L.dwg_nerf_train_shade_forward(
        st.shading, _lib.ptr(sigma_fd), _lib.ptr(albedo) if st.shading == 3 else None, int(albedo.dtype == torch.float16), _lib.ptr(st.light_d),
        ctypes.c_float(st.ratio), ctypes.c_float(st.eps), M, ch, _lib.ptr(rgbs), stream), "dwg_nerf_train_shade_forward")


class _RenderRaysTrain(Function):
    """march -> field -> composite in the forward; of the per-sample arrays only the rows the composite used are kept, and the backward
    (composite backward -> field backward) runs over those.  `st`: the call's settings, and where the non-differentiable extras go.
    With st.shading (B19): the field also returns the densities at the six shifted points, the colours are shaded from them
    (csrc/shade_math.h), and the backward goes composite -> shade -> the seven-point-set field backward, all over the live rows."""

    @staticmethod
    def forward(ctx, st, rays_o, rays_d, nears, fars, bits, noises, counter, embeddings, sigma_scale, *wb):
        spec, L, dev = st.spec, _lib.lib(), rays_o.device
        N, ch = rays_o.shape[0], spec.out_dim - 1
        # 1. the march of raymarch.march_rays_train: count pass, one host read of M, write pass
        rays = torch.empty(N, 2, dtype=torch.int32, device=dev)
        march = (rays_o, rays_d, bits, st.bound, st.contract, st.dt_gamma, st.max_steps, N, st.C, st.H, nears, fars)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        raymarch.march_rays_train_into(*march, None, None, None, rays, count, noises)
        M = int(count.item())
        if counter is not None:
            counter[:1].add_(count)                                         # what the march adds to the caller's counter
        xyzs = torch.zeros(M, 3, dtype=torch.float32, device=dev)
        ts = torch.zeros(M, 2, dtype=torch.float32, device=dev)
        if M:
            dirs = torch.zeros(M, 3, dtype=torch.float32, device=dev)       # the write pass fills it; 'albedo' never reads it
            raymarch.march_rays_train_into(*march, xyzs, dirs, ts, rays, count, noises)
            del dirs
        # 2. the field
        if st.shading:
            sigmas = torch.empty(M, dtype=torch.float32, device=dev)
            albedo = torch.empty(M, ch, dtype=torch.float16 if spec.precision else torch.float32, device=dev)
            sigma_fd = torch.empty(M, 6, dtype=torch.float32, device=dev)
            if M:
                d = spec.desc(embeddings, sigma_scale, wb)
                _lib.check(L.dwg_nerf_field_forward_fd(ctypes.byref(d), _lib.ptr(xyzs), M, ctypes.c_float(st.eps), _lib.ptr(sigmas),
                                                       _lib.ptr(albedo), _lib.ptr(sigma_fd), _lib.stream(rays_o)), "dwg_nerf_field_forward_fd")
            rgbs = torch.empty(M, ch, dtype=torch.float32, device=dev)
            _shade_train(L, st, sigma_fd, albedo, M, ch, rgbs, _lib.stream(rays_o))
        else:
            sigma_fd = None
            sigmas, albedo = nerf.field_forward(spec, embeddings, sigma_scale, wb, xyzs)
            rgbs = albedo.float() if spec.precision else albedo             # the composite reads fp32, as composite_rays_train casts
        # 3. the composite, which also reports where each ray stopped
        weights = torch.zeros(M, dtype=torch.float32, device=dev) if st.return_weights else None
        weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        image = torch.empty(N, ch, dtype=torch.float32, device=dev)
        live = torch.empty(N, dtype=torch.int32, device=dev)
        _lib.check(L.dwg_raymarch_composite_rays_train_forward_live(
            _lib.ptr(sigmas), _lib.ptr(rgbs), _lib.ptr(ts), _lib.ptr(rays), M, N, ch, ctypes.c_float(st.T_thresh), int(st.binarize),
            _lib.ptr(weights), _lib.ptr(weights_sum), _lib.ptr(depth), _lib.ptr(image), _lib.ptr(live), _lib.stream(rays_o)),
            "dwg_raymarch_composite_rays_train_forward_live")
        del rgbs
        st.M, st.weights, st.sigmas = M, weights, sigmas if st.return_sigmas else None
        st.live = live if st.return_stats else None
        if not (st.keep or st.return_stats):
            st.M_live = None
            return weights_sum, depth, image
        # 4. offsets of the live samples; the one host read this render adds to the march's
        rays_live = torch.empty(N, 2, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int32, device=dev)
        nbytes = int(L.dwg_nerf_train_workspace_bytes(N))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(L.dwg_nerf_train_compact_offsets(_lib.ptr(live), N, _lib.ptr(rays_live), _lib.ptr(total), _lib.ptr(ws), nbytes, _lib.stream(rays_o)),
                   "dwg_nerf_train_compact_offsets")
        M_live = int(total.item()) if N and M else 0
        st.M_live = M_live
        if not st.keep:
            return weights_sum, depth, image
        # 5. the gather: only the live rows stay for the backward (nothing culled: the live rows are the rows, rays_live is rays)
        if st.shading != 3 and st.shading:
            albedo = albedo[:0]                                             # only 'lambertian' reads the albedo again
        if M_live == M:
            xyzs_l, ts_l, sigmas_l, albedo_l, sigma_fd_l = xyzs, ts, sigmas, albedo, sigma_fd
        else:
            xyzs_l = torch.empty(M_live, 3, dtype=torch.float32, device=dev)
            ts_l = torch.empty(M_live, 2, dtype=torch.float32, device=dev)
            sigmas_l = torch.empty(M_live, dtype=torch.float32, device=dev)
            albedo_l = torch.empty(M_live if albedo.shape[0] else 0, ch, dtype=albedo.dtype, device=dev)
            sigma_fd_l = torch.empty(M_live, 6, dtype=torch.float32, device=dev) if st.shading else None
        if 0 < M_live < M:
            moved = albedo.shape[0] > 0
            _lib.check(L.dwg_nerf_train_gather_live(
                _lib.ptr(rays), _lib.ptr(rays_live), N, M, M_live, _lib.ptr(xyzs), _lib.ptr(xyzs_l), _lib.ptr(ts), _lib.ptr(ts_l),
                _lib.ptr(sigmas), _lib.ptr(sigmas_l), _lib.ptr(albedo) if moved else None, _lib.ptr(albedo_l) if moved else None, ch,
                int(spec.precision), _lib.stream(rays_o)), "dwg_nerf_train_gather_live")
            if st.shading:
                _lib.check(L.dwg_nerf_train_gather_live_rows(_lib.ptr(rays), _lib.ptr(rays_live), N, M, M_live, _lib.ptr(sigma_fd),
                                                             _lib.ptr(sigma_fd_l), 6, _lib.stream(rays_o)), "dwg_nerf_train_gather_live_rows")
        ctx.st = st
        if st.shading:
            ctx.save_for_backward(xyzs_l, ts_l, sigmas_l, albedo_l, rays_live, weights_sum, depth, image, embeddings, sigma_scale, *wb,
                                  sigma_fd_l, st.light_d)
        else:
            ctx.save_for_backward(xyzs_l, ts_l, sigmas_l, albedo_l, rays_live, weights_sum, depth, image, embeddings, sigma_scale, *wb)
        if st.debug is not None:
            st.debug.update(rays=rays, rays_live=rays_live)
            if st.shading:
                st.debug.update(xyzs_live=xyzs_l, ts_live=ts_l, sigmas_live=sigmas_l, albedo_live=albedo_l, sigma_fd_live=sigma_fd_l)
        return weights_sum, depth, image

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_weights_sum, grad_depth, grad_image):
        xyzs, ts, sigmas, albedo, rays_live, weights_sum, depth, image, embeddings, sigma_scale, *wb = ctx.saved_tensors
        st, need = ctx.st, ctx.needs_input_grad
        if st.shading:
            *wb, sigma_fd, _ = wb                                           # the last one is st.light_d, kept alive with the graph
        spec, L = st.spec, _lib.lib()
        M, N, ch = xyzs.shape[0], rays_live.shape[0], spec.out_dim - 1
        n_in = 10 + len(wb)
        # the table gradient is added into, the others are overwritten (accumulate = 0), as in _NerfField.backward
        g_emb = torch.zeros_like(embeddings) if need[8] else None
        g_ss = torch.empty_like(sigma_scale) if (need[9] and spec.act == nerf.ACTIVATIONS['scaling']) else None
        g_wb = [torch.empty_like(t) if need[10 + i] else None for i, t in enumerate(wb)]
        out = (None,) * 8 + (g_emb, g_ss if need[9] else None, *g_wb)
        assert len(out) == n_in
        if g_emb is None and g_ss is None and all(t is None for t in g_wb):
            return out
        if M == 0:                                                          # no live sample: the kernels launch nothing
            for t in [g_ss] + g_wb:
                if t is not None:
                    t.zero_()
            return out

        def g(t, like):
            return torch.zeros_like(like) if t is None else t.float().contiguous()
        # 1. the composite backward over the live rows; its temporaries go before the field backward allocates its workspace
        if st.shading:                                                      # the colours of the live rows again: the forward's bits
            rgbs = torch.empty(M, ch, dtype=torch.float32, device=xyzs.device)
            _shade_train(L, st, sigma_fd, albedo, M, ch, rgbs, _lib.stream(xyzs))
        else:
            rgbs = albedo.float()
        grad_weights = torch.zeros(M, dtype=torch.float32, device=xyzs.device)
        grad_sigmas = torch.zeros(M, dtype=torch.float32, device=xyzs.device)
        grad_rgbs = torch.zeros(M, ch, dtype=torch.float32, device=xyzs.device)
        raymarch.composite_rays_train_backward_into(
            grad_weights, g(grad_weights_sum, weights_sum), g(grad_depth, depth), g(grad_image, image), sigmas, rgbs, ts, rays_live,
            weights_sum, depth, image, M, N, st.T_thresh, st.binarize, grad_sigmas, grad_rgbs, ch)
        del rgbs, grad_weights
        if st.debug is not None:
            st.debug.update(grad_sigmas_live=grad_sigmas, grad_rgbs_live=grad_rgbs)
        if st.shading:
            # 1b. the shade backward: d colour -> d of the six shifted densities, and the albedo's gradient where the shading reads it
            dsigma_fd = torch.empty(M, 6, dtype=torch.float32, device=xyzs.device)
            dalbedo = torch.empty(M, ch, dtype=albedo.dtype, device=xyzs.device) if st.shading == 3 else None
            _lib.check(L.dwg_nerf_train_shade_backward(
                st.shading, _lib.ptr(sigma_fd), _lib.ptr(albedo) if st.shading == 3 else None, int(albedo.dtype == torch.float16),
                _lib.ptr(st.light_d), ctypes.c_float(st.ratio), ctypes.c_float(st.eps), M, ch, _lib.ptr(grad_rgbs), _lib.ptr(dsigma_fd),
                _lib.ptr(dalbedo), _lib.stream(xyzs)), "dwg_nerf_train_shade_backward")
            if st.debug is not None:
                st.debug.update(dsigma_fd_live=dsigma_fd, dalbedo_live=dalbedo)
        else:
            dalbedo = grad_rgbs.to(albedo.dtype)
        del grad_rgbs
        # 2. the field backward over the live rows
        nerf.field_backward(spec, embeddings, sigma_scale, wb, xyzs, grad_sigmas, dalbedo, g_emb, g_ss, g_wb,
                            fd=(st.eps, dsigma_fd) if st.shading else None)
        return out


class _TrainSettings:
    pass


def render_rays_train(rays_o, rays_d, nears, fars, density_bitfield, cascade, grid_size, encoder, sigma_net, sigma_scale, bound, *,
                      density_activation, density_prior, albedo_sigmoid, perturb=True, noises=None, dt_gamma=0, max_steps=1024,
                      T_thresh=1e-4, binarize=False, contract=False, precision=None, counter=None, return_weights=False, return_sigmas=False,
                      return_stats=False, _debug=None, shading='albedo', light_d=None, ambient_ratio=1.0, epsilon=1e-3):
    """The training render (boundary B18): what the training branch of run_cuda computes for shading 'albedo'
    (core/nerf/nerf_renderer.py:334-349) -- raymarch.march_rays_train -> nerf.nerf_field -> raymarch.composite_rays_train -- as one
    autograd function that keeps, for the backward, only the samples the composite used.  A ray stops at the first sample after which
    T < T_thresh; the samples behind it get no weight and no gradient, so the composite backward and the field backward run over the
    M_live <= M live rows.

      -> weights_sum [N], depth [N], image [N, out_dim - 1]        fp32, bit-equal to the composition's; differentiable with respect to
         [, weights [M]] [, sigmas [M]]                             encoder.embeddings, sigma_net's parameters and sigma_scale (rays are
         [, {'M': int, 'M_live': int, 'live': int32 [N]}]           not differentiated).  The optional returns are not differentiable.

    rays_o / rays_d [N, 3], nears / fars [N] fp32 on the device, none requiring grad.  perturb / noises [N]: as march_rays_train (noises
    overrides the torch.rand(N) draw).  counter: an int32 device tensor whose first element the march adds M to (default: a private
    zero).  precision: None follows autocast, 0 f32, 1 f16.  Host reads: the march's read of M, and 4 bytes of M_live; the backward reads
    nothing.  Under no_grad / inference_mode, or when no parameter requires grad, nothing is gathered or saved.  The parameter gradients
    are the composition's up to the order of the fp32 sums over samples (with T_thresh = 0, where no sample is culled, bit-equal).

    shading 'normal' / 'textureless' / 'lambertian' (boundary B19): the colours come from the finite-difference normal with step epsilon
    (seven field evaluations per sample in one launch, dwg_nerf_field_forward_fd) and forward()'s shading with light_d [3] fp32 on the
    device (needed by the lambert shadings, never read on the host) and ambient_ratio; the backward goes through the shading and the
    normal into the six shifted densities (csrc/shade_math.h restates torch autograd there) and through the field at all seven point
    sets, over the live rows.  weights_sum, depth, weights, sigmas and live are the 'albedo' call's bits.  'lambertian' with a latent
    field is ill-formed in the reference and refused; the lambert shadings are refused in f16 (the reference's normal @ -l is a
    half-precision product under autocast, not restated); 'normal' runs in both precisions."""
    st = _TrainSettings()
    st.shading = SHADINGS.get(shading, 0)
    spec, emb_d, _, _, N, C, H = _check_render(
        rays_o, rays_d, nears, fars, density_bitfield, cascade, grid_size, max_steps, shading, light_d if st.shading >= 2 else None,
        ambient_ratio, epsilon, "epsilon", encoder, sigma_net, sigma_scale, bound, density_activation, density_prior, albedo_sigmoid, precision)
    wb = []
    for lin in sigma_net.net:
        wb += [lin.weight, lin.bias]
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d), ("nears", nears), ("fars", fars)):
        if t.requires_grad:
            raise RuntimeError("render_rays_train does not differentiate the rays: %s requires grad" % name)
    if N >= 1 << 31:
        raise RuntimeError("render_rays_train takes fewer than 2^31 rays")
    if st.shading >= 2 and spec.precision:
        raise RuntimeError("shading %r is not taken in f16: the reference's normal @ -l is a half-precision product there" % shading)
    dev = rays_o.device
    st.light_d, st.ratio, st.eps = light_d.detach() if st.shading >= 2 else None, float(ambient_ratio), float(epsilon)
    others = []
    if noises is not None:
        _lib.check_tensor("noises", noises, torch.float32, (N,))
        others.append(("noises", noises))
    if counter is not None:
        _lib.check_tensor("counter", counter, torch.int32, (None,))
        if counter.numel() < 1:
            raise RuntimeError("counter must hold at least one element")
        others.append(("counter", counter))
    _same_device(dev, others)
    st.spec, st.bound, st.C, st.H = spec, float(bound), C, H
    st.contract, st.dt_gamma, st.max_steps = bool(contract), float(dt_gamma), int(max_steps)
    st.T_thresh, st.binarize = float(T_thresh), bool(binarize)
    st.return_weights, st.return_sigmas, st.return_stats = bool(return_weights), bool(return_sigmas), bool(return_stats)
    st.debug = _debug
    ss = sigma_scale.reshape(1)
    # the saved state follows the CALLER's grad mode: inside Function.forward gradients are always off, and needs_input_grad does not
    # know about inference_mode
    st.keep = torch.is_grad_enabled() and any(t.requires_grad for t in [encoder.embeddings, ss] + wb)
    with torch.cuda.device(dev):
        if noises is None:
            noises = torch.rand(N, device=dev) if perturb else torch.zeros(N, device=dev)
        weights_sum, depth, image = _RenderRaysTrain.apply(st, rays_o, rays_d, nears, fars, density_bitfield, noises, counter,
                                                           encoder.embeddings, ss, *wb)
    out = [weights_sum, depth, image]
    if return_weights:
        out.append(st.weights)
    if return_sigmas:
        out.append(st.sigmas)
    if return_stats:
        out.append({'M': st.M, 'M_live': st.M_live, 'live': st.live})
    st.weights = st.sigmas = st.live = None
    return tuple(out)


def _covered_shading(ref, flag, shading, light_d, rays_o):
    """A bound network takes this shading: 'albedo' always; with the opt-in `flag` set on it also 'normal' and, without autocast only,
    'textureless' and rgb 'lambertian'.  A given light_d must be a [3] fp32 tensor on the rays' device."""
    if shading == 'albedo':
        return True
    if not getattr(ref, flag, False) or shading not in SHADINGS:
        return False
    if shading != 'normal' and torch.is_autocast_enabled():
        return False
    if shading == 'lambertian' and ref.sigma_net.net[-1].out_features - 1 != 3:
        return False
    return light_d is None or (isinstance(light_d, torch.Tensor) and light_d.dtype == torch.float32 and tuple(light_d.shape) == (3,)
                               and isinstance(rays_o, torch.Tensor) and light_d.device == rays_o.device)


def covered_call(ref, rays_o, rays_d, shading, perturb, light_d=None):
    """The native render takes this run_cuda call: evaluation mode, no perturbation, CUDA fp32 rays, the bitfield and the parameters on
    the device, and no autocast dtype but fp16.  shading 'albedo' always; with the network bound with shaded_render, also 'normal' (the
    reference's normal arithmetic is fp32 under fp16 autocast too: the field returns an fp32 density) and, without autocast only,
    'textureless' and 'lambertian' (under fp16 autocast the reference's normal @ -l is a half-precision matmul, not restated; latent
    'lambertian' is ill-formed).  A given light_d must be a [3] fp32 tensor on the rays' device."""
    if ref.training or perturb or not getattr(ref, "cuda_ray", False):
        return False
    return _covered_shading(ref, "_dwg_shaded_render", shading, light_d, rays_o) and _covered_state(ref, rays_o, rays_d)


def _covered_state(ref, rays_o, rays_d):
    """covered_call's conditions on the rays, the bitfield, the parameters and autocast (shared with covered_train_call)."""
    for t in (rays_o, rays_d):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            return False
    bits = getattr(ref, "density_bitfield", None)
    if not isinstance(bits, torch.Tensor) or not bits.is_cuda or bits.dtype != torch.uint8 or not bits.is_contiguous():
        return False
    C, H = ref.cascade, ref.grid_size
    if not (isinstance(C, int) and isinstance(H, int) and _grid_shape(C, H)):
        return False
    if bits.numel() * 8 != C * H ** 3 or ref.sigma_net.net[-1].out_features - 1 not in (3, 4):
        return False
    if not (ref.encoder.embeddings.is_cuda and ref.sigma_scale.is_cuda and all(p.is_cuda for p in ref.sigma_net.parameters())):
        return False
    return nerf.autocast_covered()


def covered_train_call(ref, rays_o, rays_d, shading, light_d=None):
    """The native training render takes this run_cuda call: the network bound with train_render, in training mode, shading 'albedo',
    rays that need no gradient, and covered_call's conditions on the rays, the bitfield, the parameters and autocast.  Bound with
    train_render='shaded' (B19) also the shadings covered_call takes for a shaded evaluation view, on the same terms: 'normal' always,
    'textureless' and rgb 'lambertian' without autocast, a given light_d a [3] fp32 tensor on the rays' device."""
    if not ref.training or not getattr(ref, "_dwg_train_render", False) or not getattr(ref, "cuda_ray", False):
        return False
    if not _covered_shading(ref, "_dwg_train_shaded", shading, light_d, rays_o):
        return False
    if not _covered_state(ref, rays_o, rays_d) or rays_o.requires_grad or rays_d.requires_grad:
        return False
    sc = getattr(ref, "step_counter", None)
    return isinstance(sc, torch.Tensor) and sc.is_cuda and sc.dtype == torch.int32 and sc.dim() == 2 and sc.shape[0] >= 16


def _safe_normalize(x, eps=1e-20):
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


def run_cuda(ref, orig, rays_o, rays_d, light_d=None, ambient_ratio=1.0, shading='albedo', perturb=False, dt_gamma=0, max_steps=1024,
             T_thresh=1e-4, **kwargs):
    """run_cuda of a bound network.  Calls the native renders do not take (perturb in evaluation, CPU, bf16 autocast; a shading other
    than 'albedo' unless the network was bound with shaded_render, see covered_call; a training call unless it was bound with
    train_render, a shaded one unless with train_render='shaded', see covered_train_call) go to `orig` unchanged.  The native branches keep the original's statements around the render:
    near_far_from_aabb with aabb_infer (aabb_train in training), the light_d draw (it consumes the device generator as the original
    does), in training the step counter's statements, the reshapes and mask = nears < fars.  Evaluation: results['xyzs'], ['sigmas'] and
    ['rgbs'] -- in the original the last loop iteration's leftovers, read by nothing outside training -- are None.  Training
    (render_rays_train, B18): results['weights'] and ['sigmas'] are the full [M] arrays, detached; ['xyzs'] and ['rgbs'] are None; the
    march adds its sample count into the step counter's row."""
    train = covered_train_call(ref, rays_o, rays_d, shading, light_d) and (shading == 'albedo' or isinstance(ambient_ratio, (int, float)))
    if not train and (not covered_call(ref, rays_o, rays_d, shading, perturb, light_d) or not isinstance(ambient_ratio, (int, float))):
        return orig(rays_o, rays_d, light_d=light_d, ambient_ratio=ambient_ratio, shading=shading, perturb=perturb, dt_gamma=dt_gamma,
                    max_steps=max_steps, T_thresh=T_thresh, **kwargs)
    prefix = rays_o.shape[:-1]
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)

    # pre-calculate near far
    nears, fars = ref.raymarching.near_far_from_aabb(rays_o, rays_d, ref.aabb_train if train else ref.aabb_infer)
    return run_cuda_native(ref, train, prefix, rays_o, rays_d, nears, fars, light_d, ambient_ratio, shading, perturb, dt_gamma, max_steps,
                           T_thresh)


def run_cuda_native(ref, train, prefix, rays_o, rays_d, nears, fars, light_d, ambient_ratio, shading, perturb, dt_gamma, max_steps, T_thresh,
                    noises=None):
    """run_cuda's native branches behind near_far_from_aabb: rays_o / rays_d [N, 3] and nears / fars [N] as that statement leaves them
    (nerf_view.render_view gets all four from one launch).  train: the training render (covered_train_call held), else the evaluation
    render (covered_call held).  noises [N]: the training march's perturbation instead of its torch.rand(N) draw."""
    device = rays_o.device

    # random sample light_d if not provided
    if light_d is None:
        light_d = (rays_o[0] + torch.randn(3, device=device, dtype=torch.float))
        light_d = _safe_normalize(light_d)

    latent = bool(getattr(ref, "latent_mode", False))
    field = (ref.density_bitfield, ref.cascade, ref.grid_size, ref.encoder, ref.sigma_net, ref.sigma_scale, ref.bound)
    results = {}
    xyzs, sigmas = None, None
    if train:
        # setup counter
        counter = ref.step_counter[ref.local_step % 16]
        counter.zero_()  # set to 0
        ref.local_step += 1

        weights_sum, depth, image, weights, sigmas = render_rays_train(
            rays_o, rays_d, nears.float().contiguous(), fars.float().contiguous(), *field, density_activation=ref.opt.density_activation,
            density_prior=ref.density_prior_type, albedo_sigmoid=not latent, perturb=perturb, dt_gamma=dt_gamma, max_steps=max_steps,
            T_thresh=T_thresh, counter=counter, return_weights=True, return_sigmas=True, noises=noises,
            **({} if shading == 'albedo' else dict(shading=shading, light_d=light_d.contiguous(), ambient_ratio=ambient_ratio)))
        results['weights'] = weights
    else:
        weights_sum, depth, image = render_rays(
            rays_o, rays_d, nears.float().contiguous(), fars.float().contiguous(), *field, density_activation=ref.opt.density_activation,
            density_prior=ref.density_prior_type, albedo_sigmoid=not latent, dt_gamma=dt_gamma, max_steps=max_steps, T_thresh=T_thresh,
            shading=shading, light_d=light_d.contiguous() if shading != 'albedo' else None, ambient_ratio=ambient_ratio)

    results['image'] = image.reshape(*prefix, image.shape[-1])
    results['depth'] = depth.reshape(*prefix)
    results['weights_sum'] = weights_sum.reshape(*prefix)
    results['mask'] = (nears < fars).reshape(*prefix)
    results['xyzs'] = xyzs
    results['sigmas'] = sigmas
    results['rgbs'] = None
    return results
