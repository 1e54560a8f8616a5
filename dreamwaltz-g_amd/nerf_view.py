"""MI355X-native view around the NeRF stage's render (boundary B20): what the reference's _NeRFRenderer.render
(core/nerf/nerf_renderer.py:404-472) does before and after run_cuda, and SparsityLoss (core/nerf/nerf_loss.py:17-56), on
csrc/nerf_view.hip through include/dwg_nerf_view.h.

  view_rays(c2w, intrinsics, H, W, aabb)      get_rays (N = -1) + near_far_from_aabb in one launch, the camera read on the device
  view_compose(image_fg, weights_sum, bg, ..)  the background mix written planar ([1, C, H, W], what the guidance takes) and the
                                               sparsity loss of weights_sum, one autograd function; backward in one launch
  SparsityLoss(cfg)                            the reference's fields and schedule; the loss itself is the fused one
  render_view(net, data, shading, bg_mode)     render() of a cuda_ray network: rays -> nerf_render.run_cuda_native -> the background
                                               (the learned 'nerf' one through nerf_background.learned_background, B22) -> compose
  covered_view(ref, data, ...)                 which render() calls of a bound reference network render_view takes

No CPU fallback; every tensor is checked (CUDA, fp32, shape, contiguity) and a violation raises RuntimeError before any launch.
"""
import ctypes
from random import random

import torch
from torch.autograd import Function

from . import _lib
from . import nerf_background
from . import nerf_render

_C = _lib.CONSTANTS
BG_NONE, BG_CONSTANT, BG_IMAGE, MAX_SIZE = _C["DWG_VIEW_BG_NONE"], _C["DWG_VIEW_BG_CONSTANT"], _C["DWG_VIEW_BG_IMAGE"], _C["DWG_VIEW_MAX_SIZE"]


def _image_size(H, W):
    if int(H) != H or int(W) != W or not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE) or H * W >= 1 << 31:
        raise RuntimeError("bad image size %r x %r (1..%d each, fewer than 2^31 pixels)" % (H, W, MAX_SIZE))
    return int(H), int(W)


def _one_camera(name, t, tail):
    """[*tail] or [1, *tail] -> the tensor; a batch of several cameras is refused (run_cuda assumes B == 1)."""
    if isinstance(t, torch.Tensor) and t.dim() == len(tail) + 1:
        if t.shape[0] != 1:
            raise RuntimeError("%s holds %d cameras: the view takes one camera per call (B == 1)" % (name, t.shape[0]))
        t = t[0]
    return t


def view_rays(c2w, intrinsics, H, W, aabb, min_near=0.2):
    """get_rays(c2w, intrinsics, H, W) with N = -1 (core/nerf/nerf_utils.py:72-137) and near_far_from_aabb on its rays, one launch.

    c2w [4, 4] or [1, 4, 4], intrinsics [3, 3] or [1, 3, 3], aabb [6]: fp32 on the device, read there (nothing about the camera is a
    host value).  -> rays_o, rays_d [1, H W, 3], nears, fars [H W]; pixel p = row * W + col.  nears / fars are the bits of
    raymarch.near_far_from_aabb on the returned rays.  Not differentiable."""
    H, W = _image_size(H, W)
    c2w = _one_camera("c2w", c2w, (4, 4))
    intrinsics = _one_camera("intrinsics", intrinsics, (3, 3))
    _lib.check_tensor("c2w", c2w, shape=(4, 4))
    _lib.check_tensor("intrinsics", intrinsics, shape=(3, 3))
    _lib.check_tensor("aabb", aabb, shape=(6,))
    dev = c2w.device
    for name, t in (("intrinsics", intrinsics), ("aabb", aabb)):
        if t.device != dev:
            raise RuntimeError("%s is on %s, c2w on %s" % (name, t.device, dev))
    N = H * W
    rays_o = torch.empty((1, N, 3), dtype=torch.float32, device=dev)
    rays_d = torch.empty((1, N, 3), dtype=torch.float32, device=dev)
    nears = torch.empty(N, dtype=torch.float32, device=dev)
    fars = torch.empty(N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().dwg_nerf_view_rays(_lib.ptr(c2w.detach()), _lib.ptr(intrinsics.detach()), _lib.ptr(aabb.detach()), H, W,
                                                 ctypes.c_float(min_near), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(nears), _lib.ptr(fars),
                                                 _lib.stream(c2w)), "dwg_nerf_view_rays")
    return rays_o, rays_d, nears, fars


class SparsityLoss:
    """The reference's SparsityLoss (core/nerf/nerf_loss.py:30-56): its constructor fields and its schedule.  terms() gives what the
    fused kernels take; calling it evaluates the loss of pred_ws on the device (view_compose without an image)."""

    def __init__(self, cfg, use_schedule: bool = True) -> None:
        self.lambda_opacity = cfg.lambda_opacity
        self.lambda_entropy = cfg.lambda_entropy
        self.lambda_emptiness = cfg.lambda_emptiness
        self.use_schedule = use_schedule
        self.sparsity_multiplier = cfg.sparsity_multiplier
        self.sparsity_step = cfg.sparsity_step
        self.available = self.lambda_opacity > 0.0 or self.lambda_entropy > 0.0 or self.lambda_emptiness > 0.0

    def terms(self, current_step=None, max_iteration=None):
        """(lambda_opacity, lambda_entropy, lambda_emptiness, multiplier) of this step."""
        mult = 1.0
        if self.use_schedule and current_step / max_iteration >= self.sparsity_step:
            mult = self.sparsity_multiplier
        return (float(self.lambda_opacity), float(self.lambda_entropy), float(self.lambda_emptiness), float(mult))

    def __call__(self, pred_ws, current_step=None, max_iteration=None):
        if not self.available:
            return 0.0
        return view_compose(None, pred_ws, None, 1, pred_ws.numel(), sparsity=self.terms(current_step, max_iteration))[1]


class _Settings:
    pass


class _ViewCompose(Function):
    @staticmethod
    def forward(ctx, st, image_fg, weights_sum, bg):
        L = _lib.lib()
        dev = weights_sum.device
        N, C, co = st.N, st.C, st.channels_out
        image = torch.empty((1, co, st.H, st.W), dtype=torch.float32, device=dev) if image_fg is not None else None
        loss = torch.zeros((), dtype=torch.float32, device=dev) if st.sparsity is None else torch.empty((), dtype=torch.float32, device=dev)
        nbytes = int(L.dwg_nerf_view_compose_workspace_bytes(N))
        ws_buf = torch.empty(nbytes // 8, dtype=torch.float64, device=dev) if st.sparsity is not None else None
        lam = st.sparsity if st.sparsity is not None else (0.0, 0.0, 0.0, 1.0)
        with torch.cuda.device(dev):
            _lib.check(L.dwg_nerf_view_compose_forward(N, C, co, _lib.ptr(image_fg), _lib.ptr(weights_sum), _lib.ptr(bg), st.bg_mode, lam[0],
                                                       lam[1], lam[2], lam[3], _lib.ptr(image), _lib.ptr(loss) if st.sparsity is not None else None,
                                                       _lib.ptr(ws_buf), nbytes if ws_buf is not None else 0, _lib.stream(weights_sum)),
                       "dwg_nerf_view_compose_forward")
        ctx.st = st
        if st.keep:
            ctx.save_for_backward(weights_sum, bg, ws_buf)
        if st.sparsity is None:
            ctx.mark_non_differentiable(loss)
        if image is None:
            image = torch.zeros((), dtype=torch.float32, device=dev)
            ctx.mark_non_differentiable(image)
        return image, loss

    @staticmethod
    def backward(ctx, d_image, d_loss):
        st = ctx.st
        if not st.keep:
            raise RuntimeError("view_compose was called with gradients off: nothing was saved for a backward")
        weights_sum, bg, ws_buf = ctx.saved_tensors
        L = _lib.lib()
        dev = weights_sum.device
        N, C = st.N, st.C
        has_image = st.has_image
        d_image = d_image.contiguous().float() if has_image else None
        d_loss = d_loss.contiguous().float() if st.sparsity is not None else None
        d_fg = torch.empty((N, C), dtype=torch.float32, device=dev) if has_image and ctx.needs_input_grad[1] else None
        d_ws = torch.empty(N, dtype=torch.float32, device=dev)
        d_bg = (torch.empty((N, C), dtype=torch.float32, device=dev)
                if st.bg_mode == BG_IMAGE and ctx.needs_input_grad[3] else None)
        lam = st.sparsity if st.sparsity is not None else (0.0, 0.0, 0.0, 1.0)
        with torch.cuda.device(dev):
            _lib.check(L.dwg_nerf_view_compose_backward(N, C, st.channels_out, _lib.ptr(d_image), _lib.ptr(d_loss), _lib.ptr(weights_sum),
                                                        _lib.ptr(bg), st.bg_mode, int(st.detach_ws), lam[0], lam[1], lam[2], lam[3],
                                                        _lib.ptr(ws_buf), ws_buf.numel() * 8 if ws_buf is not None else 0, _lib.ptr(d_fg),
                                                        _lib.ptr(d_ws), _lib.ptr(d_bg), _lib.stream(weights_sum)), "dwg_nerf_view_compose_backward")
        return (None, d_fg.view(st.fg_shape) if d_fg is not None else None, d_ws.view(st.ws_shape) if ctx.needs_input_grad[2] else None,
                d_bg.view(st.bg_shape) if d_bg is not None else None)


def view_compose(image_fg, weights_sum, background, H, W, *, detach_ws=False, channels_out=None, sparsity=None):
    """The tail of render() (nerf_renderer.py:437-470) in the layout the guidance takes, and the sparsity loss, as one autograd function.

    image_fg [..., C] with H W pixels (C = 3, or 4 in latent mode), weights_sum with H W elements, fp32 contiguous on the device.
    background: None (image = image_fg[..., :channels_out], the 'normal' shading's branch), a colour [C], or a per-pixel image
    [..., C] with H W pixels (differentiable).  detach_ws: the mix does not differentiate weights_sum (detach_bg_weights_sum).
    channels_out (default C): the leading channels written.  sparsity: None, or (lambda_opacity, lambda_entropy, lambda_emptiness,
    multiplier) as SparsityLoss.terms gives them.
      -> image_nchw [1, channels_out, H, W] = image_fg + (1 - weights_sum) * background, every operation rounded on its own,
         sparsity_loss: a 0-dim fp32 tensor, or None without `sparsity`.
    image_fg None: only the loss is computed (image_nchw is None); H W is then just the element count of weights_sum and the per-side
    limit of an image does not apply.  It follows the caller's grad mode: under no_grad, or when no input
    requires grad, nothing is saved."""
    if image_fg is None:
        # the loss alone has no image: only the element count matters (H = 1, W = N for any N below 2^31)
        if int(H) != H or int(W) != W or H < 1 or W < 1 or H * W >= 1 << 31:
            raise RuntimeError("bad element count %r x %r (at least 1, fewer than 2^31)" % (H, W))
        H, W = int(H), int(W)
    else:
        H, W = _image_size(H, W)
    N = H * W
    st = _Settings()
    if not isinstance(weights_sum, torch.Tensor) or weights_sum.numel() != N:
        raise RuntimeError("weights_sum must be a tensor of H * W = %d elements" % N)
    st.has_image = image_fg is not None
    if st.has_image and (not isinstance(image_fg, torch.Tensor) or image_fg.dim() < 1 or image_fg.shape[-1] not in (3, 4)
                         or image_fg.numel() != N * image_fg.shape[-1]):
        raise RuntimeError("image_fg must be a tensor [..., C] of H * W = %d pixels with C = 3 or 4" % N)
    _lib.check_tensor("weights_sum", weights_sum)
    dev = weights_sum.device
    if st.has_image:
        _lib.check_tensor("image_fg", image_fg)
        C = int(image_fg.shape[-1])
        if image_fg.device != dev:
            raise RuntimeError("image_fg is on %s, weights_sum on %s" % (image_fg.device, dev))
        if image_fg.data_ptr() % 16:
            raise RuntimeError("image_fg must be 16-byte aligned")
    else:
        if background is not None or channels_out is not None:
            raise RuntimeError("without image_fg there is nothing to mix: background and channels_out must be None")
        C = 3
    co = C if channels_out is None else channels_out
    if int(co) != co or not 1 <= co <= C:
        raise RuntimeError("channels_out must lie in 1..%d, got %r" % (C, channels_out))
    if background is None:
        st.bg_mode = BG_NONE
    else:
        if not isinstance(background, torch.Tensor):
            raise RuntimeError("background must be None or a tensor, got %s" % type(background).__name__)
        if background.numel() == C and background.dim() == 1:
            st.bg_mode = BG_CONSTANT
        elif background.dim() >= 1 and background.shape[-1] == C and background.numel() == N * C:
            st.bg_mode = BG_IMAGE
        else:
            raise RuntimeError("background must be a colour [%d] or an image [..., %d] of %d pixels, got %s" % (C, C, N, tuple(background.shape)))
        _lib.check_tensor("background", background)
        if background.device != dev:
            raise RuntimeError("background is on %s, weights_sum on %s" % (background.device, dev))
        if st.bg_mode == BG_IMAGE and background.data_ptr() % 16:
            raise RuntimeError("background must be 16-byte aligned")
    if sparsity is not None:
        sparsity = tuple(float(v) for v in sparsity)
        if len(sparsity) != 4 or any(v != v for v in sparsity):
            raise RuntimeError("sparsity must be (lambda_opacity, lambda_entropy, lambda_emptiness, multiplier), got %r" % (sparsity,))
    st.N, st.C, st.H, st.W, st.channels_out, st.detach_ws, st.sparsity = N, C, H, W, int(co), bool(detach_ws), sparsity
    st.fg_shape = image_fg.shape if st.has_image else None
    st.ws_shape, st.bg_shape = weights_sum.shape, (background.shape if background is not None else None)
    # the saved state follows the CALLER's grad mode (inside Function.forward gradients are always off)
    st.keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (image_fg, weights_sum, background))
    image, loss = _ViewCompose.apply(st, image_fg, weights_sum, background)
    return (image if st.has_image else None), (loss if sparsity is not None else None)


# ------------------------------------------------------------------------------------------------------------------------------------
# render()
# ------------------------------------------------------------------------------------------------------------------------------------
def _camera_ok(t, tail):
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (1,) + tuple(tail)
            and not t.requires_grad)


def _learned_background_reason(net, device=None):
    """None when the learned 'nerf' background of this network is built natively (boundary B22), else why not: a bg_net whose `.net` holds
    supported biased nn.Linear layers (on `device`), an encoder_bg of 3 inputs with a supported degree, and no decoder_layer."""
    if getattr(net, "bg_net", None) is None:
        return "the network has no bg_net"
    if getattr(net, "decoder_layer", None) is not None:
        return "a decoder_layer is not covered"
    return nerf_background.unsupported_reason(getattr(net, "encoder_bg", None), net.bg_net, device)


def covered_view(ref, data, shading='albedo', bg_mode=None, staged=False, light_d=None, ambient_ratio=1.0):
    """render_view takes this render() call of a network: cuda_ray (no dmtet, not staged), one fp32 camera on the device, a background
    mode it builds -- the learned 'nerf' one only with a bg_net and encoder_bg the kernels take (_learned_background_reason) --, and a
    run_cuda call the native renders take (nerf_render.covered_train_call in training, covered_call in evaluation: shading, autocast,
    the bitfield and the parameters on the device).  Decided before anything is drawn."""
    if getattr(ref, "dmtet", False) or not getattr(ref, "cuda_ray", False) or staged:
        return False
    try:
        c2w, intrinsics = data['c2w'], data['intrinsics']
        H, W = data['image_height'], data['image_width']
    except (KeyError, TypeError):
        return False
    if not _camera_ok(c2w, (4, 4)) or not _camera_ok(intrinsics, (3, 3)) or c2w.device != intrinsics.device:
        return False
    if not isinstance(H, int) or not isinstance(W, int) or not (1 <= H <= MAX_SIZE and 1 <= W <= MAX_SIZE):
        return False
    mode = ref.bg_mode if bg_mode is None else bg_mode
    if shading != 'normal':                           # shading 'normal' never asks for a background
        if mode == 'nerf':
            if _learned_background_reason(ref, c2w.device) is not None:
                return False
        elif mode not in ('none', None, 'disable', 'zero', 'zeros', 'normal', 'uniform') and mode not in getattr(ref, "bg_colors", {}):
            return False
    if not isinstance(ambient_ratio, (int, float)):
        return False
    aabb = ref.aabb_train if ref.training else ref.aabb_infer
    if not (isinstance(aabb, torch.Tensor) and aabb.device == c2w.device and aabb.dtype == torch.float32 and tuple(aabb.shape) == (6,)):
        return False
    # the rays will be fp32 tensors on the camera's device that need no gradient: the camera stands in for them
    if ref.training:
        return nerf_render.covered_train_call(ref, c2w, c2w, shading, light_d)
    return nerf_render.covered_call(ref, c2w, c2w, shading, False, light_d)


def render_view(net, data, shading='albedo', bg_mode=None, *, sparsity=None, noises=None, light_d=None, ambient_ratio=1.0, dt_gamma=0,
                max_steps=1024, T_thresh=1e-4, **kwargs):
    """_NeRFRenderer.render (nerf_renderer.py:404-472) of a cuda_ray network: view_rays, nerf_render.run_cuda_native's branches
    (render_rays_train in training, render_rays in evaluation), the background's statements, view_compose.

    data: 'c2w' [1, 4, 4], 'intrinsics' [1, 3, 3] (fp32 on the device), 'image_height', 'image_width'.  Returns the reference's keys with
    its shapes -- image [1, H, W, C], depth / mask / weights_sum / alpha [1, H, W, 1], image_bg / image_fg (when a background is mixed),
    weights, sigmas, xyzs, rgbs -- and image_nchw [1, C, H, W], the planar buffer the guidance takes.  image is the [1, H, W, C] view of
    that buffer: it is NOT contiguous, and image.permute(0, 3, 1, 2).contiguous() is image_nchw itself.  sparsity: SparsityLoss.terms
    of this step; the fused loss comes back as 'sparsity_loss'.  noises [H W]: the training march's perturbation instead of its draw.

    The host and device generators are consumed as the reference consumes them: run_cuda's light_d draw, the march's perturbation,
    rand_bg_prob's random(), 'uniform''s torch.rand(img_dims), 'normal''s randn_like.  The learned 'nerf' background
    (nerf_background.learned_background of the rays' directions) needs a network with a bg_net and encoder_bg the kernels take and no
    decoder_layer: otherwise NotImplementedError.  A call the native renders do not take (nerf_render.covered_train_call / covered_call) is an error here; a
    bound reference network sends such calls to its original method instead (covered_view)."""
    if kwargs.pop('staged', False):
        raise RuntimeError("render_view does not stage: cuda_ray never does")
    kwargs.pop('perturb', None)                       # render() sets it from the training flag
    if kwargs:
        raise RuntimeError("render_view does not take %s" % ", ".join(sorted(kwargs)))
    if getattr(net, "dmtet", False) or not getattr(net, "cuda_ray", False):
        raise RuntimeError("render_view renders a cuda_ray network (dmtet and run() without cuda_ray are not covered)")
    c2w = data['c2w']
    intrinsics = data['intrinsics']
    H = data['image_height']
    W = data['image_width']
    train = bool(net.training)
    mode_now = net.bg_mode if bg_mode is None else bg_mode
    if shading != 'normal' and mode_now == 'nerf' and _learned_background_reason(net) is not None:
        raise NotImplementedError("the learned 'nerf' background is not built natively")

    # rays_o, rays_d: [B, N, 3], assumes B == 1
    rays_o, rays_d, nears, fars = view_rays(c2w, intrinsics, H, W, net.aabb_train if train else net.aabb_infer)
    perturb = train
    ro, rd = rays_o.view(-1, 3), rays_d.view(-1, 3)
    if train:
        if not (nerf_render.covered_train_call(net, ro, rd, shading, light_d) and isinstance(ambient_ratio, (int, float))):
            raise RuntimeError("the native training render does not take this call (shading %r; see nerf_render.covered_train_call)" % (shading,))
    elif not (nerf_render.covered_call(net, ro, rd, shading, perturb, light_d) and isinstance(ambient_ratio, (int, float))):
        raise RuntimeError("the native evaluation render does not take this call (shading %r; see nerf_render.covered_call)" % (shading,))
    results = nerf_render.run_cuda_native(net, train, rays_o.shape[:-1], ro, rd, nears, fars, light_d, ambient_ratio, shading, perturb,
                                          dt_gamma, max_steps, T_thresh, noises=noises)

    # Reshape
    B = rays_o.shape[0]
    image_fg = results['image'].reshape(B, H, W, -1)
    results['depth'] = results['depth'].reshape(B, H, W, 1)
    results['mask'] = results['mask'].reshape(B, H, W, 1)
    results['weights_sum'] = results['weights_sum'].reshape(B, H, W, 1)
    results['alpha'] = results['weights_sum']

    if shading == 'normal':
        image_bg, channels_out = None, 3
    else:
        # mix background color
        image_bg, channels_out = _background(net, image_fg, bg_mode, rays_d), None
        if image_bg is not None:
            results['image_bg'] = image_bg.expand_as(image_fg)
            results['image_fg'] = image_fg
    image_nchw, loss = view_compose(image_fg, results['weights_sum'], image_bg, H, W, detach_ws=bool(net.opt.detach_bg_weights_sum),
                                    channels_out=channels_out, sparsity=sparsity)
    results['image_nchw'] = image_nchw
    results['image'] = image_nchw.permute(0, 2, 3, 1)
    if sparsity is not None:
        results['sparsity_loss'] = loss
    return results


def _background(net, image, bg_mode, rays_d):
    """_NeRFNetwork.background (core/nerf/nerf_model.py:107-144): None, a colour [C] or an image like `image`, with the reference's
    draws.  rays_d [B, H W, 3]: read by the learned mode."""
    if bg_mode is None:
        bg_mode = net.bg_mode

    # use random background color with probability random_aug_prob
    if net.training and net.rand_bg_prob is not None:
        if random() < net.rand_bg_prob:
            bg_mode = 'gray'

    if bg_mode in ('none', None, 'disable'):
        return None
    elif bg_mode in ('zero', 'zeros'):
        return torch.zeros(image.shape[-1], dtype=image.dtype, device=image.device)
    elif bg_mode == 'normal':
        return torch.randn_like(image)
    elif bg_mode == 'uniform':
        return torch.rand(net.img_dims).to(image).contiguous()
    elif bg_mode == 'nerf':
        h = nerf_background.learned_background(rays_d.view(-1, 3), net.encoder_bg, net.bg_net, sigmoid=not net.latent_mode)
        return h.reshape(image.shape)
    return net.bg_colors[bg_mode].to(image).contiguous()
