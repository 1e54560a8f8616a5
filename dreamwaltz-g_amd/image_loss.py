"""The image loss of the nerf2gs loop on the device (boundary B17): `ImageReconstructionLoss`, `ssim` and `l1_loss` of the reference's
core/gaussian/gaussian_loss.py:9-60,131-138 -- 0.8 L1 + 0.2 (1 - SSIM), 11 x 11 Gaussian window, sigma 1.5, zero padding -- as one forward and
one backward call of csrc/image_loss.hip (include/dwg_image_loss.h), and `nerf2gs_forward`, Trainer.pretrain_nerf2gs_forward
(core/trainer.py:1370-1386) over them.

Images are [B, C, H, W] (or [C, H, W]) fp32 tensors of ANY strides: the kernels read them in place, so the [B, H, W, C] renders of Scene and
of the NeRF go in as `.permute(0, 3, 1, 2)` views, without the reference's `.contiguous()` copy, and the gradient comes back in the
first image's layout.

What differs from the reference, deliberately:
  * only the first image is differentiated; a second image that requires grad raises (in the loop it is the no_grad teacher render);
  * only window_size 11 and fp32;
  * the filter and the SSIM map are accumulated in fp64; the results are fp32 scalars.
There is no CPU fallback: CPU tensors raise."""

import torch

from . import _lib

WINDOW_SIZE, MAX_SIZE, MAX_PLANES = (_lib.CONSTANTS["DWG_IMAGE_LOSS_" + n] for n in ("WINDOW", "MAX_SIZE", "MAX_PLANES"))
_ws = {}
# what the forward kept for a backward: tests read it, nothing else does.  `maps_allocations` counts the derivative-map tensors ever
# allocated, `last_maps_bytes` is the size of the one the LAST forward allocated (0: it stored none)
stats = {"forward_calls": 0, "maps_allocations": 0, "last_maps_bytes": 0}


def _workspace(device, B, C, H, W):
    need = max(int(_lib.lib().dwg_image_loss_workspace_bytes(B, C, H, W)), 16)
    key = str(device)
    if key not in _ws or _ws[key].numel() < need:
        _ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return _ws[key]


def _image_args(t):
    return (_lib.ptr(t),) + tuple(int(s) for s in t.stride())


class _ImageLossFn(torch.autograd.Function):
    """kind: 'loss' | 'l1' | 'ssim' (a scalar each) | 'ssim_batch' ([B]).  keep: store the derivative maps for a backward."""

    @staticmethod
    def forward(ctx, x, y, lambda_dssim, kind, keep):
        dev = x.device
        B, C, H, W = x.shape
        ws = _workspace(dev, B, C, H, W)
        scalars = torch.empty(3, dtype=torch.float32, device=dev)
        per_item = torch.empty(B, dtype=torch.float32, device=dev) if kind == 'ssim_batch' else None
        maps = None
        if keep and kind != 'l1':
            maps = torch.empty((3, B, C, H, W), dtype=torch.float32, device=dev)
            stats["maps_allocations"] += 1
        stats["forward_calls"] += 1
        stats["last_maps_bytes"] = 0 if maps is None else maps.numel() * 4
        p = _lib.ptr
        _lib.check(_lib.lib().dwg_image_loss_forward(B, C, H, W, WINDOW_SIZE, float(lambda_dssim), *_image_args(x), *_image_args(y), p(scalars),
                                                     p(per_item), p(maps), p(ws), ws.numel(), _lib.stream(dev)), "dwg_image_loss_forward")
        ctx.kind, ctx.lambda_dssim, ctx.keep = kind, float(lambda_dssim), keep
        if keep:
            ctx.save_for_backward(x, y, maps)
        if kind == 'ssim_batch':
            return per_item
        return scalars[{'loss': 0, 'l1': 1, 'ssim': 2}[kind]].reshape(())

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if not ctx.keep:
            raise RuntimeError("dreamwaltz_g_amd.image_loss: this forward ran with gradients disabled and kept nothing for a backward")
        x, y, maps = ctx.saved_tensors
        B, C, H, W = x.shape
        n = float(B * C * H * W)
        lam = ctx.lambda_dssim
        coef_ssim, coef_l1 = {'loss': (-(lam / n), (1.0 - lam) / n), 'l1': (0.0, 1.0 / n), 'ssim': (1.0 / n, 0.0),
                              'ssim_batch': (1.0 / float(C * H * W), 0.0)}[ctx.kind]
        g = grad_out.detach().reshape(-1).float().contiguous()
        grad_x = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
        p = _lib.ptr
        _lib.check(_lib.lib().dwg_image_loss_backward(B, C, H, W, WINDOW_SIZE, coef_ssim, coef_l1, *_image_args(x), *_image_args(y), p(maps), p(g),
                                                      int(ctx.kind == 'ssim_batch'), p(grad_x), _lib.stream(x.device)), "dwg_image_loss_backward")
        return grad_x, None, None, None, None


def _call(image, gt_image, lambda_dssim, kind, window_size=WINDOW_SIZE):
    """Every refusal happens here, before the library is touched."""
    if not (torch.is_tensor(image) and torch.is_tensor(gt_image)):
        raise TypeError("images are torch tensors")
    if image.dtype != torch.float32 or gt_image.dtype != torch.float32:
        raise TypeError("images are float32; got %s and %s" % (image.dtype, gt_image.dtype))
    if window_size != WINDOW_SIZE:
        raise ValueError("window_size is %d; got %r" % (WINDOW_SIZE, window_size))
    if image.shape != gt_image.shape or image.dim() not in (3, 4) or image.numel() == 0:
        raise ValueError("images are two non-empty [B, C, H, W] or [C, H, W] tensors of one shape; got %s and %s"
                         % (tuple(image.shape), tuple(gt_image.shape)))
    if gt_image.requires_grad:
        raise RuntimeError("the second image is the target: it gets no gradient (detach it)")
    # the device check comes after the checks a host without a GPU can exercise, and before anything reads a pointer
    if not (image.is_cuda and gt_image.is_cuda):
        raise RuntimeError("dreamwaltz_g_amd.image_loss runs on the GPU only (HIP kernels); got a CPU tensor")
    if image.dim() == 3:
        if kind == 'ssim_batch':
            raise ValueError("size_average=False needs a batch dimension; got %s" % (tuple(image.shape),))
        image, gt_image = image.unsqueeze(0), gt_image.unsqueeze(0)
    B, C, H, W = image.shape
    if H > MAX_SIZE or W > MAX_SIZE or B * C > MAX_PLANES:
        raise ValueError("image of shape %s: at most %d x %d pixels and %d planes" % (tuple(image.shape), MAX_SIZE, MAX_SIZE, MAX_PLANES))
    if any(n > 1 and s == 0 for n, s in zip(image.shape, image.stride())):
        image = image.contiguous()                      # an expanded tensor has no layout a gradient could be written in
    # the saved state follows the CALLER's grad mode: inside Function.forward gradients are always off, and needs_input_grad does not
    # know about inference_mode
    keep = torch.is_grad_enabled() and image.requires_grad
    return _ImageLossFn.apply(image, gt_image.detach(), lambda_dssim, kind, keep)


def l1_loss(network_output, gt):
    """mean |network_output - gt| (gaussian_loss.py:9-10).  It runs the whole forward kernel; the loop's loss is ImageReconstructionLoss."""
    return _call(network_output, gt, 0.0, 'l1')


def ssim(img1, img2, window_size=11, size_average=True):
    """gaussian_loss.py:29-60: the mean of the SSIM map, or one mean per batch item ([B]) with size_average=False."""
    return _call(img1, img2, 0.0, 'ssim' if size_average else 'ssim_batch', window_size=window_size)


class ImageReconstructionLoss:
    """gaussian_loss.py:131-138: (1 - lambda_dssim) * l1_loss + lambda_dssim * (1 - ssim), one forward and one backward call."""

    def __init__(self, lambda_dssim: float = 0.2):
        if not 0.0 <= float(lambda_dssim) <= 1.0:
            raise ValueError("lambda_dssim is a weight in [0, 1]; got %r" % (lambda_dssim,))
        self.lambda_dssim = lambda_dssim

    def __call__(self, image: torch.Tensor, gt_image: torch.Tensor):
        return _call(image, gt_image, self.lambda_dssim, 'loss')


_default_loss = ImageReconstructionLoss()


def nerf2gs_forward(trainer, data):
    """Trainer.pretrain_nerf2gs_forward (trainer.py:1370-1386) -> (loss, render_outputs, nerf_outputs): the avatar's render against the
    NeRF's albedo render of the same camera (no_grad), both `image_fg` [B, H, W, C] read in place."""
    render_outputs = trainer.render(data=data)
    render_image = render_outputs['image_fg']
    if not render_image.is_cuda:
        raise RuntimeError("dreamwaltz_g_amd.image_loss runs on the GPU only (HIP kernels); got a CPU render")
    with torch.no_grad():
        nerf_outputs = trainer.nerf_guidance.render(data=data, shading='albedo')
        nerf_image = nerf_outputs['image_fg']
    loss_fn = getattr(trainer, 'losses', None)
    loss_fn = loss_fn.get('image') if isinstance(loss_fn, dict) else None
    if not isinstance(loss_fn, ImageReconstructionLoss):
        loss_fn = _default_loss                          # the reference's own object would copy both images and run its conv2d composition
    loss = loss_fn(render_image.permute(0, 3, 1, 2), nerf_image.permute(0, 3, 1, 2).float())
    return loss, render_outputs, nerf_outputs
