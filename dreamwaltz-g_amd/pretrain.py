"""The NeRF pretrain step of scripts/pretrain_nerf.sh on the device (boundary B9): `Trainer.pretrain_forward` (core/trainer.py:1242-1279)
fits the NeRF's `depth` and `weights_sum` to the SMPL-X depth map of the loader (`condition.SMPL2Condition(..., 'depth_raw', ...)`) with
two MSE terms.  Here the two terms are one forward and one backward call of csrc/depthmap.hip (include/dwg_depthmap.h), and the map stays
on the device when it arrives as a `condition.DepthMap`.

What differs from the reference, deliberately:
  * `visual_outputs` is built only when `trainer.time_to_snapshot` (the only place the reference reads it: trainer.py:1219-1224) -- the
    depth picture needs max(smpl_depth) on the host, so with snapshots off the step makes no host synchronisation;
  * the loss is always fp32 (under autocast the reference's mse_loss runs in fp32 too); the gradients have the dtype of the renders.
There is no CPU fallback: CPU renders raise."""

import numpy as np
import torch

from . import _lib
from .condition import DepthMap

_DTYPES = {torch.float32: _lib.CONSTANTS["DWG_DTYPE_F32"], torch.float16: _lib.CONSTANTS["DWG_DTYPE_F16"]}
_ws = {}


def _workspace(device, n):
    need = max(int(_lib.lib().dwg_pretrain_loss_workspace_bytes(n)), 16)
    key = str(device)
    if key not in _ws or _ws[key].numel() < need:
        _ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return _ws[key]


class _DepthMaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render_depth, render_ws, smpl_depth):
        dev, n = render_depth.device, render_depth.numel()
        ws = _workspace(dev, n)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        p = _lib.ptr
        _lib.check(_lib.lib().dwg_pretrain_loss_forward(_DTYPES[render_depth.dtype], n, p(render_depth), p(render_ws), p(smpl_depth), p(loss),
                                                        p(ws), ws.numel(), _lib.stream(dev)), "dwg_pretrain_loss_forward")
        ctx.save_for_backward(render_depth, render_ws, smpl_depth)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        render_depth, render_ws, smpl_depth = ctx.saved_tensors
        dev, n = render_depth.device, render_depth.numel()
        g = grad_loss.detach().reshape(1).float().contiguous()
        g_depth = torch.empty_like(render_depth) if ctx.needs_input_grad[0] else None
        g_ws = torch.empty_like(render_ws) if ctx.needs_input_grad[1] else None
        if g_depth is None and g_ws is None:
            return None, None, None
        p = _lib.ptr
        _lib.check(_lib.lib().dwg_pretrain_loss_backward(_DTYPES[render_depth.dtype], n, p(render_depth), p(render_ws), p(smpl_depth), p(g),
                                                         p(g_depth), p(g_ws), _lib.stream(dev)), "dwg_pretrain_loss_backward")
        return g_depth, g_ws, None


def depth_mask_loss(render_depth: torch.Tensor, render_ws: torch.Tensor, smpl_depth: torch.Tensor) -> torch.Tensor:
    """mean((render_ws - mask)^2) + mean((render_depth - sd)^2) with sd = nan_to_num(smpl_depth, nan=0, posinf=0, neginf=0) and
    mask = sd > 1e-6 (trainer.py:1250,1264-1269,1277): a fp32 scalar.  The renders are fp32 or fp16, of one shape; smpl_depth has as
    many elements (it is not differentiated)."""
    if not (render_depth.is_cuda and render_ws.is_cuda and smpl_depth.is_cuda):
        raise RuntimeError("dreamwaltz_g_amd.pretrain runs on the GPU only (HIP kernels); got a CPU tensor")
    if render_depth.dtype not in _DTYPES or render_ws.dtype != render_depth.dtype:
        raise TypeError("render_depth and render_ws are both float32 or both float16; got %s and %s" % (render_depth.dtype, render_ws.dtype))
    if render_depth.shape != render_ws.shape or smpl_depth.numel() != render_depth.numel() or render_depth.numel() == 0:
        raise ValueError("render_depth %s, render_ws %s and smpl_depth %s do not match" % (tuple(render_depth.shape), tuple(render_ws.shape),
                                                                                          tuple(smpl_depth.shape)))
    return _DepthMaskLoss.apply(render_depth.contiguous(), render_ws.contiguous(), smpl_depth.detach().float().contiguous())


def pretrain_forward(trainer, data):
    """Trainer.pretrain_forward (trainer.py:1242-1279) -> (loss, render_outputs, visual_outputs).  `data['cond_images'][0]` is a
    `condition.DepthMap` (stays on the device) or the reference's np.ndarray [H,W] (uploaded)."""
    render_outputs = trainer.render(data=data)
    render_depth = render_outputs['depth'].permute(0, 3, 1, 2).contiguous()
    render_ws = render_outputs['weights_sum'].permute(0, 3, 1, 2).contiguous()
    if not render_depth.is_cuda:
        raise RuntimeError("dreamwaltz_g_amd.pretrain runs on the GPU only (HIP kernels); got a CPU render")
    device = render_depth.device

    cond = data['cond_images'][0]
    if isinstance(cond, DepthMap):
        smpl_depth = cond.t.detach().to(device=device, dtype=torch.float)
    else:
        smpl_depth = torch.from_numpy(np.ascontiguousarray(np.asarray(cond, dtype=np.float32))).to(device)
    smpl_depth = smpl_depth.reshape(1, 1, smpl_depth.shape[-2], smpl_depth.shape[-1])

    visual_outputs = {}
    resample = render_depth.shape[-2:] != smpl_depth.shape[-2:]
    if resample or trainer.time_to_snapshot:
        smpl_depth = torch.nan_to_num(smpl_depth, nan=0.0, posinf=0.0, neginf=0.0)          # trainer.py:1250 (the loss kernel does it itself)
    if trainer.time_to_snapshot:
        from PIL import Image
        sd = smpl_depth[0, 0].cpu().numpy()
        visual_outputs['depth'] = Image.fromarray((255 * sd / np.max(sd)).clip(0, 255).astype(np.uint8), mode="L")
    if resample:
        smpl_depth = torch.nn.functional.interpolate(smpl_depth, size=render_depth.shape[-2:], mode='bicubic')
    if trainer.time_to_snapshot:
        visual_outputs['mask'] = (smpl_depth > 1e-6).float()
    if smpl_depth.shape[0] != render_depth.shape[0]:
        smpl_depth = smpl_depth.expand(render_depth.shape[0], -1, -1, -1).contiguous()     # mse_loss broadcasts over the batch

    loss = depth_mask_loss(render_depth, render_ws, smpl_depth)
    return loss, render_outputs, visual_outputs
