"""MI355X-native inference render of the NeRF stage (boundaries B14 and B15): what the evaluation branch of the reference's
_NeRFRenderer.run_cuda (core/nerf/nerf_renderer.py:351-385) computes for perturb False, in ONE launch of csrc/nerf_field.hip's
k_nf_render (shading 'albedo') or k_nf_render_shaded ('normal', 'textureless', 'lambertian': seven field evaluations per sample, the
finite-difference normal and the shading in the kernel) instead of a Python loop of march_rays -> field -> composite_rays with three
zeroed buffers and one host wait per iteration.

  render_rays(rays_o, rays_d, nears, fars, density_bitfield, cascade, grid_size, encoder, sigma_net, sigma_scale, bound, ...)
                                 (weights_sum [N], depth [N], image [N, out_dim - 1][, counts [N]]) through dwg_nerf_render_infer
                                 or, with shading=..., dwg_nerf_render_shaded (include/dwg_nerf_render.h)
  run_cuda(ref, orig, ...)       the statements of run_cuda around it, for a bound reference network (nerf.bind_nerf_network installs it)

A ray's samples, and everything composited from them, are the loop's: the marching rule is the shared csrc/raymarch_common.h, the field
is the fused kernel's field_tile, the composite is composite_rays' statements in their order.  The one difference: a ray stops after
exactly max_steps composited samples, where the loop's budget (n_step per iteration) lets a ray still alive at the end take between
max_steps and max_steps + 7; rays that end at far or by T_thresh are unaffected.  Precision follows autocast like nerf.nerf_field.
No CPU fallback, no host synchronisation (after the encoder's offsets have been read once); every buffer is checked (CUDA, dtype, shape,
contiguity) and a violation raises RuntimeError before any launch.  Nothing here records autograd state."""
import ctypes

import torch

from . import _lib
from . import nerf
from . import pointcloud

_st = nerf._st
_check = pointcloud._dev_check


SHADINGS = {'albedo': 0, 'normal': 1, 'textureless': 2, 'lambertian': 3}


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
    if shading not in SHADINGS:
        raise RuntimeError("shading must be one of %s, got %r" % (", ".join(sorted(SHADINGS)), shading))
    try:
        spec, emb, ss, wb = pointcloud.field_spec(encoder, sigma_net, sigma_scale, bound, density_activation, density_prior, albedo_sigmoid, precision)
    except ValueError as e:
        raise RuntimeError(str(e)) from None
    _check("rays_o", rays_o, torch.float32, (None, 3))
    N = rays_o.shape[0]
    _check("rays_d", rays_d, torch.float32, (N, 3))
    _check("nears", nears, torch.float32, (N,))
    _check("fars", fars, torch.float32, (N,))
    C, H = int(cascade), int(grid_size)
    if C != cascade or H != grid_size or not (1 <= C <= 8 and 2 <= H <= 1024 and C * H ** 3 < 1 << 32) or H & (H - 1):
        raise RuntimeError("bad occupancy grid shape: cascade %r, grid_size %r (a power of two: a cell's Morton index must stay below "
                           "grid_size^3)" % (cascade, grid_size))
    _check("density_bitfield", density_bitfield, torch.uint8, (C * H ** 3 // 8,))
    if int(max_steps) != max_steps or not 1 <= max_steps < 1 << 31:
        raise RuntimeError("max_steps must be an integer >= 1, got %r" % (max_steps,))
    if N >= 1 << 32:
        raise RuntimeError("render_rays takes fewer than 2^32 rays")
    if int(max_workgroups) != max_workgroups or not 0 <= max_workgroups < 1 << 31:
        raise RuntimeError("max_workgroups must be a non-negative integer, got %r" % (max_workgroups,))
    dev = rays_o.device
    others = []
    if SHADINGS[shading]:
        if light_d is not None:
            _check("light_d", light_d, torch.float32, (3,))
            others.append(("light_d", light_d))
        elif SHADINGS[shading] >= 2:
            raise RuntimeError("shading %r needs light_d" % shading)
        if SHADINGS[shading] == 3 and spec.out_dim == 5:
            raise RuntimeError("shading 'lambertian' with four albedo channels (latent mode) is ill-formed in the reference: five channels "
                               "into a four-channel image")
        if not float(normal_epsilon) > 0:
            raise RuntimeError("normal_epsilon must be positive, got %r" % (normal_epsilon,))
        if float(ambient_ratio) != float(ambient_ratio):
            raise RuntimeError("ambient_ratio is NaN")
    for name, t in [("rays_d", rays_d), ("nears", nears), ("fars", fars), ("density_bitfield", density_bitfield), ("embeddings", emb)] + others:
        if t.device != dev:
            raise RuntimeError("%s is on %s, rays_o on %s" % (name, t.device, dev))
    weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    image = torch.empty((N, spec.out_dim - 1), dtype=torch.float32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev) if return_counts else None
    if N:
        d = spec.desc(emb, ss, wb)
        head = (ctypes.byref(d), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(nears), _lib.ptr(fars), N, _lib.ptr(density_bitfield),
                ctypes.c_float(bound), int(bool(contract)), ctypes.c_float(dt_gamma), int(max_steps), C, H, ctypes.c_float(T_thresh),
                int(bool(binarize)))
        tail = (_lib.ptr(weights_sum), _lib.ptr(depth), _lib.ptr(image), _lib.ptr(counts), int(max_workgroups), _st(rays_o))
        with torch.cuda.device(dev):
            if SHADINGS[shading]:
                _lib.check(_lib.lib().dwg_nerf_render_shaded(*head, SHADINGS[shading], _lib.ptr(light_d), ctypes.c_float(ambient_ratio),
                                                             ctypes.c_float(normal_epsilon), *tail), "dwg_nerf_render_shaded")
            else:
                _lib.check(_lib.lib().dwg_nerf_render_infer(*head, *tail), "dwg_nerf_render_infer")
    return (weights_sum, depth, image, counts) if return_counts else (weights_sum, depth, image)


def covered_call(ref, rays_o, rays_d, shading, perturb, light_d=None):
    """The native render takes this run_cuda call: evaluation mode, no perturbation, CUDA fp32 rays, the bitfield and the parameters on
    the device, and no autocast dtype but fp16.  shading 'albedo' always; with the network bound with shaded_render, also 'normal' (the
    reference's normal arithmetic is fp32 under fp16 autocast too: the field returns an fp32 density) and, without autocast only,
    'textureless' and 'lambertian' (under fp16 autocast the reference's normal @ -l is a half-precision matmul, not restated; latent
    'lambertian' is ill-formed).  A given light_d must be a [3] fp32 tensor on the rays' device."""
    if ref.training or perturb or not getattr(ref, "cuda_ray", False):
        return False
    if shading != 'albedo':
        if not getattr(ref, "_dwg_shaded_render", False) or shading not in SHADINGS:
            return False
        if shading != 'normal' and torch.is_autocast_enabled():
            return False
        if shading == 'lambertian' and ref.sigma_net.net[-1].out_features - 1 != 3:
            return False
        if light_d is not None and not (isinstance(light_d, torch.Tensor) and light_d.dtype == torch.float32 and tuple(light_d.shape) == (3,)
                                        and isinstance(rays_o, torch.Tensor) and light_d.device == rays_o.device):
            return False
    for t in (rays_o, rays_d):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            return False
    bits = getattr(ref, "density_bitfield", None)
    if not isinstance(bits, torch.Tensor) or not bits.is_cuda or bits.dtype != torch.uint8 or not bits.is_contiguous():
        return False
    C, H = ref.cascade, ref.grid_size
    if not (isinstance(C, int) and isinstance(H, int) and 1 <= C <= 8 and 2 <= H <= 1024 and not H & (H - 1) and C * H ** 3 < 1 << 32):
        return False
    if bits.numel() * 8 != C * H ** 3 or ref.sigma_net.net[-1].out_features - 1 not in (3, 4):
        return False
    if not (ref.encoder.embeddings.is_cuda and ref.sigma_scale.is_cuda and all(p.is_cuda for p in ref.sigma_net.parameters())):
        return False
    if torch.is_autocast_enabled():
        dt = torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.get_autocast_gpu_dtype()
        return dt == torch.float16
    return True


def _safe_normalize(x, eps=1e-20):
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


def run_cuda(ref, orig, rays_o, rays_d, light_d=None, ambient_ratio=1.0, shading='albedo', perturb=False, dt_gamma=0, max_steps=1024,
             T_thresh=1e-4, **kwargs):
    """run_cuda of a bound network.  Calls the native render does not take (training, perturb, CPU, bf16 autocast; a shading other than
    'albedo' unless the network was bound with shaded_render, see covered_call) go to `orig` unchanged.  The native branch keeps the original's statements around the loop: near_far_from_aabb with aabb_infer, the light_d
    draw (it consumes the device generator as the original does), the reshapes and mask = nears < fars.  results['xyzs'], ['sigmas'] and
    ['rgbs'] -- in the original the last loop iteration's leftovers, read by nothing outside training -- are None."""
    if not covered_call(ref, rays_o, rays_d, shading, perturb, light_d) or not isinstance(ambient_ratio, (int, float)):
        return orig(rays_o, rays_d, light_d=light_d, ambient_ratio=ambient_ratio, shading=shading, perturb=perturb, dt_gamma=dt_gamma,
                    max_steps=max_steps, T_thresh=T_thresh, **kwargs)
    prefix = rays_o.shape[:-1]
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    device = rays_o.device

    # pre-calculate near far
    nears, fars = ref.raymarching.near_far_from_aabb(rays_o, rays_d, ref.aabb_infer)

    # random sample light_d if not provided
    if light_d is None:
        light_d = (rays_o[0] + torch.randn(3, device=device, dtype=torch.float))
        light_d = _safe_normalize(light_d)

    latent = bool(getattr(ref, "latent_mode", False))
    weights_sum, depth, image = render_rays(
        rays_o, rays_d, nears.float().contiguous(), fars.float().contiguous(), ref.density_bitfield, ref.cascade, ref.grid_size, ref.encoder,
        ref.sigma_net, ref.sigma_scale, ref.bound, density_activation=ref.opt.density_activation, density_prior=ref.density_prior_type,
        albedo_sigmoid=not latent, dt_gamma=dt_gamma, max_steps=max_steps, T_thresh=T_thresh, shading=shading,
        light_d=light_d.contiguous() if shading != 'albedo' else None, ambient_ratio=ambient_ratio)

    results = {}
    results['image'] = image.reshape(*prefix, image.shape[-1])
    results['depth'] = depth.reshape(*prefix)
    results['weights_sum'] = weights_sum.reshape(*prefix)
    results['mask'] = (nears < fars).reshape(*prefix)
    results['xyzs'] = None
    results['sigmas'] = None
    results['rgbs'] = None
    return results
