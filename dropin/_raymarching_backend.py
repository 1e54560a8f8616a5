"""Shared body of the import-compatible stand-ins for the pybind modules `_raymarchingrgb` and `_raymarchinglatent`
(/root/reference/core/nerf/raymarching/{rgb,latent}/src/bindings.cpp; prototypes in raymarching.h).  With `<repo>/dropin` on PYTHONPATH,
`import _raymarchingrgb as _backend` in the reference's raymarching.py:14-27 resolves to dropin/_raymarchingrgb.py, which is
`functions(3, binarize=True)` of this module; the latent one is `functions(4, binarize=False)`.

Same names, same positional order, outputs written in place into the caller's tensors.  dtypes: the kernels compute in fp32; fp16 / fp64
buffers (the backends dispatch AT_DISPATCH_FLOATING_TYPES_AND_HALF) go through fp32 temporaries and are copied back in the caller's dtype.
A CPU, non-contiguous, wrongly typed or wrongly sized buffer raises RuntimeError (the reference's TORCH_CHECKs) before any launch.
"""
import os
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
import dwg_import  # noqa: E402,F401
from dreamwaltz_g_amd import raymarch as _rm  # noqa: E402

NAMES = ("flatten_rays", "packbits", "near_far_from_aabb", "sph_from_ray", "morton3D", "morton3D_invert", "march_rays_train",
         "composite_rays_train_forward", "composite_rays_train_backward", "march_rays", "composite_rays")
_FLOATS = (torch.float32, torch.float16, torch.float64)


def _pre(name, t, floating=True):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous tensor" % name)
    if floating and t.dtype not in _FLOATS:
        raise RuntimeError("%s must be a floating tensor (float, half or double), got %s" % (name, t.dtype))


def _f(name, t):
    """floating input -> fp32 (a copy only when the caller's dtype is not fp32)"""
    _pre(name, t)
    return t if t.dtype == torch.float32 else t.float()


class _Outs:
    """floating outputs: an fp32 temporary holding the caller's current values (the kernels accumulate into some of them), copied
    back in the caller's dtype by flush()"""

    def __init__(self):
        self.pairs = []

    def __call__(self, name, t):
        _pre(name, t)
        if t.dtype == torch.float32:
            return t
        tmp = t.float()
        self.pairs.append((t, tmp))
        return tmp

    def flush(self):
        for t, tmp in self.pairs:
            t.copy_(tmp)


def _i(name, t):
    _pre(name, t, floating=False)
    return t


def flatten_rays(rays, N, M, res):
    _rm.flatten_rays_into(_i("rays", rays), N, M, _i("res", res))


def packbits(grid, N, density_thresh, bitfield):
    _rm.packbits_into(_f("grid", grid), N, density_thresh, _i("bitfield", bitfield))


def near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars):
    o = _Outs()
    _rm.near_far_from_aabb_into(_f("rays_o", rays_o), _f("rays_d", rays_d), _f("aabb", aabb), N, min_near, o("nears", nears), o("fars", fars))
    o.flush()


def sph_from_ray(rays_o, rays_d, radius, N, coords):
    o = _Outs()
    _rm.sph_from_ray_into(_f("rays_o", rays_o), _f("rays_d", rays_d), radius, N, o("coords", coords))
    o.flush()


def morton3D(coords, N, indices):
    _rm.morton3D_into(_i("coords", coords), N, _i("indices", indices))


def morton3D_invert(indices, N, coords):
    _rm.morton3D_invert_into(_i("indices", indices), N, _i("coords", coords))


def march_rays_train(rays_o, rays_d, grid, bound, contract, dt_gamma, max_steps, N, C, H, nears, fars, xyzs, dirs, ts, rays, counter, noises):
    o = _Outs()
    outs = [None if t is None else o(name, t) for name, t in (("xyzs", xyzs), ("dirs", dirs), ("ts", ts))]
    _rm.march_rays_train_into(_f("rays_o", rays_o), _f("rays_d", rays_d), _i("grid", grid), bound, contract, dt_gamma, max_steps, N, C, H,
                              _f("nears", nears), _f("fars", fars), *outs, _i("rays", rays), _i("counter", counter), _f("noises", noises))
    o.flush()


def _composite_forward(channels, sigmas, rgbs, ts, rays, M, N, T_thresh, binarize, weights, weights_sum, depth, image):
    o = _Outs()
    _rm.composite_rays_train_forward_into(_f("sigmas", sigmas), _f("rgbs", rgbs), _f("ts", ts), _i("rays", rays), M, N, T_thresh, binarize,
                                          o("weights", weights), o("weights_sum", weights_sum), o("depth", depth), o("image", image), channels)
    o.flush()


def _composite_backward(channels, grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth, image, M,
                        N, T_thresh, binarize, grad_sigmas, grad_rgbs):
    o = _Outs()
    _rm.composite_rays_train_backward_into(_f("grad_weights", grad_weights), _f("grad_weights_sum", grad_weights_sum), _f("grad_depth", grad_depth),
                                           _f("grad_image", grad_image), _f("sigmas", sigmas), _f("rgbs", rgbs), _f("ts", ts), _i("rays", rays),
                                           _f("weights_sum", weights_sum), _f("depth", depth), _f("image", image), M, N, T_thresh, binarize,
                                           o("grad_sigmas", grad_sigmas), o("grad_rgbs", grad_rgbs), channels)
    o.flush()


def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, contract, dt_gamma, max_steps, C, H, grid, near, far, xyzs, dirs, ts,
               noises):
    o = _Outs()
    _rm.march_rays_into(n_alive, n_step, _i("rays_alive", rays_alive), _f("rays_t", rays_t), _f("rays_o", rays_o), _f("rays_d", rays_d), bound,
                        contract, dt_gamma, max_steps, C, H, _i("grid", grid), _f("near", near), _f("far", far), o("xyzs", xyzs), o("dirs", dirs),
                        o("ts", ts), _f("noises", noises))
    o.flush()


def _composite_rays(channels, n_alive, n_step, T_thresh, binarize, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image):
    o = _Outs()
    _rm.composite_rays_into(n_alive, n_step, T_thresh, binarize, _i("rays_alive", rays_alive), o("rays_t", rays_t), _f("sigmas", sigmas),
                            _f("rgbs", rgbs), _f("ts", ts), o("weights_sum", weights_sum), o("depth", depth), o("image", image), channels)
    o.flush()


def functions(channels, binarize):
    """{name: function} of one backend module: the 11 names of bindings.cpp, in raymarching.h's positional order (the latent module's
    composite functions have no `binarize`)."""
    if binarize:
        def composite_rays_train_forward(sigmas, rgbs, ts, rays, M, N, T_thresh, binarize, weights, weights_sum, depth, image):
            _composite_forward(channels, sigmas, rgbs, ts, rays, M, N, T_thresh, binarize, weights, weights_sum, depth, image)

        def composite_rays_train_backward(grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth,
                                          image, M, N, T_thresh, binarize, grad_sigmas, grad_rgbs):
            _composite_backward(channels, grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth, image,
                                M, N, T_thresh, binarize, grad_sigmas, grad_rgbs)

        def composite_rays(n_alive, n_step, T_thresh, binarize, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image):
            _composite_rays(channels, n_alive, n_step, T_thresh, binarize, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image)
    else:
        def composite_rays_train_forward(sigmas, rgbs, ts, rays, M, N, T_thresh, weights, weights_sum, depth, image):
            _composite_forward(channels, sigmas, rgbs, ts, rays, M, N, T_thresh, False, weights, weights_sum, depth, image)

        def composite_rays_train_backward(grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth,
                                          image, M, N, T_thresh, grad_sigmas, grad_rgbs):
            _composite_backward(channels, grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth, image,
                                M, N, T_thresh, False, grad_sigmas, grad_rgbs)

        def composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image):
            _composite_rays(channels, n_alive, n_step, T_thresh, False, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image)
    fns = dict(flatten_rays=flatten_rays, packbits=packbits, near_far_from_aabb=near_far_from_aabb, sph_from_ray=sph_from_ray,
               morton3D=morton3D, morton3D_invert=morton3D_invert, march_rays_train=march_rays_train,
               composite_rays_train_forward=composite_rays_train_forward, composite_rays_train_backward=composite_rays_train_backward,
               march_rays=march_rays, composite_rays=composite_rays)
    assert tuple(sorted(fns)) == tuple(sorted(NAMES))
    return fns
