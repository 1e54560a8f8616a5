"""MI355X-native occupancy-grid ray marcher of the NeRF stage (boundary B6).

  backend-shaped entries   *_into(...)  one per function of the reference's pybind backends `_raymarchingrgb` / `_raymarchinglatent`
                           (/root/reference/core/nerf/raymarching/rgb/src/bindings.cpp), fp32 buffers written in place, plus the colour
                           width `channels` (3 rgb, 4 latent).  dropin/_raymarching_backend.py puts the reference's names and dtypes on them.
  package API              near_far_from_aabb, packbits, morton3D(_invert), march_rays_train, composite_rays_train (autograd),
                           march_rays, composite_rays: the reference's raymarching.py functions (rgb/raymarching.py:35-400) with the same
                           arguments and results.
The arithmetic is csrc/raymarch.hip through include/dwg_raymarch.h; no CPU fallback.  Every buffer is checked (CUDA, contiguous, dtype,
element count) and a violation raises RuntimeError before any launch.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _lib


def check(name, t, dtype, numel=None, optional=False):
    if t is None:
        if optional:
            return
        raise RuntimeError("%s must be a tensor, got None" % name)
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous tensor" % name)
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if numel is not None and t.numel() != numel:
        raise RuntimeError("%s has %d elements, expected %d" % (name, t.numel(), numel))


def _channels(channels):
    if channels not in (3, 4):
        raise RuntimeError("channels must be 3 (rgb) or 4 (latent), got %r" % (channels,))


def _grid_bytes(C, H):
    if C < 1 or H < 2 or H % 2:
        raise RuntimeError("bad occupancy grid shape C=%d H=%d" % (C, H))
    return C * H ** 3 // 8


_F, _I = torch.float32, torch.int32


# ------------------------------------------------------------------------------------------------------------------------------------
# backend-shaped entries (fp32; outputs written in place)
# ------------------------------------------------------------------------------------------------------------------------------------
def near_far_from_aabb_into(rays_o, rays_d, aabb, N, min_near, nears, fars):
    check("rays_o", rays_o, _F, 3 * N); check("rays_d", rays_d, _F, 3 * N); check("aabb", aabb, _F, 6)
    check("nears", nears, _F, N); check("fars", fars, _F, N)
    _lib.check(_lib.lib().dwg_raymarch_near_far_from_aabb(_lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(aabb), N, ctypes.c_float(min_near), _lib.ptr(nears), _lib.ptr(fars),
                                                          _lib.stream(rays_o)), "dwg_raymarch_near_far_from_aabb")


def sph_from_ray_into(rays_o, rays_d, radius, N, coords):
    check("rays_o", rays_o, _F, 3 * N); check("rays_d", rays_d, _F, 3 * N); check("coords", coords, _F, 2 * N)
    _lib.check(_lib.lib().dwg_raymarch_sph_from_ray(_lib.ptr(rays_o), _lib.ptr(rays_d), ctypes.c_float(radius), N, _lib.ptr(coords), _lib.stream(rays_o)),
               "dwg_raymarch_sph_from_ray")


def morton3D_into(coords, N, indices):
    check("coords", coords, _I, 3 * N); check("indices", indices, _I, N)
    _lib.check(_lib.lib().dwg_raymarch_morton3d(_lib.ptr(coords), N, _lib.ptr(indices), _lib.stream(coords)), "dwg_raymarch_morton3d")


def morton3D_invert_into(indices, N, coords):
    check("indices", indices, _I, N); check("coords", coords, _I, 3 * N)
    _lib.check(_lib.lib().dwg_raymarch_morton3d_invert(_lib.ptr(indices), N, _lib.ptr(coords), _lib.stream(indices)), "dwg_raymarch_morton3d_invert")


def packbits_into(grid, N, density_thresh, bitfield):
    check("grid", grid, _F, 8 * N); check("bitfield", bitfield, torch.uint8, N)
    if grid.data_ptr() % 16:
        grid = grid.clone()                                      # the kernel reads 2 x 16 bytes per output byte
    _lib.check(_lib.lib().dwg_raymarch_packbits(_lib.ptr(grid), N, ctypes.c_float(density_thresh), _lib.ptr(bitfield), _lib.stream(grid)), "dwg_raymarch_packbits")


def flatten_rays_into(rays, N, M, res):
    check("rays", rays, _I, 2 * N); check("res", res, _I, M)
    _lib.check(_lib.lib().dwg_raymarch_flatten_rays(_lib.ptr(rays), N, M, _lib.ptr(res), _lib.stream(rays)), "dwg_raymarch_flatten_rays")


def march_rays_train_into(rays_o, rays_d, grid, bound, contract, dt_gamma, max_steps, N, C, H, nears, fars, xyzs, dirs, ts, rays, counter,
                          noises):
    """xyzs / dirs / ts all None: count pass (rays[:,1] = counts, rays[:,0] = counter + exclusive prefix sum, counter += M); else the
    write pass into [M,3] / [M,3] / [M,2] buffers."""
    check("rays_o", rays_o, _F, 3 * N); check("rays_d", rays_d, _F, 3 * N); check("grid", grid, torch.uint8, _grid_bytes(C, H))
    check("nears", nears, _F, N); check("fars", fars, _F, N); check("rays", rays, _I, 2 * N); check("counter", counter, _I)
    check("noises", noises, _F, N)
    if counter.numel() < 1:
        raise RuntimeError("counter must hold at least one element")
    if max_steps < 1 or not bound > 0:
        raise RuntimeError("max_steps must be >= 1 and bound > 0")
    L = _lib.lib()
    if xyzs is None and dirs is None and ts is None:
        ws = torch.empty(max(1, L.dwg_raymarch_train_workspace_bytes(N)), dtype=torch.uint8, device=rays.device)
        _lib.check(L.dwg_raymarch_march_rays_train(_lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(grid), ctypes.c_float(bound), int(bool(contract)),
                                                   ctypes.c_float(dt_gamma), max_steps, N, C, H, _lib.ptr(nears), _lib.ptr(fars), None, None, None, 0,
                                                   _lib.ptr(rays), _lib.ptr(counter), _lib.ptr(noises), _lib.ptr(ws), ws.numel(), _lib.stream(rays)), "dwg_raymarch_march_rays_train")
        return
    if xyzs is None or dirs is None or ts is None:
        raise RuntimeError("xyzs, dirs and ts are either all None (count pass) or all tensors (write pass)")
    check("xyzs", xyzs, _F); M = xyzs.numel() // 3
    check("xyzs", xyzs, _F, 3 * M); check("dirs", dirs, _F, 3 * M); check("ts", ts, _F, 2 * M)
    if M == 0:
        return                                                   # nothing to write (an empty tensor has no address to pass)
    _lib.check(L.dwg_raymarch_march_rays_train(_lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(grid), ctypes.c_float(bound), int(bool(contract)),
                                               ctypes.c_float(dt_gamma), max_steps, N, C, H, _lib.ptr(nears), _lib.ptr(fars), _lib.ptr(xyzs), _lib.ptr(dirs), _lib.ptr(ts), M,
                                               _lib.ptr(rays), _lib.ptr(counter), _lib.ptr(noises), None, 0, _lib.stream(rays)), "dwg_raymarch_march_rays_train")


def composite_rays_train_forward_into(sigmas, rgbs, ts, rays, M, N, T_thresh, binarize, weights, weights_sum, depth, image, channels):
    _channels(channels)
    check("sigmas", sigmas, _F, M); check("rgbs", rgbs, _F, channels * M); check("ts", ts, _F, 2 * M); check("rays", rays, _I, 2 * N)
    check("weights", weights, _F, M); check("weights_sum", weights_sum, _F, N); check("depth", depth, _F, N)
    check("image", image, _F, channels * N)
    _lib.check(_lib.lib().dwg_raymarch_composite_rays_train_forward(
        _lib.ptr(sigmas), _lib.ptr(rgbs), _lib.ptr(ts), _lib.ptr(rays), M, N, channels, ctypes.c_float(T_thresh), int(bool(binarize)), _lib.ptr(weights), _lib.ptr(weights_sum),
        _lib.ptr(depth), _lib.ptr(image), _lib.stream(rays)), "dwg_raymarch_composite_rays_train_forward")


def composite_rays_train_backward_into(grad_weights, grad_weights_sum, grad_depth, grad_image, sigmas, rgbs, ts, rays, weights_sum, depth,
                                       image, M, N, T_thresh, binarize, grad_sigmas, grad_rgbs, channels):
    _channels(channels)
    check("grad_weights", grad_weights, _F, M); check("grad_weights_sum", grad_weights_sum, _F, N); check("grad_depth", grad_depth, _F, N)
    check("grad_image", grad_image, _F, channels * N); check("sigmas", sigmas, _F, M); check("rgbs", rgbs, _F, channels * M)
    check("ts", ts, _F, 2 * M); check("rays", rays, _I, 2 * N); check("weights_sum", weights_sum, _F, N); check("depth", depth, _F, N)
    check("image", image, _F, channels * N); check("grad_sigmas", grad_sigmas, _F, M); check("grad_rgbs", grad_rgbs, _F, channels * M)
    _lib.check(_lib.lib().dwg_raymarch_composite_rays_train_backward(
        _lib.ptr(grad_weights), _lib.ptr(grad_weights_sum), _lib.ptr(grad_depth), _lib.ptr(grad_image), _lib.ptr(sigmas), _lib.ptr(rgbs), _lib.ptr(ts), _lib.ptr(rays), _lib.ptr(weights_sum),
        _lib.ptr(depth), _lib.ptr(image), M, N, channels, ctypes.c_float(T_thresh), int(bool(binarize)), _lib.ptr(grad_sigmas), _lib.ptr(grad_rgbs), _lib.stream(rays)),
        "dwg_raymarch_composite_rays_train_backward")


def march_rays_into(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, contract, dt_gamma, max_steps, C, H, grid, nears, fars,
                    xyzs, dirs, ts, noises):
    check("rays_o", rays_o, _F); N = rays_o.numel() // 3
    check("rays_o", rays_o, _F, 3 * N); check("rays_d", rays_d, _F, 3 * N); check("nears", nears, _F, N); check("fars", fars, _F, N)
    check("rays_t", rays_t, _F, N); check("rays_alive", rays_alive, _I)
    if rays_alive.numel() < n_alive:
        raise RuntimeError("rays_alive has %d elements, fewer than n_alive = %d" % (rays_alive.numel(), n_alive))
    check("grid", grid, torch.uint8, _grid_bytes(C, H)); check("noises", noises, _F, n_alive)
    check("xyzs", xyzs, _F, 3 * n_alive * n_step); check("dirs", dirs, _F, 3 * n_alive * n_step); check("ts", ts, _F, 2 * n_alive * n_step)
    if max_steps < 1 or not bound > 0:
        raise RuntimeError("max_steps must be >= 1 and bound > 0")
    _lib.check(_lib.lib().dwg_raymarch_march_rays(
        n_alive, n_step, _lib.ptr(rays_alive), _lib.ptr(rays_t), _lib.ptr(rays_o), _lib.ptr(rays_d), ctypes.c_float(bound), int(bool(contract)), ctypes.c_float(dt_gamma),
        max_steps, C, H, _lib.ptr(grid), _lib.ptr(nears), _lib.ptr(fars), N, _lib.ptr(xyzs), _lib.ptr(dirs), _lib.ptr(ts), _lib.ptr(noises), _lib.stream(rays_o)), "dwg_raymarch_march_rays")


def composite_rays_into(n_alive, n_step, T_thresh, binarize, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, channels):
    _channels(channels)
    check("weights_sum", weights_sum, _F); N = weights_sum.numel()
    check("depth", depth, _F, N); check("image", image, _F, channels * N); check("rays_t", rays_t, _F, N); check("rays_alive", rays_alive, _I)
    if rays_alive.numel() < n_alive:
        raise RuntimeError("rays_alive has %d elements, fewer than n_alive = %d" % (rays_alive.numel(), n_alive))
    M = n_alive * n_step
    check("sigmas", sigmas, _F, M); check("rgbs", rgbs, _F, channels * M); check("ts", ts, _F, 2 * M)
    _lib.check(_lib.lib().dwg_raymarch_composite_rays(
        n_alive, n_step, channels, ctypes.c_float(T_thresh), int(bool(binarize)), _lib.ptr(rays_alive), _lib.ptr(rays_t), _lib.ptr(sigmas), _lib.ptr(rgbs), _lib.ptr(ts), N,
        _lib.ptr(weights_sum), _lib.ptr(depth), _lib.ptr(image), _lib.stream(rays_t)), "dwg_raymarch_composite_rays")


# ------------------------------------------------------------------------------------------------------------------------------------
# package API (the reference's raymarching.py surface)
# ------------------------------------------------------------------------------------------------------------------------------------
def _rays(t):
    return t.float().contiguous().view(-1, 3)


def near_far_from_aabb(rays_o, rays_d, aabb, min_near=0.2):
    rays_o, rays_d = _rays(rays_o), _rays(rays_d)
    N = rays_o.shape[0]
    nears = torch.empty(N, dtype=_F, device=rays_o.device)
    fars = torch.empty(N, dtype=_F, device=rays_o.device)
    near_far_from_aabb_into(rays_o, rays_d, aabb.float().contiguous(), N, min_near, nears, fars)
    return nears, fars


def packbits(grid, thresh, bitfield=None):
    grid = grid.float().contiguous()
    N = grid.numel() // 8
    if bitfield is None:
        bitfield = torch.empty(N, dtype=torch.uint8, device=grid.device)
    packbits_into(grid, N, thresh, bitfield)
    return bitfield


def morton3D(coords):
    coords = coords.int().contiguous()
    N = coords.shape[0]
    indices = torch.empty(N, dtype=_I, device=coords.device)
    morton3D_into(coords, N, indices)
    return indices


def morton3D_invert(indices):
    indices = indices.int().contiguous()
    N = indices.shape[0]
    coords = torch.empty(N, 3, dtype=_I, device=indices.device)
    morton3D_invert_into(indices, N, coords)
    return coords


def march_rays_train(rays_o, rays_d, bound, density_bitfield, C, H, nears, fars, perturb=False, dt_gamma=0, max_steps=1024, contract=False,
                     noises=None):
    """-> xyzs [M,3], dirs [M,3], ts [M,2], rays [N,2] (offset, count); ray-major, one host read of M.  `noises` [N] overrides the
    perturbation draw (tests)."""
    rays_o, rays_d = _rays(rays_o), _rays(rays_d)
    N = rays_o.shape[0]
    dev = rays_o.device
    counter = torch.zeros(1, dtype=_I, device=dev)
    if noises is None:
        noises = torch.rand(N, device=dev) if perturb else torch.zeros(N, device=dev)
    rays = torch.empty(N, 2, dtype=_I, device=dev)
    nears, fars = nears.float().contiguous(), fars.float().contiguous()
    args = (rays_o, rays_d, density_bitfield.contiguous(), bound, contract, dt_gamma, max_steps, N, C, H, nears, fars)
    march_rays_train_into(*args, None, None, None, rays, counter, noises)
    M = int(counter.item())
    xyzs = torch.zeros(M, 3, dtype=_F, device=dev)
    dirs = torch.zeros(M, 3, dtype=_F, device=dev)
    ts = torch.zeros(M, 2, dtype=_F, device=dev)
    if M:
        march_rays_train_into(*args, xyzs, dirs, ts, rays, counter, noises)
    return xyzs, dirs, ts, rays


class _CompositeRaysTrain(Function):
    @staticmethod
    def forward(ctx, sigmas, rgbs, ts, rays, T_thresh=1e-4, binarize=False):
        sigmas = sigmas.float().contiguous()
        rgbs = rgbs.float().contiguous()
        ts = ts.float().contiguous()
        rays = rays.contiguous()
        M, N, ch = sigmas.shape[0], rays.shape[0], rgbs.shape[-1]
        weights = torch.zeros(M, dtype=_F, device=sigmas.device)
        weights_sum = torch.empty(N, dtype=_F, device=sigmas.device)
        depth = torch.empty(N, dtype=_F, device=sigmas.device)
        image = torch.empty(N, ch, dtype=_F, device=sigmas.device)
        composite_rays_train_forward_into(sigmas, rgbs, ts, rays, M, N, T_thresh, binarize, weights, weights_sum, depth, image, ch)
        ctx.save_for_backward(sigmas, rgbs, ts, rays, weights_sum, depth, image)
        ctx.dims = (M, N, T_thresh, binarize, ch)
        return weights, weights_sum, depth, image

    @staticmethod
    def backward(ctx, grad_weights, grad_weights_sum, grad_depth, grad_image):
        sigmas, rgbs, ts, rays, weights_sum, depth, image = ctx.saved_tensors
        M, N, T_thresh, binarize, ch = ctx.dims

        def g(t, like):
            return torch.zeros_like(like) if t is None else t.float().contiguous()
        grad_sigmas = torch.zeros_like(sigmas)
        grad_rgbs = torch.zeros_like(rgbs)
        composite_rays_train_backward_into(g(grad_weights, sigmas), g(grad_weights_sum, weights_sum), g(grad_depth, depth), g(grad_image, image),
                                           sigmas, rgbs, ts, rays, weights_sum, depth, image, M, N, T_thresh, binarize, grad_sigmas, grad_rgbs, ch)
        return grad_sigmas, grad_rgbs, None, None, None, None


def composite_rays_train(sigmas, rgbs, ts, rays, T_thresh=1e-4, binarize=False):
    """-> weights [M], weights_sum [N], depth [N], image [N, channels]; differentiable in sigmas and rgbs (the reference's gradient
    formula, raymarching.cu:652-694)."""
    return _CompositeRaysTrain.apply(sigmas, rgbs, ts, rays, T_thresh, binarize)


def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, density_bitfield, C, H, near, far, perturb=False, dt_gamma=0,
               max_steps=1024, contract=False):
    """-> xyzs [n_alive*n_step, 3], dirs, ts [n_alive*n_step, 2] (rows of rays that stopped early stay zero)."""
    rays_o, rays_d = _rays(rays_o), _rays(rays_d)
    M = n_alive * n_step
    dev = rays_o.device
    xyzs = torch.zeros(M, 3, dtype=_F, device=dev)
    dirs = torch.zeros(M, 3, dtype=_F, device=dev)
    ts = torch.zeros(M, 2, dtype=_F, device=dev)
    noises = torch.rand(n_alive, device=dev) if perturb else torch.zeros(n_alive, device=dev)
    march_rays_into(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, contract, dt_gamma, max_steps, C, H, density_bitfield.contiguous(),
                    near, far, xyzs, dirs, ts, noises)
    return xyzs, dirs, ts


def composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, ts, weights_sum, depth, image, T_thresh=1e-2, binarize=False):
    """In place: weights_sum / depth / image accumulate, rays_alive[n] = -1 for terminated rays, rays_t advances for live ones."""
    composite_rays_into(n_alive, n_step, T_thresh, binarize, rays_alive, rays_t, sigmas.float().contiguous(), rgbs.float().contiguous(), ts,
                        weights_sum, depth, image, image.shape[-1])
