"""MI355X-native grid encoder behind the reference's interfaces (boundary B2).

  GridEncoder / grid_encode      mirror /root/reference/core/nerf/gridencoder/grid.py:28-165 (same ctor args,
                                 same offset table, same autograd contract)
  grid_encode_forward/backward   mirror the pybind backend `_gridencoder` (src/bindings.cpp:5-9) so that the
                                 reference's own grid.py can bind to this module unchanged (dropin/_gridencoder.py)
The arithmetic is csrc/gridenc.hip through include/dwg_gridenc.h; no CPU fallback.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib

_gridtype_to_id = {'hash': 0, 'tiled': 1}
_interp_to_id = {'linear': 0, 'smoothstep': 1}


def _need_cuda(t):
    if not t.is_cuda:
        raise RuntimeError("dreamwaltz_g_amd grid encoder runs on the GPU only (HIP kernels)")


def grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, dy_dx, gridtype, align_corners, interp,
                        out_layout=0):
    """Backend-compatible entry (outputs [L,B,C] when out_layout == 0)."""
    _need_cuda(inputs)
    p = _lib.ptr
    _lib.check(_lib.lib().dwg_grid_encode_forward(p(inputs), p(embeddings), p(offsets), p(outputs), B, D, C, L,
                                                  ctypes.c_float(S), H, p(dy_dx), gridtype, int(bool(align_corners)),
                                                  interp, out_layout, _lib.stream(inputs)), "dwg_grid_encode_forward")


_host_offsets = []          # [(offsets tensor kept alive, its version, ctypes array)]
_host_arrays = {}


def _host_array(values):
    """ctypes int32 array for a tuple of level offsets (cached by CONTENT)."""
    if values not in _host_arrays:
        _host_arrays[values] = (ctypes.c_int32 * len(values))(*values)
    return _host_arrays[values]


def _host_offsets_of(offsets):
    """HOST copy of the level offset table for callers that only hand over the device tensor (the `_gridencoder` backend seam).
    The cache entry holds the tensor itself -- its storage cannot be recycled for another table while the entry lives -- and its
    version counter; the array itself is shared by CONTENT."""
    for ref, ver, arr in _host_offsets:
        if ref is offsets and ref._version == ver:
            return arr
    arr = _host_array(tuple(int(v) for v in offsets.cpu().tolist()))
    _host_offsets[:] = [e for e in _host_offsets if e[0] is not offsets][-15:] + [(offsets, offsets._version, arr)]
    return arr


_INPLACE_OK = [True]


class table_grad_inplace:
    """`with table_grad_inplace(False):` -- forwards issued inside the block opt OUT of the in-place table gradient (see
    _grid_encode.backward): a multi-stream multi-view step, whose concurrent backwards must not read-add-write one gradient slice.  The
    decision is taken at FORWARD time and travels on the autograd ctx; nothing global is consulted by the backward, and leaving the block
    (normally or by an exception) restores the previous setting."""

    def __init__(self, ok: bool):
        self.ok = bool(ok)

    def __enter__(self):
        self.prev, _INPLACE_OK[0] = _INPLACE_OK[0], self.ok

    def __exit__(self, *exc):
        _INPLACE_OK[0] = self.prev

# The autograd backward takes the slab-binned path from this many points (round 5; 16384 before): it is the DETERMINISTIC one (64-bit
# fixed-point sums), and a training step's table gradient should reproduce bit for bit at every avatar size; below that the handful of
# float atomics of the device-scope path cost less than the slab path's five dependent launches
SLAB_MIN_POINTS = 2048

_SLAB_WS = {}     # (device, stream) -> byte workspace of the slab-binned backward (grown on demand; backwards on one stream are ordered,
                  # a workspace replaced by a bigger one is only released by the caching allocator in that stream's order)


def slab_path_ok(B, L, total_entries):
    """Limits of dwg_grid_encode_backward_slabs (it returns DWG_E_CAPACITY beyond them): one u32 LDS counter per 4096-entry slab within
    64 KiB, u32 record positions."""
    return (total_entries + 4095) // 4096 * 4 <= 64 * 1024 and B * L * 8 <= 0xffffffff


def slab_workspace_for(device, B, L, total_entries):
    need = int(_lib.lib().dwg_grid_backward_slabs_workspace_bytes(B, L, total_entries))
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _SLAB_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _SLAB_WS[key] = ws
    return ws


def grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs,
                         gridtype, align_corners, interp, grad_layout=0, host_offsets=None, slab_workspace=None, accumulate=False):
    """slab_workspace given: the slab-binned table gradient (overwriting a zeroed grad_embeddings, or adding into it with `accumulate`);
    else the float-atomics path."""
    _need_cuda(inputs)
    p = _lib.ptr
    ho = host_offsets if host_offsets is not None else _host_offsets_of(offsets)
    if slab_workspace is not None:
        _lib.check(_lib.lib().dwg_grid_encode_backward_slabs(p(grad), p(inputs), p(embeddings), p(offsets), p(grad_embeddings), B, D,
                                                             C, L, ctypes.c_float(S), H, p(dy_dx), p(grad_inputs), gridtype,
                                                             int(bool(align_corners)), interp, grad_layout,
                                                             ctypes.cast(ho, ctypes.c_void_p), p(slab_workspace), slab_workspace.numel(),
                                                             int(bool(accumulate)), _lib.stream(inputs)), "dwg_grid_encode_backward_slabs")
        return
    _lib.check(_lib.lib().dwg_grid_encode_backward(p(grad), p(inputs), p(embeddings), p(offsets), p(grad_embeddings), B, D,
                                                   C, L, ctypes.c_float(S), H, p(dy_dx), p(grad_inputs), gridtype,
                                                   int(bool(align_corners)), interp, grad_layout,
                                                   ctypes.cast(ho, ctypes.c_void_p), _lib.stream(inputs)),
               "dwg_grid_encode_backward")


class _grid_encode(Function):
    @staticmethod
    def forward(ctx, inputs, embeddings, offsets, per_level_scale, base_resolution, calc_grad_inputs=False, gridtype=0,
                align_corners=False, interpolation=0, host_offsets=None):
        """host_offsets: ctypes int32 array holding the same values as `offsets` (the GridEncoder module keeps one: it builds
        the table on the host).  Without it the backward falls back to a per-tensor cache keyed by the device address."""
        inputs = inputs.contiguous().float()
        embeddings = embeddings.contiguous().float()
        B, D = inputs.shape
        L = offsets.shape[0] - 1
        C = embeddings.shape[1]
        S = float(np.log2(per_level_scale))
        H = int(base_resolution)
        outputs = torch.empty(B, L * C, device=inputs.device, dtype=torch.float32)   # written directly as [B, L*C]
        dy_dx = torch.empty(B, L * D * C, device=inputs.device, dtype=torch.float32) if calc_grad_inputs else None
        grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H, dy_dx, gridtype, align_corners,
                            interpolation, out_layout=1)
        ctx.save_for_backward(inputs, embeddings, offsets, dy_dx)
        ctx.dims = [B, D, C, L, S, H, gridtype, interpolation]
        ctx.align_corners = align_corners
        ctx.host_offsets = host_offsets
        ctx.inplace_ok = _INPLACE_OK[0]
        return outputs

    @staticmethod
    def backward(ctx, grad):
        inputs, embeddings, offsets, dy_dx = ctx.saved_tensors
        B, D, C, L, S, H, gridtype, interpolation = ctx.dims
        grad = grad.contiguous().float()
        grad_inputs = torch.empty_like(inputs) if dy_dx is not None else None
        slabs = B >= SLAB_MIN_POINTS and slab_path_ok(B, L, int(embeddings.shape[0]))
        slab_ws = slab_workspace_for(inputs.device, B, L, int(embeddings.shape[0])) if slabs else None
        # The table is a leaf Parameter whose .grad is its slice of the flat gradient buffer (optim.FlatBuffers marks such parameters:
        # `_dwg_flat`): the slab pass ADDS straight into it and autograd is handed None -- instead of a zeroed 50 MB temporary that autograd
        # then adds to .grad (a 50 MB fill and a 150 MB add per backward).  Opt-in PER PARAMETER: a frozen table, a table whose .grad was
        # rebound, a table of another optimizer or one autograd did not ask a gradient for gets the gradient returned the ordinary way
        # (FlatBuffers.owns_grad).  `torch.autograd.grad(out, [table])` on a flat-buffer table cannot be told from `.backward()` here: such
        # a caller wraps the forward in `table_grad_inplace(False)`.
        flat = getattr(embeddings, "_dwg_flat", None)
        in_place = slabs and flat is not None and ctx.needs_input_grad[1] and flat.owns_grad(embeddings) and ctx.inplace_ok
        grad_embeddings = embeddings.grad if in_place else torch.zeros_like(embeddings)
        grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings, B, D, C, L, S, H, dy_dx, grad_inputs,
                             gridtype, ctx.align_corners, interpolation, grad_layout=1, host_offsets=ctx.host_offsets,
                             slab_workspace=slab_ws, accumulate=in_place)
        if in_place:
            flat.touch(embeddings)      # autograd never sees this gradient: record the parameter's participation for the optimizer
        return grad_inputs, (None if in_place else grad_embeddings), None, None, None, None, None, None, None, None


def grid_encode(inputs, embeddings, offsets, per_level_scale, base_resolution, calc_grad_inputs=False, gridtype=0,
                align_corners=False, interpolation=0, host_offsets=None):
    """Same positional signature as the reference's `grid_encode = _grid_encode.apply` (grid.py:96), plus the optional host copy."""
    return _grid_encode.apply(inputs, embeddings, offsets, per_level_scale, base_resolution, calc_grad_inputs, gridtype,
                              align_corners, interpolation, host_offsets)


class GridEncoder(nn.Module):
    """Same constructor / buffers / parameter names as the reference's GridEncoder (grid.py:99-144)."""

    def __init__(self, input_dim=3, num_levels=16, level_dim=2, per_level_scale=2, base_resolution=16,
                 log2_hashmap_size=19, desired_resolution=None, gridtype='hash', align_corners=False,
                 interpolation='linear'):
        super().__init__()
        if desired_resolution is not None:
            per_level_scale = np.exp2(np.log2(desired_resolution / base_resolution) / (num_levels - 1))
        self.input_dim, self.num_levels, self.level_dim = input_dim, num_levels, level_dim
        self.per_level_scale, self.log2_hashmap_size, self.base_resolution = per_level_scale, log2_hashmap_size, base_resolution
        self.output_dim = num_levels * level_dim
        self.gridtype, self.gridtype_id = gridtype, _gridtype_to_id[gridtype]
        self.interpolation, self.interp_id = interpolation, _interp_to_id[interpolation]
        self.align_corners = align_corners
        offsets, offset = [], 0
        self.max_params = 2 ** log2_hashmap_size
        for i in range(num_levels):
            resolution = int(np.ceil(base_resolution * per_level_scale ** i))
            params_in_level = min(self.max_params, (resolution if align_corners else resolution + 1) ** input_dim)
            params_in_level = int(np.ceil(params_in_level / 8) * 8)
            offsets.append(offset)
            offset += params_in_level
        offsets.append(offset)
        self.register_buffer('offsets', torch.from_numpy(np.array(offsets, dtype=np.int32)))
        self._host_offsets_py = tuple(int(o) for o in offsets)     # host copy for the library's LDS-path sizing
        self.n_params = offsets[-1] * level_dim
        self.embeddings = nn.Parameter(torch.empty(offset, level_dim))
        self.reset_parameters()

    def reset_parameters(self):
        self.embeddings.data.uniform_(-1e-4, 1e-4)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._host_offsets_py = None       # `offsets` may have been replaced: re-read it once on the next forward

    def forward(self, inputs, bound=1, normalized=False):
        """`normalized`: the inputs already are (x + bound) / (2 bound) (avatar.animate normalises while it gathers the rows)."""
        if not normalized:
            inputs = (inputs + bound) / (2 * bound)
        prefix_shape = list(inputs.shape[:-1])
        inputs = inputs.view(-1, self.input_dim)
        if self._host_offsets_py is None:
            self._host_offsets_py = tuple(int(o) for o in self.offsets.cpu().tolist())
        outputs = grid_encode(inputs, self.embeddings, self.offsets, self.per_level_scale, self.base_resolution,
                              inputs.requires_grad, self.gridtype_id, self.align_corners, self.interp_id,
                              _host_array(self._host_offsets_py))
        return outputs.view(prefix_shape + [self.output_dim])
