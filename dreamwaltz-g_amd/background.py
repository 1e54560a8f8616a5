"""Video backgrounds on the device (boundary B5: the reference's VideoBackground, /root/reference/core/system/background.py:92-160, and
its compositing in Scene.forward, core/system/scene.py:157-160).

The reference converts the cached BGR uint8 frame on the host per rendered frame (cvtColor, cv2.resize when the sizes differ, `/ 255`)
and copies 12 bytes per pixel to the device.  Here the frames are uploaded ONCE per device (pinned staging, asynchronous copies) and stay
in HBM as uint8; conversion, resample and `image + bg * (1 - alpha)` are one launch over F frames (csrc/background.hip), with the frame
indices read from device memory -- no host work or sync per frame, and a captured frame can replay with another index.

  VideoBackground.from_frames(frames_bgr_uint8, fps)   frames [T, h, w, 3] (numpy array or tensor), as cv2 decodes them
  VideoBackground.from_reference(ref_bg)                the reference object's frame_cache (or its get_background(i) without preload)
  VideoBackground(path, preload=True)                   the reference's signature: decodes with cv2 (ImportError when it is missing)
  video_composite(image, alpha, background, frame_index) -> (image + image_bg * (1 - alpha), image_bg): autograd over the kernels

Frame indices behave like the reference's list: a negative index counts from the end, an index outside [-T, T) raises IndexError.  That
check is made on the host for Python ints; a device index tensor (GraphedAnimation's static input) is used as it is: the kernel wraps
negative values once and clamps the rest for memory safety.  No CPU fallback: image and alpha must be fp32 CUDA tensors.

The learned MLP background of stage II (boundary B23: the reference's MLPBackground, core/system/background.py:55-89, composited by
core/system/scene.py:161-164) is here too:

  MLPBackground()                                       encoder_bg = FreqEncoder(3, 4), bg_net = MLP(27, 3, 16, 2); forward(data, skip_bg) ->
                                                        [B, H, W, 3]; get_optimizer(cfg) -> optim.FlatAdan with the reference's values;
                                                        from_reference(ref_bg)
  background_dirs(c2w, intrinsics, H, W)                the unit view direction of every pixel of F cameras, one launch
  mlp_composite(image, alpha, image_bg)                 image + image_bg * (1 - alpha): autograd over one launch each way, gradients to
                                                        image, alpha and image_bg"""
import operator
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib

_STAGE_BYTES = 64 << 20          # pinned staging per upload chunk


def _cuda(device):
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("VideoBackground keeps its frames on the GPU (HIP kernels), got device %s" % device)
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _dense(t):
    """Non-overlapping and dense: the strides are a permutation of a contiguous layout (a tensor the composite may write at them)."""
    expect = 1
    for st, sz in sorted((st, sz) for st, sz in zip(t.stride(), t.shape) if sz != 1):
        if st != expect:
            return False
        expect *= sz
    return True


def _planar_strides(t, H, W):
    """(frame, pixel, channel) element strides of a [F, H, W, 3] tensor whose H and W merge into one pixel index, else None."""
    sf, sy, sx, sc = t.stride()
    if sy != W * sx and H > 1:
        return None
    return sf, sx, sc


class VideoBackground:
    """Frames of one video, kept per device as uint8 [T, h, w, 3] in the decoder's BGR order."""

    def __init__(self, path: str, preload: bool = True):
        """core/system/background.py:92-122.  The device store needs every frame, so all are decoded here whatever `preload` says."""
        try:
            import cv2
        except ImportError as e:
            raise ImportError("VideoBackground(path) decodes the video with OpenCV (cv2), which is not importable: decode the frames "
                              "elsewhere and use VideoBackground.from_frames(frames_bgr_uint8, fps)") from e
        if not os.path.isfile(path):
            raise FileNotFoundError(f"Video File Not Found: {path}")
        source = cv2.VideoCapture(path)
        try:
            fps, count = int(source.get(cv2.CAP_PROP_FPS)), int(source.get(cv2.CAP_PROP_FRAME_COUNT))
            frames = []
            for i in range(count):
                ret, frame = source.read()
                if not ret:
                    raise ValueError(f"Failed to Read Frame at Index: {i}")
                frames.append(frame)
        finally:
            source.release()
        self._setup(np.stack(frames) if frames else np.zeros((0, 1, 1, 3), np.uint8), fps)
        self.video_path, self.preload = path, preload

    @classmethod
    def from_frames(cls, frames_bgr_uint8, fps=30):
        """frames [T, h, w, 3] uint8, BGR (numpy array, CPU or CUDA tensor)."""
        self = cls.__new__(cls)
        self._setup(frames_bgr_uint8, fps)
        return self

    @classmethod
    def from_reference(cls, ref_bg):
        """Adopt the reference's VideoBackground: its frame_cache, or its own get_background(i) when it was built with preload=False.
        The reference object is kept (`.reference`): its __del__ releases the capture and removes a temporary video file."""
        cache = getattr(ref_bg, "frame_cache", None)
        if cache is None:
            cache = [ref_bg.get_background(i) for i in range(int(ref_bg.frame_count))]
        self = cls.__new__(cls)
        self._setup(np.stack([np.asarray(f) for f in cache]) if len(cache) else np.zeros((0, 1, 1, 3), np.uint8), getattr(ref_bg, "fps", 30))
        self.reference = ref_bg
        return self

    def _setup(self, frames, fps):
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if not isinstance(frames, torch.Tensor):
            raise TypeError("frames must be a numpy array or a tensor, got %s" % type(frames).__name__)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("frames must be uint8 [T, h, w, 3] (BGR), got %s %s" % (frames.dtype, tuple(frames.shape)))
        if frames.shape[0] == 0 or frames.shape[1] == 0 or frames.shape[2] == 0:
            raise ValueError("a video background needs at least one non-empty frame, got %s" % (tuple(frames.shape),))
        self.fps = int(fps)
        self.frame_count, self.frame_height, self.frame_width = (int(s) for s in frames.shape[:3])
        self.reference = None
        self._stores, self._tables = {}, {}
        if frames.is_cuda:
            self._host = None
            self._stores[frames.device] = frames.contiguous()
        else:
            self._host = frames.contiguous()

    # -- device store -------------------------------------------------------------------------------------------------------------------
    def frames(self, device=None) -> torch.Tensor:
        """The uint8 [T, h, w, 3] BGR store on `device`, uploaded on first use (asynchronously, on the current stream)."""
        device = _cuda(device)
        t = self._stores.get(device)
        if t is None:
            t = self._upload(device)
            self._stores[device] = t
        return t

    def _upload(self, device):
        T, h, w = self.frame_count, self.frame_height, self.frame_width
        dst = torch.empty((T, h, w, 3), dtype=torch.uint8, device=device)
        if self._host is None:                                             # frames given on another GPU
            dst.copy_(next(iter(self._stores.values())))
            return dst
        per = max(1, _STAGE_BYTES // (h * w * 3))
        for i in range(0, T, per):
            n = min(per, T - i)
            stage = torch.empty((n, h, w, 3), dtype=torch.uint8, pin_memory=True)     # the caching host allocator recycles a block only
            stage.copy_(self._host[i:i + n])                                          # after the copy that reads it has completed
            dst[i:i + n].copy_(stage, non_blocking=True)
        return dst

    def _table(self, device):
        t = self._tables.get(device)
        if t is None:
            t = torch.arange(self.frame_count, dtype=torch.int32, device=device)
            self._tables[device] = t
        return t

    def wrap(self, frame_index) -> int:
        """A host frame index as the reference's list takes it: negative from the end, IndexError outside [-T, T)."""
        i = operator.index(frame_index.item() if isinstance(frame_index, (torch.Tensor, np.ndarray)) else frame_index)
        if i < -self.frame_count or i >= self.frame_count:
            raise IndexError("frame index %d out of range for a video background of %d frames" % (i, self.frame_count))
        return i + self.frame_count if i < 0 else i

    def index_tensor(self, frame_index, device=None, count=None) -> torch.Tensor:
        """int32 [F] device tensor of frame indices: a CUDA tensor is used as it is (no host check); Python ints are checked and wrapped
        on the host and become a view of a per-device arange when they are consecutive (no copy at all), else a pinned asynchronous
        copy -- never a host sync."""
        device = _cuda(device)
        if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:
            idx = frame_index.reshape(-1)
            if idx.dtype != torch.int32:
                idx = idx.to(torch.int32)
            idx = idx.contiguous()
        else:
            if isinstance(frame_index, (torch.Tensor, np.ndarray)):
                frame_index = frame_index.reshape(-1).tolist() if frame_index.ndim else frame_index.item()
            items = [frame_index] if not isinstance(frame_index, (list, tuple)) else list(frame_index)
            items = [self.wrap(i) for i in items]
            if not items:
                raise ValueError("no frame index given")
            a = items[0]
            if items == list(range(a, a + len(items))):
                idx = self._table(device)[a:a + len(items)]
            else:
                idx = torch.tensor(items, dtype=torch.int32).pin_memory().to(device, non_blocking=True)
        if count is not None and idx.numel() != count:
            raise ValueError("%d frame indices for %d frames" % (idx.numel(), count))
        return idx

    # -- the reference's surface --------------------------------------------------------------------------------------------------------
    def get_background(self, frame_index, device=None) -> torch.Tensor:
        """The BGR frame as decoded: a uint8 [h, w, 3] device tensor (a view of the store)."""
        return self.frames(device)[self.wrap(frame_index)]

    def get_background_like(self, frame_index, image: torch.Tensor) -> torch.Tensor:
        """core/system/background.py:140-155: the RGB frame at image's size (image [B, H, W, 3]), in [0, 1] -> float [H, W, 3]."""
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise RuntimeError("get_background_like: image must be a CUDA tensor")
        H, W = int(image.shape[1]), int(image.shape[2])
        out = torch.empty((1, H, W, 3), dtype=torch.float32, device=image.device)
        _launch_forward(None, None, self, self.index_tensor(frame_index, image.device, count=1), None, out)
        return out[0] if image.dtype == torch.float32 else out[0].to(image.dtype)


def _launch_forward(fg, alpha, background, idx, image, image_bg):
    ref = image_bg if fg is None else fg
    F, H, W = int(ref.shape[0]), int(ref.shape[1]), int(ref.shape[2])
    device = ref.device
    store = background.frames(device)
    sf = sp = sc = 0
    if fg is not None:
        sf, sp, sc = _planar_strides(fg, H, W)
    rc = _lib.lib().dwg_video_composite_forward(F, H, W, _lib.ptr(fg), _lib.ptr(alpha), sf, sp, sc, _lib.ptr(store), background.frame_count,
                                                background.frame_height, background.frame_width, _lib.ptr(idx), _lib.ptr(image),
                                                _lib.ptr(image_bg), _lib.stream(device))
    _lib.check(rc, "dwg_video_composite_forward")


class _VideoComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, alpha, background, idx):
        F, H, W = (int(s) for s in image.shape[:3])
        out = torch.empty_strided(image.shape, image.stride(), dtype=torch.float32, device=image.device)
        image_bg = torch.empty((F, H, W, 3), dtype=torch.float32, device=image.device)
        _launch_forward(image, alpha, background, idx, out, image_bg)
        ctx.background = background
        ctx.save_for_backward(idx)
        ctx.mark_non_differentiable(image_bg)
        return out, image_bg

    @staticmethod
    def backward(ctx, d_out, d_bg):
        idx, = ctx.saved_tensors
        bg = ctx.background
        d_alpha = None
        if d_out is not None and ctx.needs_input_grad[1]:
            F, H, W = (int(s) for s in d_out.shape[:3])
            st = _planar_strides(d_out, H, W)
            if st is None or d_out.dtype != torch.float32:
                d_out = d_out.float().contiguous()
                st = _planar_strides(d_out, H, W)
            d_alpha = torch.empty((F, H, W, 1), dtype=torch.float32, device=d_out.device)
            store = bg.frames(d_out.device)
            rc = _lib.lib().dwg_video_composite_backward(F, H, W, _lib.ptr(d_out), st[0], st[1], st[2], _lib.ptr(store), bg.frame_count,
                                                         bg.frame_height, bg.frame_width, _lib.ptr(idx), _lib.ptr(d_alpha),
                                                         _lib.stream(d_out.device))
            _lib.check(rc, "dwg_video_composite_backward")
        return (d_out if ctx.needs_input_grad[0] else None), d_alpha, None, None


def video_composite(image: torch.Tensor, alpha: torch.Tensor, background: VideoBackground, frame_index):
    """image [F, H, W, 3] fp32 (any strides whose H, W merge: the renderer's planar view included), alpha [F, H, W, 1] fp32, one frame
    index per frame (int, list of ints or int32 CUDA tensor) -> (image + image_bg * (1 - alpha) at image's strides, image_bg [F, H, W, 3]
    contiguous).  Differentiable in image (d = d_out) and alpha (d = -sum_c d_out_c * bg_c); image_bg carries no gradient."""
    if not isinstance(background, VideoBackground):
        raise TypeError("video_composite needs a VideoBackground, got %s" % type(background).__name__)
    if image.dim() != 4 or image.shape[3] != 3:
        raise RuntimeError("image must be [F, H, W, 3], got %s" % (tuple(image.shape),))
    F, H, W = (int(s) for s in image.shape[:3])
    _lib.check_tensor("image", image, shape=(F, H, W, 3), contiguous=False)
    _lib.check_tensor("alpha", alpha, shape=(F, H, W, 1), contiguous=False)
    if _planar_strides(image, H, W) is None or not _dense(image):
        image = image.contiguous()
    alpha = alpha.contiguous()
    idx = background.index_tensor(frame_index, image.device, count=F)
    return _VideoComposite.apply(image, alpha, background, idx)


# --------------------------------------------------------------------------------------------------------------------------------------
# The learned (MLP) background of stage II (boundary B23: the reference's MLPBackground, core/system/background.py:55-89, and its
# compositing in Scene.forward, core/system/scene.py:161-164)
# --------------------------------------------------------------------------------------------------------------------------------------
CAMERA_FLOATS = _lib.CONSTANTS["DWG_BACKGROUND_CAMERA_FLOATS"]


def pack_cameras(c2w: torch.Tensor, intrinsics: torch.Tensor) -> torch.Tensor:
    """c2w [F, 4, 4] (or [F, 3, 4]) and intrinsics [F, 3, 3] -> the kernel's camera rows [F, 16] fp32: rows 0..2 of c2w, then fx, fy, cx,
    cy.  Device tensors stay on the device (no host read)."""
    if c2w.dim() != 3 or c2w.shape[1] < 3 or c2w.shape[2] != 4 or intrinsics.dim() != 3 or tuple(intrinsics.shape[1:]) != (3, 3):
        raise RuntimeError("c2w must be [F, 4, 4] and intrinsics [F, 3, 3], got %s and %s" % (tuple(c2w.shape), tuple(intrinsics.shape)))
    if intrinsics.shape[0] != c2w.shape[0]:
        raise RuntimeError("%d cameras and %d intrinsics" % (c2w.shape[0], intrinsics.shape[0]))
    K = intrinsics.to(device=c2w.device, dtype=torch.float32)
    return torch.cat([c2w[:, :3, :].to(torch.float32).reshape(-1, 12), K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3]], dim=1).contiguous()


def background_dirs(c2w: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """The unit view direction of every pixel of F cameras -> [F * H * W, 3] fp32 (one launch, csrc/background.hip k_background_dirs):
    get_rays' rays_d with N = -1 (core/nerf/nerf_utils.py:124-129) divided by its norm (background.py:78).  No gradients."""
    H, W = int(H), int(W)
    cams = pack_cameras(c2w.detach(), intrinsics.detach())
    _lib.check_tensor("c2w", cams)
    F = int(cams.shape[0])
    if F < 1 or H < 1 or W < 1:
        raise RuntimeError("background_dirs needs at least one camera and one pixel, got F=%d H=%d W=%d" % (F, H, W))
    dirs = torch.empty((F * H * W, 3), dtype=torch.float32, device=cams.device)
    with torch.cuda.device(cams.device):
        _lib.check(_lib.lib().dwg_background_dirs(F, _lib.ptr(cams), H, W, _lib.ptr(dirs), _lib.stream(cams.device)), "dwg_background_dirs")
    return dirs


class MLPBackground(nn.Module):
    """The reference's MLPBackground: a degree-4 frequency encoding of the pixel's view direction (27 columns), MLP(27, 3, 16, 2) and a
    sigmoid, on the fused kernels of nerf_background (B22) at that shape.  Checkpoint keys are the reference's: bg_net.net.{0,1}.{weight,
    bias} (under `background.` in a Scene)."""

    def __init__(self) -> None:
        super().__init__()
        from . import nerf_background, nerf_model
        self.encoder_bg = nerf_background.FreqEncoder(3, 4)
        self.bg_net = nerf_model.MLP(self.encoder_bg.output_dim, 3, 16, 2)
        self._optimizer = None

    @classmethod
    def from_reference(cls, ref_bg):
        """Adopt the reference's MLPBackground: its bg_net's weights and biases (the frequency encoder has none)."""
        self = cls()
        ref = [p for lin in ref_bg.bg_net.net for p in (lin.weight, lin.bias)]
        own = [p for lin in self.bg_net.net for p in (lin.weight, lin.bias)]
        if [tuple(p.shape) for p in ref] != [tuple(p.shape) for p in own]:
            raise RuntimeError("from_reference: bg_net has shapes %s, expected %s" % ([tuple(p.shape) for p in ref], [tuple(p.shape) for p in own]))
        with torch.no_grad():
            for p, q in zip(own, ref):
                p.copy_(q.detach().to(p.dtype))
        self.reference = [ref_bg]            # kept alive, not registered as a submodule
        return self

    def directions(self, data) -> torch.Tensor:
        if 'c2w' not in data or 'intrinsics' not in data:
            raise KeyError("MLPBackground reads data['c2w'] [B, 4, 4] and data['intrinsics'] [B, 3, 3] (core/system/background.py:69-70)")
        return background_dirs(data['c2w'], data['intrinsics'], data['image_height'], data['image_width'])

    def forward(self, data, skip_bg=False):
        """data: c2w [B, 4, 4], intrinsics [B, 3, 3], image_height, image_width -> image [B, H, W, 3] (zeros under skip_bg).  Two launches:
        the directions, then encoding + network + sigmoid."""
        from . import nerf_background
        c2w = data['c2w']
        B, H, W = int(c2w.shape[0]), int(data['image_height']), int(data['image_width'])
        if skip_bg:
            return torch.zeros(B, H, W, 3, device=c2w.device)
        image = nerf_background.learned_background(self.directions(data), self.encoder_bg, self.bg_net, sigmoid=True, precision=0)
        return image.view(B, H, W, 3)

    def get_optimizer(self, cfg=None):
        """The reference's Adan(lr=1e-3, eps=1e-8, weight_decay=2e-5, max_grad_norm=5.0) over this module's parameters as an
        optim.FlatAdan (built once: it re-homes the parameters into its flat buffers)."""
        from . import optim
        if self._optimizer is None:
            params = list(self.parameters())
            spec = optim.AdanSpec([{'params': params}], lr=0.001, eps=1e-8, weight_decay=2e-5, max_grad_norm=5.0)
            self._optimizer = optim.FlatAdan(spec, params[0].device, name="background")
        return self._optimizer


class _MLPComposite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, alpha, image_bg):
        F, H, W = (int(s) for s in image.shape[:3])
        out = torch.empty_strided(image.shape, image.stride(), dtype=torch.float32, device=image.device)
        sf, sp, sc = _planar_strides(image, H, W)
        with torch.cuda.device(image.device):
            rc = _lib.lib().dwg_mlp_composite_forward(F, H, W, _lib.ptr(image), _lib.ptr(alpha), sf, sp, sc, _lib.ptr(image_bg),
                                                      0 if image_bg.shape[0] == 1 and F > 1 else H * W * 3, _lib.ptr(out), _lib.stream(image.device))
        _lib.check(rc, "dwg_mlp_composite_forward")
        ctx.save_for_backward(alpha, image_bg)
        return out

    @staticmethod
    def backward(ctx, d_out):
        alpha, image_bg = ctx.saved_tensors
        need_fg, need_alpha, need_bg = ctx.needs_input_grad
        d_alpha = d_bg = None
        if need_alpha or need_bg:
            F, H, W = (int(s) for s in d_out.shape[:3])
            if image_bg.shape[0] != F:
                raise RuntimeError("mlp_composite: no backward through a background shared by several frames")
            st = _planar_strides(d_out, H, W)
            if st is None or d_out.dtype != torch.float32 or not _dense(d_out):
                d_out = d_out.float().contiguous()
                st = _planar_strides(d_out, H, W)
            if need_alpha:
                d_alpha = torch.empty((F, H, W, 1), dtype=torch.float32, device=d_out.device)
            if need_bg:
                d_bg = torch.empty((F, H, W, 3), dtype=torch.float32, device=d_out.device)
            with torch.cuda.device(d_out.device):
                rc = _lib.lib().dwg_mlp_composite_backward(F, H, W, _lib.ptr(d_out), st[0], st[1], st[2], _lib.ptr(alpha), _lib.ptr(image_bg),
                                                           _lib.ptr(d_alpha), _lib.ptr(d_bg), _lib.stream(d_out.device))
            _lib.check(rc, "dwg_mlp_composite_backward")
        return (d_out if need_fg else None), d_alpha, d_bg


def mlp_composite(image: torch.Tensor, alpha: torch.Tensor, image_bg: torch.Tensor) -> torch.Tensor:
    """image [F, H, W, 3] fp32 (any strides whose H, W merge: the renderer's planar view included), alpha [F, H, W, 1] fp32, image_bg
    [F, H, W, 3] fp32 -- or [1, H, W, 3], one background under all F frames (no gradients then) -- -> image + image_bg * (1 - alpha) at
    image's strides, one launch.  Differentiable in image (d = d_out), alpha (d = -sum_c d_out_c * bg_c) and image_bg
    (d = d_out * (1 - alpha)): one launch for the last two."""
    if image.dim() != 4 or image.shape[3] != 3:
        raise RuntimeError("image must be [F, H, W, 3], got %s" % (tuple(image.shape),))
    F, H, W = (int(s) for s in image.shape[:3])
    _lib.check_tensor("image", image, shape=(F, H, W, 3), contiguous=False)
    _lib.check_tensor("alpha", alpha, shape=(F, H, W, 1), contiguous=False, device=image.device)
    _lib.check_tensor("image_bg", image_bg, shape=(None, H, W, 3), contiguous=False, device=image.device)
    if image_bg.shape[0] != F and not (image_bg.shape[0] == 1 and not (torch.is_grad_enabled() and image_bg.requires_grad)):
        raise RuntimeError("image_bg holds %d frames for %d images" % (image_bg.shape[0], F))
    if _planar_strides(image, H, W) is None or not _dense(image):
        image = image.contiguous()
    return _MLPComposite.apply(image, alpha.contiguous(), image_bg.contiguous())
