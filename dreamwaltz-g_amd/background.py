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
                                                        image, alpha and image_bg

The static 3D-Gaussian scene of `--render.use_gs_background PATH` (boundary B24: the reference's GaussianModel as a background,
core/system/scene.py:123-132) is here as well:

  load_gaussian_ply(path)                               the six tensors of GaussianModel.load_ply, read with numpy (no plyfile)
  GaussianBackground.from_ply / from_tensors / from_reference   frozen parameters under the reference's names; .gaussians(camera_positions)
                                                        -> the activated block (cached: one launch per parameter change)
  scene_merge(avatar_parts, background, camera_positions)   merge_gaussians(avatars..., background) in one launch per frame
  GaussianBackground.culled(cameras, H, W)              boundary B25: the scene Gaussians that may reach the image under the cameras, compacted
                                                        in index order into a CulledScene that scene_merge takes in place of the background
                                                        (cached per cameras and image size: csrc/scene_cull.hip, csrc/cull_math.h)"""
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


# --------------------------------------------------------------------------------------------------------------------------------------
# The static 3D-Gaussian scene (boundary B24: the reference's `--render.use_gs_background PATH`, a GaussianModel loaded from a .ply --
# core/gaussian/gaussian_model.py:97-171 -- and merged into every frame, core/system/scene.py:123-132)
# --------------------------------------------------------------------------------------------------------------------------------------
SCENE_MAX_PARTS, SCENE_SH_REST = _lib.CONSTANTS["DWG_SCENE_MAX_PARTS"], _lib.CONSTANTS["DWG_SCENE_SH_REST"]
ScenePartC = _lib.STRUCTS["dwg_scene_part"]
CULL_MAX_CAMERAS, CULL_CAMERA_FLOATS = _lib.CONSTANTS["DWG_SCENE_CULL_MAX_CAMERAS"], _lib.CONSTANTS["DWG_SCENE_CULL_CAMERA_FLOATS"]
CULL_MAX_ROWS, CullRowsC = _lib.CONSTANTS["DWG_SCENE_CULL_MAX_ROWS"], _lib.STRUCTS["dwg_scene_cull_rows"]

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_first_element(path):
    """(element name, {property: float64-castable array [count]}) of the FIRST element of a .ply (the reference reads `elements[0]`)."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError("%s: not a PLY file (no `ply` ... `end_header`)" % path)
    nl = raw.find(b"\n", end)
    body = raw[nl + 1:] if nl >= 0 else b""
    fmt, elements = None, []
    for line in raw[:end].decode("ascii", "replace").splitlines()[1:]:
        words = line.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else None
        elif words[0] == "element" and len(words) == 3:
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property" and elements:
            if len(elements) > 1:
                continue                                       # data behind the first element is never read
            if words[1] == "list":
                raise ValueError("%s: list property `%s` in element `%s`: a Gaussian scene has scalar properties only"
                                 % (path, words[-1], elements[0][0]))
            if len(words) != 3 or words[1] not in _PLY_TYPES:
                raise ValueError("%s: cannot read the property declaration `%s`" % (path, line.strip()))
            elements[0][2].append((words[2], _PLY_TYPES[words[1]]))
        else:
            raise ValueError("%s: cannot read the header line `%s`" % (path, line.strip()))
    if fmt not in ("binary_little_endian", "binary_big_endian", "ascii"):
        raise ValueError("%s: unknown PLY format `%s`" % (path, fmt))
    if not elements:
        raise ValueError("%s: no element in the header" % path)
    name, count, props = elements[0]
    if len({p for p, _ in props}) != len(props):
        raise ValueError("%s: a property of element `%s` is declared twice" % (path, name))
    if fmt == "ascii":
        tokens = body.split()
        if len(tokens) < count * len(props):
            raise ValueError("%s: %d values for %d x %d properties of element `%s`" % (path, len(tokens), count, len(props), name))
        table = np.array(tokens[:count * len(props)], dtype=np.float64).reshape(count, len(props))
        return name, {p: table[:, i].astype(t) for i, (p, t) in enumerate(props)}
    dtype = np.dtype([(p, ("<" if fmt == "binary_little_endian" else ">") + t) for p, t in props])
    if len(body) < count * dtype.itemsize:
        raise ValueError("%s: %d bytes of data for %d rows of %d bytes of element `%s`" % (path, len(body), count, dtype.itemsize, name))
    rec = np.frombuffer(body, dtype=dtype, count=count)
    return name, {p: rec[p] for p, _ in props}


def load_gaussian_ply(path, max_sh_degree: int = 3):
    """The six tensors of the reference's GaussianModel.load_ply (gaussian_model.py:97-147) from a 3DGS .ply, read with numpy alone:
    {'positions' [N, 3], 'sh_features_dc' [N, 1, 3], 'sh_features_rest' [N, (max_sh_degree + 1)^2 - 1, 3], 'opacities' [N, 1] (logits),
    'scales' [N, 3] (log), 'quaternions' [N, 4] (raw)}, fp32 on the CPU.  `f_rest_*` sorted by numeric suffix, reshaped (N, 3, 15), then
    transposed, as the reference does.  binary_little_endian, binary_big_endian and ascii; the first element; properties in any order;
    other properties (nx, ny, nz, ...) ignored; any scalar type (float and double are what such files carry).  ValueError for a wrong
    `f_rest_*` count, a missing property or a list property (the reference asserts there)."""
    name, cols = _ply_first_element(path)

    def numbered(prefix):
        try:
            return sorted((c for c in cols if c.startswith(prefix)), key=lambda c: int(c.split("_")[-1]))
        except ValueError:
            raise ValueError("%s: a `%s*` property without a numeric suffix" % (path, prefix)) from None

    def table(names):
        n = len(next(iter(cols.values()))) if cols else 0
        out = np.zeros((n, len(names)), dtype=np.float64)
        for i, c in enumerate(names):
            if c not in cols:
                raise ValueError("%s: element `%s` has no property `%s`" % (path, name, c))
            out[:, i] = cols[c]
        return out
    rest, scales, rots = numbered("f_rest_"), numbered("scale_"), numbered("rot")
    want = 3 * (max_sh_degree + 1) ** 2 - 3
    if len(rest) != want:
        raise ValueError("%s: %d `f_rest_*` properties, expected %d for max_sh_degree %d" % (path, len(rest), want, max_sh_degree))
    for names, n, what in ((scales, 3, "scale_0..2"), (rots, 4, "rot_0..3")):
        if len(names) != n:
            raise ValueError("%s: element `%s` has the properties %s, expected `%s`" % (path, name, names, what))
    xyz, opac, dc = table(["x", "y", "z"]), table(["opacity"]), table(["f_dc_0", "f_dc_1", "f_dc_2"])
    extra = table(rest).reshape(xyz.shape[0], 3, (max_sh_degree + 1) ** 2 - 1)
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)       # noqa: E731
    return {'positions': f32(xyz), 'sh_features_dc': f32(dc[:, :, None]).transpose(1, 2).contiguous(),
            'sh_features_rest': f32(extra).transpose(1, 2).contiguous(), 'opacities': f32(opac), 'scales': f32(table(scales)),
            'quaternions': f32(table(rots))}


def _camera_words(camera_positions):
    """(tensor, element stride) of a camera position on the device: data['c2w'][:, :3, 3] is read in place (stride 4)."""
    cam = camera_positions
    while cam.dim() > 1:
        if cam.shape[0] != 1:
            raise ValueError("one camera position per frame, got %s" % (tuple(camera_positions.shape),))
        cam = cam[0]
    if cam.numel() != 3:
        raise ValueError("camera_positions must hold 3 values, got %s" % (tuple(camera_positions.shape),))
    if cam.dtype != torch.float32 or cam.stride(0) < 1:
        cam = cam.float().contiguous()
    return cam, int(cam.stride(0))


CULL_CACHE_BLOCKS = 4            # culled blocks a GaussianBackground keeps
_CULL_CAMERA_KEYS = ('extrinsic', 'projection', 'c2w', 'tanfov', 'tanfov_x')


def _cull_camera_dicts(cameras):
    dicts = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras]
    if not dicts or not all(isinstance(d, dict) for d in dicts):
        raise TypeError("cameras: one camera dict, a list of them, or a [C, %d] fp32 device tensor of camera blocks" % CULL_CAMERA_FLOATS)
    return dicts


def _cull_camera_tensors(cameras):
    """The tensors a culled block's cameras are read from, in a fixed order (what the cache key identifies)."""
    if isinstance(cameras, torch.Tensor):
        return (cameras,)
    out = []
    for d in _cull_camera_dicts(cameras):
        if d.get('tanfov_dev') is not None:
            raise ValueError("culling under a camera whose field of view lives in device memory (data['tanfov_dev']) is not supported: the "
                             "cull reads data['tanfov'] on the host and would not follow the device value")
        for k in _CULL_CAMERA_KEYS:
            t = d.get(k)
            if t is None and k != 'tanfov_x':
                raise KeyError("a camera dict needs '%s'" % k)
            if t is not None:
                if not isinstance(t, torch.Tensor):
                    raise TypeError("camera dict: '%s' must be a tensor, got %s" % (k, type(t).__name__))
                out.append(t)
    return tuple(out)


def _cull_camera_blocks(cameras, dev):
    """[C, 37] fp32 on `dev`: per camera the 35 floats the renderer's own camera launch writes (dwg_raster_camera_setup: the very view and
    projection matrices the rasterizer reads), then tanfovx, tanfovy as the renderer passes them."""
    if isinstance(cameras, torch.Tensor):
        return cameras
    dicts = _cull_camera_dicts(cameras)
    blocks = torch.empty((len(dicts), CULL_CAMERA_FLOATS), dtype=torch.float32, device=dev)
    tanfov = []
    with torch.cuda.device(dev):
        for i, d in enumerate(dicts):
            mats = [d[k][0].to(dev).float().contiguous() for k in ('extrinsic', 'projection', 'c2w')]
            _lib.check(_lib.lib().dwg_raster_camera_setup(*(_lib.ptr(m) for m in mats), _lib.ptr(blocks[i]), _lib.stream(dev)),
                       "dwg_raster_camera_setup")
            ty = float(d['tanfov'][0])
            tanfov.append([float(d['tanfov_x'][0]) if d.get('tanfov_x') is not None else ty, ty])
    blocks[:, 35:] = torch.tensor(tanfov, dtype=torch.float32).to(dev)
    return blocks


class CulledScene:
    """The part of a GaussianBackground that may reach the image under a set of cameras (GaussianBackground.culled): what scene_merge
    reads of a background -- n_points (the kept count), activated(), _positions, _sh_features_dc / _sh_features_rest (sh_levels > 1 only,
    else None: the merge does not read them) and sh_levels -- over the kept rows in their original order, plus `index` (int32 [n_points],
    ascending: row k is scene Gaussian index[k]) and `n_total` (the scene's Gaussian count).  A copy: it does not follow later changes
    of the scene; `key` is the GaussianBackground.cull_key() it was computed under, and `camera_tensors` are the tensors that key
    identifies by address and version counter -- held here, so that no other tensor can get their addresses while the block is cached."""

    def __init__(self, key, n_total, sh_levels, index, rows, camera_tensors=()):
        self.key, self.n_total, self.sh_levels, self.index = key, int(n_total), int(sh_levels), index
        self.camera_tensors = tuple(camera_tensors)
        self._positions = rows['positions']
        self._sh_features_dc, self._sh_features_rest = rows.get('sh_features_dc'), rows.get('sh_features_rest')
        self._block = {k: rows[k] for k in ('opacities', 'scales', 'quaternions', 'colors')}

    @property
    def n_points(self) -> int:
        return int(self.index.shape[0])

    def activated(self) -> dict:
        return self._block


class GaussianBackground(nn.Module):
    """A static scene of N Gaussians behind the avatars.  Parameters carry the reference's names (GaussianModel: `_positions` [N, 3],
    `_sh_features_dc` [N, 1, 3], `_sh_features_rest` [N, 15, 3], `_opacities` [N, 1] logits, `_scales` [N, 3] log, `_quaternions` [N, 4]
    raw), so that a Scene's state_dict has the reference's `background.*` keys.  They are frozen: the reference has no optimizer for this
    background.  `sh_levels` 1 (the reference's hard-coded view-independent colour max(C0 dc + 0.5, 0)) .. 4 (view-dependent colour from
    the file's higher bands, renderer.compute_colors' semantics).  The activated block -- sigmoid, exp, F.normalize, DC colour: one launch
    -- is kept until optim.PARAM_EPOCH, a parameter's address or version counter, or invalidate_caches() says otherwise."""
    NAMES = ('_positions', '_sh_features_dc', '_sh_features_rest', '_opacities', '_scales', '_quaternions')

    def __init__(self, positions, sh_features_dc, sh_features_rest, opacities, scales, quaternions, sh_levels: int = 1):
        super().__init__()
        n = int(positions.shape[0])
        opacities = opacities.reshape(n, 1) if opacities.dim() == 1 else opacities
        given = dict(zip(self.NAMES, (positions, sh_features_dc, sh_features_rest, opacities, scales, quaternions)))
        tails = {'_positions': (3,), '_sh_features_dc': (1, 3), '_sh_features_rest': (None, 3), '_opacities': (1,), '_scales': (3,),
                 '_quaternions': (4,)}
        for k, t in given.items():
            if t.dim() != 1 + len(tails[k]) or t.shape[0] != n or any(w is not None and t.shape[1 + i] != w for i, w in enumerate(tails[k])):
                raise ValueError("GaussianBackground: %s has shape %s, expected [%d, %s]" % (k, tuple(t.shape), n, ", ".join(map(str, tails[k]))))
            setattr(self, k, nn.Parameter(t.detach().to(torch.float32).contiguous(), requires_grad=False))
        self.sh_levels = int(sh_levels)
        if not 1 <= self.sh_levels <= 4:
            raise ValueError("sh_levels must be 1..4, got %r" % (sh_levels,))
        if self.sh_levels > 1 and self._sh_features_rest.shape[1] != SCENE_SH_REST:
            raise ValueError("sh_levels %d reads the higher bands of a degree-3 file: _sh_features_rest must be [N, %d, 3], got %s"
                             % (self.sh_levels, SCENE_SH_REST, tuple(self._sh_features_rest.shape)))
        self.reference = None
        self.activation_launches = 0            # how often the activation kernel ran (the cache's counter)
        self._generation, self._cache, self._block = 0, None, None
        self.cull_launches = 0                  # how often culled() ran its kernels (the culled blocks' cache counter)
        self._cull_cache = {}                   # cull_key() -> CulledScene, least recently used first

    @classmethod
    def from_tensors(cls, positions, sh_features_dc, sh_features_rest, opacities, scales, quaternions, sh_levels: int = 1):
        return cls(positions, sh_features_dc, sh_features_rest, opacities, scales, quaternions, sh_levels=sh_levels)

    @classmethod
    def from_ply(cls, path, device=None, sh_levels: int = 1, max_sh_degree: int = 3):
        self = cls(**load_gaussian_ply(path, max_sh_degree=max_sh_degree), sh_levels=sh_levels)
        return self if device is None else self.to(device)

    @classmethod
    def from_reference(cls, ref_gaussian_model, sh_levels: int = 1):
        """Adopt a loaded reference GaussianModel (load_ply_and_initialize): its six parameters' storage, frozen here."""
        missing = [k for k in cls.NAMES if getattr(ref_gaussian_model, k, None) is None]
        if missing:
            raise ValueError("from_reference: the Gaussian model has no %s (load_ply_and_initialize first)" % ", ".join(missing))
        self = cls(*(getattr(ref_gaussian_model, k) for k in cls.NAMES), sh_levels=sh_levels)
        self.reference = [ref_gaussian_model]                  # kept alive, not registered as a submodule
        return self

    @property
    def n_points(self) -> int:
        return int(self._positions.shape[0])

    def invalidate_caches(self):
        self._generation += 1
        self._cache = None
        self._cull_cache = {}

    def reset_by_state_dict(self, state_dict):
        """GaussianModel.reset_by_state_dict (gaussian_model.py:58-85): resize the parameters to the checkpoint's Gaussian count."""
        for k in self.NAMES:
            v, cur = state_dict.get(k), getattr(self, k)
            if v is not None and v.dim() and cur.shape[0] != v.shape[0]:
                setattr(self, k, nn.Parameter(torch.empty(v.shape[0], *cur.shape[1:], dtype=cur.dtype, device=cur.device), requires_grad=False))
        self.invalidate_caches()

    def _cache_key(self):
        from . import optim
        ps = (self._opacities, self._scales, self._quaternions, self._sh_features_dc)
        return (optim.PARAM_EPOCH[0], self._generation,
                tuple((p.data_ptr(), 0 if p.is_inference() else p._version, tuple(p.shape)) for p in ps))

    def activated(self) -> dict:
        """{'opacities' [N, 1], 'scales' [N, 3], 'quaternions' [N, 4], 'colors' [N, 3] (the DC colour)}: cached, one launch when stale.
        A stale block is recomputed into the SAME tensors while the Gaussian count and the device stay: a graph captured earlier
        (player.GraphedAnimation) has their addresses baked in and must never find them freed.  The graph does not contain the activation,
        so after the scene's parameters change a replay shows the new values only once activated() has run again outside the graph."""
        key = self._cache_key()
        if self._cache is not None and self._cache[0] == key:
            return self._cache[1]
        n, dev = self.n_points, self._positions.device
        for k in self.NAMES:
            _lib.check_tensor(k, getattr(self, k), device=dev)
        capturing = torch.cuda.is_current_stream_capturing()
        block = None if capturing else self._block
        if block is None or block['opacities'].shape[0] != n or block['opacities'].device != dev:
            block = {'opacities': torch.empty((n, 1), dtype=torch.float32, device=dev), 'scales': torch.empty((n, 3), dtype=torch.float32, device=dev),
                     'quaternions': torch.empty((n, 4), dtype=torch.float32, device=dev), 'colors': torch.empty((n, 3), dtype=torch.float32, device=dev)}
        with torch.cuda.device(dev):
            rc = _lib.lib().dwg_scene_gaussians_activate(n, _lib.ptr(self._opacities), _lib.ptr(self._scales), _lib.ptr(self._quaternions),
                                                         _lib.ptr(self._sh_features_dc), _lib.ptr(block['opacities']), _lib.ptr(block['scales']),
                                                         _lib.ptr(block['quaternions']), _lib.ptr(block['colors']), _lib.stream(dev))
        _lib.check(rc, "dwg_scene_gaussians_activate")
        self.activation_launches += 1
        if not capturing:                                      # a block allocated inside a capture belongs to that graph's pool
            self._cache, self._block = (key, block), block
        return block

    def view_colors(self, camera_positions) -> torch.Tensor:
        """[N, 3]: the colour seen from `camera_positions` ([1, 3] or [3], a device tensor read in place) at this background's sh_levels."""
        if self.sh_levels == 1:
            return self.activated()['colors']
        if camera_positions is None:
            raise ValueError("sh_levels %d is view dependent: gaussians(camera_positions=) needs the camera position" % self.sh_levels)
        n, dev = self.n_points, self._positions.device
        cam, stride = _camera_words(camera_positions.to(dev))
        colors = torch.empty((n, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().dwg_scene_gaussians_colors(n, _lib.ptr(self._positions), _lib.ptr(self._sh_features_dc), _lib.ptr(self._sh_features_rest),
                                                       self.sh_levels, _lib.ptr(cam), stride, _lib.ptr(colors), _lib.stream(dev))
        _lib.check(rc, "dwg_scene_gaussians_colors")
        return colors

    def gaussians(self, camera_positions=None):
        """The activated scene as a GaussianOutput (positions: the parameter itself; sh_features None): what the reference's
        `background.forward()` + `compute_colors(..., sh_levels=1)` (scene.py:124-131) hands to merge_gaussians."""
        from .avatar import GaussianOutput
        block = self.activated()
        return GaussianOutput(positions=self._positions.detach(), opacities=block['opacities'], colors=self.view_colors(camera_positions),
                              scales=block['scales'], quaternions=block['quaternions'], sh_features=None)

    def forward(self, camera_positions=None):
        return self.gaussians(camera_positions)

    def get_optimizer(self, cfg=None):
        raise NotImplementedError("GaussianBackground is frozen: the reference has no optimizer for a Gaussian scene background either "
                                  "(its init_gaussian_solvers fails at background.get_optimizer)")

    # -- the per-camera cull (boundary B25, csrc/scene_cull.hip) --------------------------------------------------------------------------
    def cull_key(self, cameras, image_height, image_width):
        """What a culled block depends on: the activated block's key, the positions (and, at sh_levels > 1, the SH tables the compact
        block copies), `(data_ptr, _version, shape)` of every camera tensor, and the image size.  No launch, no host read."""
        ident = lambda t: (t.data_ptr(), 0 if t.is_inference() else t._version, tuple(t.shape))      # noqa: E731
        own = (self._positions,) + ((self._sh_features_dc, self._sh_features_rest) if self.sh_levels > 1 else ())
        return (self._cache_key(), tuple(ident(p) for p in own), tuple(ident(t) for t in _cull_camera_tensors(cameras)),
                int(image_height), int(image_width))

    def culled(self, cameras, image_height, image_width) -> "CulledScene":
        """The scene Gaussians that MAY reach an image_height x image_width image under any of `cameras` (one camera dict of the loader, a
        list of them -- the union: one block for all frames of a forward_frames call -- or a [C, 37] fp32 device tensor of camera blocks as
        dwg_raster_camera_block writes them), compacted in index order into a block that scene_merge takes in place of this background.
        The test (csrc/cull_math.h) never drops a Gaussian the rasterizer would give radius > 0, and the kept rows keep their relative
        order, so a frame merged from the culled block is the frame merged from the whole scene, bit for bit.  Cached like the activated
        block, under cull_key(): a hit launches nothing and reads nothing back; a miss runs flags, compaction and gather
        (`cull_launches` += 1) and reads the kept count back ONCE, to size the block.  The last CULL_CACHE_BLOCKS blocks are kept
        (a second camera does not evict the first), each with its camera tensors: a key identifies them by address, and a held tensor's
        address cannot pass to another camera's tensor.  Never inside a graph capture."""
        key = self.cull_key(cameras, image_height, image_width)
        hit = self._cull_cache.pop(key, None)
        if hit is not None:
            self._cull_cache[key] = hit                        # most recently used last
            return hit
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("GaussianBackground.culled: the culled block is not cached for these cameras and cannot be computed inside a "
                               "graph capture (its size is read back from the device): call culled() before the capture")
        n, dev, H, W = self.n_points, self._positions.device, int(image_height), int(image_width)
        if n > 0x7fffffff:
            raise ValueError("GaussianBackground.culled: %d Gaussians, the kept indices are int32" % n)
        block = self.activated()
        cams = _cull_camera_blocks(cameras, dev)
        _lib.check_tensor("camera blocks", cams, shape=(None, CULL_CAMERA_FLOATS), device=dev)
        C = int(cams.shape[0])
        if not 1 <= C <= CULL_MAX_CAMERAS:
            raise ValueError("GaussianBackground.culled: %d cameras, expected 1..%d" % (C, CULL_MAX_CAMERAS))
        _lib.check_tensor("_positions", self._positions, shape=(n, 3), device=dev)
        L = _lib.lib()
        index = torch.empty((n,), dtype=torch.int32, device=dev)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)
        if n:
            flags = torch.empty((n,), dtype=torch.uint8, device=dev)
            work = torch.empty((max(int(L.dwg_scene_cull_workspace_bytes(n)), 4),), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                _lib.check(L.dwg_scene_cull_flags(n, _lib.ptr(self._positions), _lib.ptr(block['scales']), C, _lib.ptr(cams), CULL_CAMERA_FLOATS,
                                                  H, W, _lib.ptr(flags), _lib.stream(dev)), "dwg_scene_cull_flags")
                _lib.check(L.dwg_scene_cull_compact(n, _lib.ptr(flags), _lib.ptr(index), _lib.ptr(count), _lib.ptr(work), _lib.stream(dev)),
                           "dwg_scene_cull_compact")
        kept = int(count.item())                               # the one host read of a cull: sizes the block and the chain's G
        index = index[:kept].clone()                           # the scene-sized scratch goes back to the allocator
        src = {'positions': self._positions.detach(), 'opacities': block['opacities'], 'scales': block['scales'],
               'quaternions': block['quaternions'], 'colors': block['colors']}
        if self.sh_levels > 1:
            src['sh_features_dc'], src['sh_features_rest'] = self._sh_features_dc.detach(), self._sh_features_rest.detach()
        out = {k: torch.empty((kept,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev) for k, t in src.items()}
        if kept:
            for k, t in src.items():
                _lib.check_tensor(k, t, device=dev)
            tables = (CullRowsC * CULL_MAX_ROWS)()
            for row, (k, t) in zip(tables, src.items()):
                row.src, row.dst, row.width = t.data_ptr(), out[k].data_ptr(), t[0].numel()
            with torch.cuda.device(dev):
                _lib.check(L.dwg_scene_cull_gather(kept, _lib.ptr(index), n, len(src), tables, _lib.stream(dev)), "dwg_scene_cull_gather")
        self.cull_launches += 1
        culled = self._cull_cache[key] = CulledScene(key, n, self.sh_levels, index, out, _cull_camera_tensors(cameras))
        while len(self._cull_cache) > CULL_CACHE_BLOCKS:
            del self._cull_cache[next(iter(self._cull_cache))]
        return culled


_MERGE_ATTRS = (("positions", 3), ("opacities", 1), ("colors", 3), ("scales", 3), ("quaternions", 4))


def _merge_launch(part_tensors, counts, background, camera_positions, out):
    """part_tensors: 5 dense fp32 tensors per avatar part, flat; the background's block goes last -> rows [0, sum) of the 5 `out` tensors."""
    dev = out[0].device
    block = background.activated()
    n_bg, levels = background.n_points, background.sh_levels
    if len(counts) + 1 > SCENE_MAX_PARTS:
        raise ValueError("a frame merges at most %d avatars with the scene, got %d" % (SCENE_MAX_PARTS - 1, len(counts)))
    parts = (ScenePartC * SCENE_MAX_PARTS)()
    for i, n in enumerate(counts):
        p = parts[i]
        p.positions, p.opacities, p.colors, p.scales, p.quaternions = (t.data_ptr() for t in part_tensors[5 * i:5 * i + 5])
        p.count = n
    p = parts[len(counts)]
    p.positions, p.opacities, p.scales, p.quaternions = (background._positions.data_ptr(), block['opacities'].data_ptr(),
                                                         block['scales'].data_ptr(), block['quaternions'].data_ptr())
    p.colors = block['colors'].data_ptr() if levels == 1 else None
    p.count = n_bg
    cam, stride = (None, 1)
    if levels > 1:
        if camera_positions is None:
            raise ValueError("sh_levels %d is view dependent: the merge needs the camera position" % levels)
        cam, stride = _camera_words(camera_positions.to(dev))
    total = sum(counts) + n_bg
    if any(int(o.shape[0]) != total for o in out):
        raise RuntimeError("scene_merge: %d rows for buffers of %s rows" % (total, [int(o.shape[0]) for o in out]))
    with torch.cuda.device(dev):
        rc = _lib.lib().dwg_scene_merge(len(counts) + 1, parts, levels, _lib.ptr(background._sh_features_dc), _lib.ptr(background._sh_features_rest),
                                        _lib.ptr(cam), stride, total, *(_lib.ptr(o) for o in out), _lib.stream(dev))
    _lib.check(rc, "dwg_scene_merge")


class _SceneMerge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, background, camera_positions, counts, shapes, *tensors):
        dev, total = tensors[0].device, sum(counts) + background.n_points
        out = tuple(torch.empty((total, w), dtype=torch.float32, device=dev) for _, w in _MERGE_ATTRS)
        _merge_launch([t.detach().reshape(-1, w).contiguous() for t, (_, w) in zip(tensors, _MERGE_ATTRS * len(counts))], counts, background,
                      camera_positions, out)
        ctx.counts, ctx.shapes = counts, shapes
        return out

    @staticmethod
    def backward(ctx, *grads):
        # the avatar parts get their row slices of the incoming gradients (what torch.cat's backward hands out); the scene gets none
        out, row = [], 0
        for i, n in enumerate(ctx.counts):
            for a in range(5):
                g = grads[a]
                k = 5 * i + a
                out.append(g[row:row + n].reshape(ctx.shapes[k]) if g is not None and ctx.needs_input_grad[4 + k] else None)
            row += n
        return (None, None, None, None) + tuple(out)


def scene_merge(avatar_parts, background: GaussianBackground, camera_positions=None, out=None):
    """merge_gaussians(*avatar_parts, background.gaussians(camera_positions)) (scene.py:107-132) in ONE launch: the five attributes of every
    part into rows [0, sum N) -- of `out` (five [sum N, .] fp32 tensors: rows of the stacked buffers a frames chain reads; no gradients) or of
    fresh tensors.  `background` may be a CulledScene (GaussianBackground.culled): only its kept rows are merged.  With gradients enabled and an avatar part that requires them the merge is an autograd function whose backward slices
    the incoming gradients per part.  -> GaussianOutput (sh_features None)."""
    from .avatar import GaussianOutput
    if not isinstance(background, (GaussianBackground, CulledScene)):
        raise TypeError("scene_merge needs a GaussianBackground, got %s" % type(background).__name__)
    tensors, counts = [], []
    dev = background._positions.device
    for i, g in enumerate(avatar_parts):
        if g.colors is None:
            raise NotImplementedError("scene_merge: avatar part %d has no precomputed `colors` (sh_features only): the merge with a Gaussian "
                                      "scene takes precomputed colours, as the reference's scene.py:123-132 produces for the scene" % i)
        n = int(g.positions.shape[0])
        for name, w in _MERGE_ATTRS:
            t = g[name]
            _lib.check_tensor("part %d %s" % (i, name), t, contiguous=False, device=dev)
            if t.numel() != n * w:
                raise RuntimeError("part %d: %s has shape %s, expected [%d, %d]" % (i, name, tuple(t.shape), n, w))
            tensors.append(t)
        counts.append(n)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        if out is not None:
            raise RuntimeError("scene_merge: no gradients through preallocated rows (out=)")
        res = _SceneMerge.apply(background, camera_positions, tuple(counts), tuple(tuple(t.shape) for t in tensors), *tensors)
    else:
        total = sum(counts) + background.n_points
        res = out if out is not None else tuple(torch.empty((total, w), dtype=torch.float32, device=dev) for _, w in _MERGE_ATTRS)
        for o, (name, w) in zip(res, _MERGE_ATTRS):
            _lib.check_tensor("out " + name, o, shape=(total, w), device=dev)
        _merge_launch([t.detach().reshape(-1, w).contiguous() for t, (_, w) in zip(tensors, _MERGE_ATTRS * len(counts))], counts, background,
                      camera_positions, res)
    return GaussianOutput(**{name: t for (name, _), t in zip(_MERGE_ATTRS, res)}, sh_features=None)
