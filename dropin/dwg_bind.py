"""dwg_bind -- binds the reference's OWN main.py / Trainer to the HIP path at import time, without editing a reference file.

Enable:   PYTHONPATH=<repo>/dropin:<repo>  DWG_BIND=1  python main.py --stage gs ...
(`dropin/sitecustomize.py` calls `install()` when DWG_BIND=1; or call `dwg_bind.install()` yourself before importing `core.*`.)

What gets bound, all through attributes the reference resolves AT CALL TIME (`from core.system.avatar import build_gaussian_avatar` etc.
sit inside Trainer methods: /root/reference/core/trainer.py:446-453,529-530), so replacing the module attribute is enough:

  B1  diff_gaussian_rasterization           dropin/diff_gaussian_rasterization/  (found through PYTHONPATH; nothing to patch)
  B2  core.nerf.gridencoder backend         dropin/_gridencoder.py               (found through PYTHONPATH before the JIT build)
  B6  _raymarchingrgb / _raymarchinglatent  dropin/_raymarching{rgb,latent}.py    (found through PYTHONPATH; nothing to patch -- the NeRF
                                             stage's ray marcher, core/nerf/raymarching/*/raymarching.py:14-27)
  B7  core.nerf.nerf_model.build_NeRFNetwork (nerf_model.py:565-574)  -> the reference builds ITS network (resolved at call time:
                                             trainer.py:499-501), then dreamwaltz_g_amd.nerf.bind_nerf_network rebinds common_forward and
                                             local_geometry_forward of that object to the fused field kernel (grid encoding -> sigma_net ->
                                             density / albedo); density, forward and normal reach it through them; with cuda_ray it also installs
                                             update_extra_state on the native occupancy update (B13, dreamwaltz_g_amd.occupancy) and
                                             run_cuda on the one-launch inference render (dreamwaltz_g_amd.nerf_render: an evaluation view
                                             with shading 'albedo', B14, and -- bound here with shaded_render=True -- the shaded view the
                                             trainer renders beside it, B15: 'normal' without autocast or under fp16 autocast, 'textureless'
                                             and rgb 'lambertian' without autocast, the seven field evaluations per sample, the
                                             finite-difference normal and the shading inside the one launch; latent 'lambertian' and the
                                             lambert shadings under autocast stay on the reference's loop; with DWG_BIND_NERF_TRAIN=1
                                             also the training view with shading 'albedo', B18: march, field and composite as one autograd
                                             function whose backward runs over the samples the composite used).  The
                                             network's own Parameters are read in place.  What the kernel does not cover (dual_mlp / dual_enc,
                                             density_prior smpl, a decoder_layer, a non-grid backbone) stays unbound with the reason in
                                             `_dwg_nerf_unbound`.  DWG_BIND_NERF=0: nothing is bound
  B8  core.trainer.Trainer.calc_sigma_loss (trainer.py:718-825)     -> dreamwaltz_g_amd.sigma_guidance.calc_sigma_loss: the SMPL-X sigma
                                             guidance's geometry (part-mesh normals, area-weighted samples, point-to-mesh distance, keep
                                             mask) on the device instead of trimesh + igl on the host, with no host sync; the loss runs
                                             on the reference's own network (B7 when bound).  CPU vertices and unknown sigma_loss_types
                                             go to the original method.  The samples are drawn from torch's CUDA generator: the same
                                             distribution as trimesh's, not the same draws.  DWG_BIND_SIGMA=0: nothing is bound
  B9  core.trainer.Trainer.pretrain_forward (trainer.py:1242-1279)   -> dreamwaltz_g_amd.pretrain.pretrain_forward: the pretrain recipe's
                                             two MSE terms against the SMPL-X depth map as one fused forward and one fused backward
                                             launch; the map stays on the device when the loader hands a condition.DepthMap (INTEGRATION
                                             B9), an np.ndarray is uploaded.  visual_outputs is built only when time_to_snapshot.  CPU
                                             renders go to the original method.  DWG_BIND_PRETRAIN=0: nothing is bound
  B17 core.trainer.Trainer.init_losses (trainer.py:633-645) and Trainer.pretrain_nerf2gs_forward (trainer.py:1370-1386), the nerf2gs
                                             loop (`--log.nerf2gs`) -> dreamwaltz_g_amd.image_loss: init_losses runs the original; where
                                             that fails because core/gaussian/gaussian_loss.py imports the absent pytorch3d, it runs once
                                             more with cfg.log.nerf2gs off (restored afterwards); with cfg.log.nerf2gs set, losses['image']
                                             is the native ImageReconstructionLoss (L1 + D-SSIM, one forward and one backward launch
                                             chain).  pretrain_nerf2gs_forward renders once; a device render goes to
                                             image_loss.nerf2gs_forward, which reads both [B, H, W, C] renders in place; a CPU render goes
                                             to the original method.  DWG_BIND_NERF2GS=0: nothing is bound
  B3  core.system.avatar.build_gaussian_avatar (avatar.py:1642-1714)  -> the reference builds ITS avatar (point cloud, nearest triangles,
                                             inverse LBS, LBS weights ...), then `DreamWaltzG.from_reference(ref)` adopts every Parameter
                                             and buffer by name; non-DreamWaltzG gs_types are returned untouched (reference path)
  B11 core.system.avatar.find_nearest_triangles (avatar.py:766-806), knn_points (avatar.py:24-34) and
      LBSUtils.initialize_lbs_weights (avatar.py:865-911)            -> dreamwaltz_g_amd.avatar_init: the constructor-time geometry of
                                             that avatar (and of every reset_by_state_dict) on the device instead of libigl, pytorch3d
                                             and a torch loop: closest faces and barycentric coordinates, exact K nearest neighbours,
                                             the interpolated LBS weights and their smooth_N Jacobi sweeps.  All three are resolved at call
                                             time, so build_gaussian_avatar, reset_by_state_dict and the module's other knn_points callers
                                             reach them; the results come back in the reference's containers, dtypes and placements.
                                             Without a HIP device the originals run.  DWG_BIND_INIT=0: nothing is bound
  B12 core.nerf.to_point_cloud.export_point_cloud (to_point_cloud.py:27-92) and remove_points_inside_bboxes (:95-114), both resolved at
      call time by Trainer.init_gaussian_model (trainer.py:544)  -> dreamwaltz_g_amd.pointcloud: the density of the fused field (B7's
                                             kernel) once per lattice point, an ordered on-device selection, and albedo + the six
                                             finite-difference evaluations for the survivors only, instead of seven evaluations of every
                                             lattice point, four host copies per chunk and a Python loop over the points.  The export
                                             wrapper runs the reference's own preamble on the reference's network (update_extra_state,
                                             the resolution and threshold defaults), returns the reference's BasicPointCloud (float64
                                             numpy) and logs its two lines.  Without a HIP device, for a network B7 does not cover or with
                                             CPU parameters the originals run.  DWG_BIND_POINTCLOUD=0: nothing is bound
  B5  core.system.scene.build_scene (scene.py:224-245)                -> dreamwaltz_g_amd.scene.Scene around that avatar (same forward /
                                             state_dict / avatar.get_optimizer surface the Trainer uses: trainer.py:578-604,680-709,859-890).
                                             `--render.use_video_background`: the reference's VideoBackground decodes the video, and
                                             dreamwaltz_g_amd.background.VideoBackground.from_reference adopts its frames on the device
  B4  core.guidance.controlnet.ControlNetScoreDistillation (controlnet.py:75-114) -> the reference constructs its object as always
                                             (diffusers pipeline, text encoder, schedulers); after __init__ the two hot methods of THAT object,
                                             `_predict` (controlnet.py:83-114) and `encode_images` (vae.py:34-40), are bound to the HIP plans
                                             built from the loaded modules' state_dict()s.  Everything else (get_text_embeds, __call__,
                                             calc_gradients, tp_scheduler, pipe, decode_latents, isinstance checks) is the reference's own
                                             (decode_latents: unless DWG_BIND_VAE_DECODER=1, below).

Environment: DWG_BIND_NERF = 0                        leave the NeRF stage's field network (B7) on the reference path
             DWG_BIND_NERF_TRAIN = 1                  also bind the NeRF stage's training render (B18, nerf_render.render_rays_train);
                                 = shaded             and its shaded training views (B19: shading 'normal', 'textureless', 'lambertian', as the
                                                     normal-adapted guidance renders them); unset or any other value: training calls of run_cuda
                                                     stay on the reference's statements
             DWG_BIND_NERF_VIEW = 1                   also bind the NeRF network's render() (B20, nerf.bind_nerf_view: rays, the background
                                                     mix and the planar image in one launch each; a network built with bg_mode 'nerf' -- it
                                                     has a bg_net and an encoder_bg -- also gets its learned background from one launch, B22:
                                                     dreamwaltz_g_amd.nerf_background); unset or any other value: render() is the reference's
             DWG_BIND_MLP_BACKGROUND = 1              also bind `--render.use_mlp_background` (B23): the reference's own MLPBackground is built
                                                     and adopted by dreamwaltz_g_amd.background.MLPBackground.from_reference, and its
                                                     get_optimizer() is the fused Adan (optim.FlatAdan); unset or any other value: the bound
                                                     build_scene refuses that flag as before
             DWG_BIND_INIT = 0                        leave the avatar constructor's geometry (B11) on the reference path (igl + pytorch3d)
             DWG_BIND_POINTCLOUD = 0                  leave the NeRF-to-Gaussian point-cloud export (B12) on the reference path
             DWG_BIND_SIGMA = 0                       leave Trainer.calc_sigma_loss (B8) on the reference path (trimesh + igl)
             DWG_BIND_PRETRAIN = 0                    leave Trainer.pretrain_forward (B9) on the reference path (numpy on the host)
             DWG_BIND_NERF2GS = 0                     leave Trainer.init_losses / pretrain_nerf2gs_forward (B17) on the reference path (pytorch3d)
             DWG_BIND_DTYPE = f32x | f32 | f16 | bf16  storage type of the denoiser / VAE plans.  Unset: the precision the reference loaded its
                                                     pipeline in -- torch.float32 (its default, core/guidance/basic.py:233) -> f32x (fp32-grade
                                                     split precision on the 16-bit MFMA pipe), torch.float16 (`--guide.dtype fp16`,
                                                     basic.py:24-27) -> f16.  bf16 narrows the user's precision: only on request
             DWG_BIND_VAE_DECODER = 1                also bind `decode_latents` (B26, vae.py:42-46: every snapshot and evaluation frame of a latent
                                                     NeRF, the grad_viz pictures, the x0 losses' targets) to sd15.VAEDecoderPlan, fed from
                                                     post_quant_conv.* / decoder.* of the loaded VAE; 'pt' outputs of device tensors only, anything
                                                     else goes to the original method.  Unset or any other value: decode_latents is the reference's
             DWG_BIND_KEEP_MODULES = 1               keep the diffusers UNet / ControlNet on the GPU (default: moved to the CPU once their
                                                     weights live in the plans -- the text encoder and the VAE decoder stay where they were)
"""
import importlib
import importlib.abc
import importlib.util
import os
import sys
import types

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_PATCHED = "__dwg_bound__"


def _pkg():
    if _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)
    import dwg_import  # noqa: F401
    import dreamwaltz_g_amd
    return dreamwaltz_g_amd


# --------------------------------------------------------------------------------------------------------------------------------------
# B3: avatar
# --------------------------------------------------------------------------------------------------------------------------------------
def bind_avatar(ref_avatar):
    """reference DreamWaltzG -> HIP-backed DreamWaltzG with the same tensors; anything else is returned as it is."""
    if type(ref_avatar).__name__ != "DreamWaltzG" or getattr(ref_avatar, _PATCHED, False):
        return ref_avatar
    _pkg()
    from dreamwaltz_g_amd.avatar import DreamWaltzG
    av = DreamWaltzG.from_reference(ref_avatar)
    setattr(av, _PATCHED, True)
    return av


def _patch_avatar_module(mod):
    orig = mod.build_gaussian_avatar
    if getattr(orig, _PATCHED, False):
        return

    def build_gaussian_avatar(*args, **kwargs):
        return bind_avatar(orig(*args, **kwargs))
    build_gaussian_avatar.__doc__ = orig.__doc__
    setattr(build_gaussian_avatar, _PATCHED, True)
    build_gaussian_avatar.__wrapped__ = orig
    mod.build_gaussian_avatar = build_gaussian_avatar


# --------------------------------------------------------------------------------------------------------------------------------------
# B11: the avatar constructor's geometry
# --------------------------------------------------------------------------------------------------------------------------------------
def _hip_device():
    """The current HIP device, or None when the process has none (then the B11 wrappers call the reference's functions)."""
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None


def _on(dev, x, dtype):
    import numpy as np
    import torch
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return torch.as_tensor(x).detach().to(device=dev, dtype=dtype)


def _patch_avatar_init(mod):
    if os.environ.get("DWG_BIND_INIT", "1") == "0":
        return
    import functools
    orig_fnt, orig_knn = mod.find_nearest_triangles, mod.knn_points
    utils = mod.LBSUtils
    orig_init = utils.__dict__["initialize_lbs_weights"]
    orig_init = getattr(orig_init, "__func__", orig_init)
    if getattr(orig_fnt, _PATCHED, False):
        return

    @functools.wraps(orig_fnt)
    def find_nearest_triangles(points, vertices, triangles, device=None):
        dev = _hip_device()
        if dev is None:
            return orig_fnt(points, vertices, triangles, device=device)
        import torch
        _pkg()
        from dreamwaltz_g_amd import avatar_init
        # torch.tensor(x, device=None) of the reference lands on the CPU
        return avatar_init.find_nearest_triangles(_on(dev, points, torch.float32), _on(dev, vertices, torch.float32), _on(dev, triangles, torch.int64),
                                                  device="cpu" if device is None else device)

    @functools.wraps(orig_knn)
    def knn_points(query_points, reference_points, K=3, device=None):
        dev = _hip_device()
        if dev is None:
            return orig_knn(query_points, reference_points, K=K, device=device)
        import torch
        _pkg()
        from dreamwaltz_g_amd import avatar_init
        if device is None:
            device = query_points.device
        res = avatar_init.knn_points(_on(dev, query_points, torch.float32), _on(dev, reference_points, torch.float32), K=K, device=device)
        try:
            from pytorch3d.ops.knn import _KNN
        except Exception:
            return res                                            # same field names
        return _KNN(dists=res.dists, idx=res.idx, knn=None)

    @functools.wraps(orig_init)
    def initialize_lbs_weights(lbs_model, nearest_triangles_buffer, positions=None, smooth=False, smooth_K=None, smooth_N=None, use_sqrt=True,
                               valid_dist_threshold=0.01):
        dev = _hip_device()
        if dev is None:
            return orig_init(lbs_model, nearest_triangles_buffer, positions=positions, smooth=smooth, smooth_K=smooth_K, smooth_N=smooth_N,
                             use_sqrt=use_sqrt, valid_dist_threshold=valid_dist_threshold)
        import torch
        _pkg()
        from dreamwaltz_g_amd import avatar_init
        table = lbs_model.lbs_weights
        out = avatar_init.initialize_lbs_weights(_on(dev, table, torch.float32), nearest_triangles_buffer,
                                                 positions=None if positions is None else _on(dev, positions, torch.float32), smooth=smooth,
                                                 smooth_K=smooth_K, smooth_N=smooth_N, use_sqrt=use_sqrt, valid_dist_threshold=valid_dist_threshold)
        return out.to(table.device)

    for f, orig in ((find_nearest_triangles, orig_fnt), (knn_points, orig_knn), (initialize_lbs_weights, orig_init)):
        setattr(f, _PATCHED, True)
        f.__wrapped__ = orig
    mod.find_nearest_triangles = find_nearest_triangles
    mod.knn_points = knn_points
    utils.initialize_lbs_weights = staticmethod(initialize_lbs_weights)


def _patch_avatar_hooks(mod):
    _patch_avatar_module(mod)
    _patch_avatar_init(mod)


# --------------------------------------------------------------------------------------------------------------------------------------
# B7: the NeRF stage's field network
# --------------------------------------------------------------------------------------------------------------------------------------
def bind_nerf(ref):
    """Bind a constructed reference NeRF network to the fused field kernel; returns it (bound or, with the reason recorded, not)."""
    if os.environ.get("DWG_BIND_NERF", "1") == "0":
        return ref
    _pkg()
    from dreamwaltz_g_amd.nerf import bind_nerf_network
    if os.environ.get("DWG_BIND_NERF_TRAIN", "0") == "shaded":
        reason = bind_nerf_network(ref, shaded_render=True, train_render='shaded')
    elif os.environ.get("DWG_BIND_NERF_TRAIN", "0") == "1":
        reason = bind_nerf_network(ref, shaded_render=True, train_render=True)
    else:
        reason = bind_nerf_network(ref, shaded_render=True)
    if reason is not None:
        print("[dwg_bind] NeRF field left on the reference path: %s" % reason, file=sys.stderr)
    elif os.environ.get("DWG_BIND_NERF_VIEW", "0") == "1":
        from dreamwaltz_g_amd.nerf import bind_nerf_view
        reason = bind_nerf_view(ref)
        if reason is not None:
            print("[dwg_bind] NeRF render() left on the reference path: %s" % reason, file=sys.stderr)
    return ref


def _patch_nerf_module(mod):
    orig = mod.build_NeRFNetwork
    if getattr(orig, _PATCHED, False):
        return

    def build_NeRFNetwork(cfg):
        return bind_nerf(orig(cfg))
    build_NeRFNetwork.__doc__ = orig.__doc__
    setattr(build_NeRFNetwork, _PATCHED, True)
    build_NeRFNetwork.__wrapped__ = orig
    mod.build_NeRFNetwork = build_NeRFNetwork


# --------------------------------------------------------------------------------------------------------------------------------------
# B12: the point-cloud export between the NeRF and the Gaussian stage
# --------------------------------------------------------------------------------------------------------------------------------------
def _export_covered(net):
    """The native export takes this network: a HIP device, a field B7 covers, parameters on the device."""
    if _hip_device() is None:
        return False
    _pkg()
    from dreamwaltz_g_amd import nerf
    if nerf.unbound_reason(net) is not None:
        return False
    return all(p.is_cuda for p in net.parameters())


def _patch_pointcloud_module(mod):
    if os.environ.get("DWG_BIND_POINTCLOUD", "1") == "0":
        return
    import functools
    orig_export, orig_remove = mod.export_point_cloud, mod.remove_points_inside_bboxes
    if getattr(orig_export, _PATCHED, False):
        return

    @functools.wraps(orig_export)
    def export_point_cloud(self, resolution=None, split_size=128, density_thresh=None):
        if not _export_covered(self):
            return orig_export(self, resolution=resolution, split_size=split_size, density_thresh=density_thresh)
        import numpy as np
        import torch
        from dreamwaltz_g_amd import pointcloud
        with torch.inference_mode():                        # the reference's decorator
            return _export(self, resolution, split_size, density_thresh, np, pointcloud)

    def _export(self, resolution, split_size, density_thresh, np, pointcloud):
        logger = mod.logger
        logger.info(f'Extracting point cloud from NeRF...')
        # the reference's preamble on the reference's object (to_point_cloud.py:32-46)
        self.update_extra_state()
        if resolution is None:
            resolution = self.grid_size
        if density_thresh is None:
            if self.cuda_ray:
                density_thresh = min(self.mean_density, self.density_thresh) \
                    if np.greater(self.mean_density, 0) else self.density_thresh
            else:
                density_thresh = self.density_thresh
        if self.density_activation == 'softplus':          # as the reference reads: on _NeRFNetwork a function against a string, False
            density_thresh = density_thresh * 25
        native = pointcloud.export_point_cloud_from(self, resolution=resolution, split_size=split_size, density_thresh=density_thresh)
        pc = native.to_basic(mod.BasicPointCloud)
        min_density = min(self.max_density, native.info["min_density"])
        max_density = max(0.0, native.info["max_density"])
        logger.info(f'Extracting point cloud done! Obtain {pc.points.shape[0]} points!')
        logger.info(f'    density thresh: {density_thresh} ({min_density} ~ {max_density})')
        return pc

    @functools.wraps(orig_remove)
    def remove_points_inside_bboxes(point_cloud, bboxes):
        if _hip_device() is None:
            return orig_remove(point_cloud, bboxes)
        _pkg()
        from dreamwaltz_g_amd import pointcloud
        try:
            pointcloud.parse_boxes(bboxes)
            return pointcloud.remove_points_inside_bboxes(point_cloud, bboxes)
        except TypeError:                                   # a nesting or point values the device test does not take: the reference's loop
            return orig_remove(point_cloud, bboxes)

    for f, orig in ((export_point_cloud, orig_export), (remove_points_inside_bboxes, orig_remove)):
        setattr(f, _PATCHED, True)
        f.__wrapped__ = orig
    mod.export_point_cloud = export_point_cloud
    mod.remove_points_inside_bboxes = remove_points_inside_bboxes


# --------------------------------------------------------------------------------------------------------------------------------------
# B8: the NeRF stage's SMPL-X sigma guidance
# --------------------------------------------------------------------------------------------------------------------------------------
def _sigma_covered(trainer, data):
    verts = getattr(data.get('smpl_outputs') if isinstance(data, dict) else None, 'vertices', None)
    if verts is None or not getattr(verts, 'is_cuda', False):
        return False
    _pkg()
    from dreamwaltz_g_amd.sigma_guidance import LOSS_TYPES
    return getattr(trainer.cfg, 'sigma_loss_type', None) in LOSS_TYPES


def _patch_trainer_module(mod):
    _patch_trainer_sigma(mod)
    _patch_trainer_pretrain(mod)
    _patch_trainer_nerf2gs(mod)


def _patch_trainer_sigma(mod):
    if os.environ.get("DWG_BIND_SIGMA", "1") == "0":
        return
    cls = mod.Trainer
    orig = cls.calc_sigma_loss
    if getattr(orig, _PATCHED, False):
        return
    import functools

    @functools.wraps(orig)
    def calc_sigma_loss(self, data, render_outputs, sd_inputs, selected_parts, wo_wrist: bool = True):
        if not _sigma_covered(self, data):
            return orig(self, data, render_outputs, sd_inputs, selected_parts, wo_wrist=wo_wrist)
        from dreamwaltz_g_amd.sigma_guidance import calc_sigma_loss as native
        return native(self, data, render_outputs, sd_inputs, selected_parts, wo_wrist=wo_wrist, logger=getattr(mod, 'logger', None))
    setattr(calc_sigma_loss, _PATCHED, True)
    calc_sigma_loss.__wrapped__ = orig
    cls.calc_sigma_loss = calc_sigma_loss


# --------------------------------------------------------------------------------------------------------------------------------------
# B9: the NeRF pretrain step against the SMPL-X depth map
# --------------------------------------------------------------------------------------------------------------------------------------
class _RenderedOnce:
    """Stands for the trainer inside pretrain_forward (the native one or the wrapped original) once the render has been made."""

    def __init__(self, trainer, render_outputs):
        self._trainer, self._render_outputs = trainer, render_outputs

    def render(self, data):
        return self._render_outputs

    def __getattr__(self, name):
        return getattr(self._trainer, name)


def _patch_trainer_pretrain(mod):
    if os.environ.get("DWG_BIND_PRETRAIN", "1") == "0":
        return
    cls = mod.Trainer
    orig = cls.pretrain_forward
    if getattr(orig, _PATCHED, False):
        return
    import functools

    @functools.wraps(orig)
    def pretrain_forward(self, data):
        once = _RenderedOnce(self, self.render(data=data))
        if not getattr(once._render_outputs.get('depth'), 'is_cuda', False):
            return orig(once, data)                                # a CPU render: the reference's own statements fit it
        _pkg()
        from dreamwaltz_g_amd.pretrain import pretrain_forward as native
        return native(once, data)
    setattr(pretrain_forward, _PATCHED, True)
    pretrain_forward.__wrapped__ = orig
    cls.pretrain_forward = pretrain_forward


# --------------------------------------------------------------------------------------------------------------------------------------
# B17: the nerf2gs loop's image loss
# --------------------------------------------------------------------------------------------------------------------------------------
def _patch_trainer_nerf2gs(mod):
    if os.environ.get("DWG_BIND_NERF2GS", "1") == "0":
        return
    cls = mod.Trainer
    orig_losses, orig_forward = cls.init_losses, cls.pretrain_nerf2gs_forward
    if getattr(orig_losses, _PATCHED, False):
        return
    import functools

    @functools.wraps(orig_losses)
    def init_losses(self):
        log = self.cfg.log
        try:
            losses = orig_losses(self)
        except ModuleNotFoundError as e:
            # core/gaussian/gaussian_loss.py imports pytorch3d at module level (for a regularizer nothing calls); without it the
            # reference cannot build losses['image'].  Everything else of init_losses is built with the switch off
            if not (e.name or "").startswith("pytorch3d") or not log.nerf2gs:
                raise
            saved = log.nerf2gs
            log.nerf2gs = False
            try:
                losses = orig_losses(self)
            finally:
                log.nerf2gs = saved
        if log.nerf2gs:
            _pkg()
            from dreamwaltz_g_amd.image_loss import ImageReconstructionLoss
            losses['image'] = ImageReconstructionLoss()
        return losses

    @functools.wraps(orig_forward)
    def pretrain_nerf2gs_forward(self, data):
        once = _RenderedOnce(self, self.render(data=data))
        if not getattr(once._render_outputs.get('image_fg'), 'is_cuda', False):
            return orig_forward(once, data)                        # a CPU render: the reference's own statements fit it
        _pkg()
        from dreamwaltz_g_amd.image_loss import nerf2gs_forward as native
        return native(once, data)

    for f, orig in ((init_losses, orig_losses), (pretrain_nerf2gs_forward, orig_forward)):
        setattr(f, _PATCHED, True)
        f.__wrapped__ = orig
    cls.init_losses = init_losses
    cls.pretrain_nerf2gs_forward = pretrain_nerf2gs_forward


# --------------------------------------------------------------------------------------------------------------------------------------
# B5: scene
# --------------------------------------------------------------------------------------------------------------------------------------
def _patch_scene_module(mod):
    orig = mod.build_scene
    if getattr(orig, _PATCHED, False):
        return

    def build_scene(cfg, avatar):
        items = avatar if isinstance(avatar, (list, tuple)) else [avatar]
        if not all(getattr(a, _PATCHED, False) for a in items):
            return orig(cfg=cfg, avatar=avatar)            # not ours (another gs_type): the reference's scene
        _pkg()
        from dreamwaltz_g_amd.scene import Scene
        import torch
        r = cfg.render
        mlp = bool(r.use_mlp_background) and os.environ.get("DWG_BIND_MLP_BACKGROUND") == "1"
        # the reference's precedence (scene.py:227-235): MLP, then video, then the Gaussian scene
        gs_bound = os.environ.get("DWG_BIND_GS_BACKGROUND") == "1"
        gs = bool(r.use_gs_background) and gs_bound and not r.use_mlp_background and not r.use_video_background
        if (r.use_mlp_background and not mlp) or (r.use_gs_background and not gs_bound):
            raise NotImplementedError("learned / Gaussian backgrounds are outside the bound hot path (scene.py:226-237); "
                                      "DWG_BIND_MLP_BACKGROUND=1 binds the learned MLP background (B23), DWG_BIND_GS_BACKGROUND=1 the "
                                      "Gaussian scene background for playback (B24)")
        background = None
        if mlp:
            # the reference's OWN MLPBackground is built (its initial weights are the reference's draw) and adopted: the scene's
            # background.get_optimizer() -- what init_gaussian_solvers puts under 'background' (trainer.py:594-598) -- is the fused Adan
            from dreamwaltz_g_amd.background import MLPBackground
            background = MLPBackground.from_reference(mod.MLPBackground())
        elif r.use_video_background:
            # the reference's OWN VideoBackground (resolved at call time like its build_scene does: scene.py:229-230) decodes the video,
            # with its motionx temp-file extraction; the adopted device store keeps it alive (its __del__ removes that file)
            from dreamwaltz_g_amd.background import VideoBackground
            background = VideoBackground.from_reference(mod.VideoBackground(r.use_video_background))
        elif gs:
            # the .ply is read by the package's own reader (the reference's load_ply needs plyfile); the parameters go to cfg.device with
            # the scene, frozen
            from dreamwaltz_g_amd.background import GaussianBackground
            background = GaussianBackground.from_ply(r.use_gs_background)
        # exact pair sizing through the 16-byte read-back per frame, like the reference's CUDA extension: the reference's loop body does
        # not know about re-rendering a truncated frame
        return Scene(cfg, avatar, background=background, async_pair_count=False).to(torch.device(cfg.device))
    setattr(build_scene, _PATCHED, True)
    build_scene.__wrapped__ = orig
    mod.build_scene = build_scene


# --------------------------------------------------------------------------------------------------------------------------------------
# B4: guidance
# --------------------------------------------------------------------------------------------------------------------------------------
def plan_dtype_for(ref, dtype=None):
    """Storage type of the HIP plans for a constructed reference guidance object: the explicit argument, else DWG_BIND_DTYPE, else the
    precision the reference itself loaded its pipeline in (core/guidance/basic.py:233 `torch_dtype=self.torch_dtype`): torch.float32 (the
    default of every shipped recipe) -> "f32x", whose results are the fp32 ones (eps 3e-6 vs the fp32 oracle); torch.float16
    (`--guide.dtype fp16`, basic.py:24-27) -> "f16".  The binding never narrows the user's arithmetic on its own: bf16 plans (eps 1.5 % off)
    only through the argument / DWG_BIND_DTYPE=bf16."""
    import torch
    return dtype or os.environ.get("DWG_BIND_DTYPE") or ("f16" if getattr(ref, "torch_dtype", None) is torch.float16 else "f32x")


def bind_guidance(ref, dtype=None, keep_modules=None):
    """Binds `_predict` and `encode_images` of a constructed reference ControlNetScoreDistillation to HIP plans fed from the state_dict()s
    of its loaded diffusers modules (pipe.unet, controlnet, pipe.vae).  Returns `ref` (the same object)."""
    if getattr(ref, _PATCHED, False):
        return ref
    _pkg()
    import torch
    from dreamwaltz_g_amd import guidance as gd, sd15
    dtype = plan_dtype_for(ref, dtype)
    unet, cnet, vae = ref.pipe.unet, ref.controlnet, ref.pipe.vae
    if type(cnet).__name__ == "MultiControlNetModel":
        raise NotImplementedError("MultiControlNetModel (several condition types at once)")
    ucfg, vcfg = sd15.unet_config_from(getattr(unet, "config", None)), sd15.vae_config_from(getattr(vae, "config", None))
    f32 = lambda sd: {k: v.detach().float().cpu() for k, v in sd.items()}       # noqa: E731
    vsd = {k: v for k, v in f32(vae.state_dict()).items() if k.startswith(("encoder.", "quant_conv."))}
    bind_decoder = os.environ.get("DWG_BIND_VAE_DECODER") == "1"
    dec_kw = {}
    if bind_decoder:                                        # B26: the decoder's plans read post_quant_conv.* / decoder.* of the same VAE
        dec_kw = dict(decoder=True, vae_decoder_sd={k: v for k, v in f32(vae.state_dict()).items() if k.startswith(("decoder.", "post_quant_conv."))})
    hip = gd.ControlNetScoreDistillation(ref.device, unet_cfg=ucfg, vae_cfg=vcfg, unet_sd=f32(unet.state_dict()), controlnet_sd=f32(cnet.state_dict()),
                                         vae_sd=vsd, image_hw=int(ref.default_image_size), cfg=ref.cfg, dtype=dtype, **dec_kw)
    if os.environ.get("DWG_BIND_EAGER") != "1":
        stream_ok = torch.cuda.current_stream(ref.device).cuda_stream != 0
        if stream_ok:
            hip.capture_graphs()

    # f32x range safety (round 5): the split-precision plans saturate at +-65504 and thin out below 6.1e-5 where the reference's fp32
    # pipeline (core/guidance/basic.py:233) does neither.  The stored activations of a call are scanned after EVERY one of the first
    # DWG_BIND_RANGE_CHECK_FIRST calls (default 20: a run that saturates does so at its first high-noise timesteps, and must not train
    # 200 steps on clipped values before anything is said) and every DWG_BIND_RANGE_CHECK_EVERY calls after that (default 200; 0: never);
    # a hit is reported ONCE per layer set with the layers' names and the documented way out.  DWG_BIND_RANGE_STRICT=1 raises instead.
    check_every = int(os.environ.get("DWG_BIND_RANGE_CHECK_EVERY", "200"))
    check_first = int(os.environ.get("DWG_BIND_RANGE_CHECK_FIRST", "20")) if check_every > 0 else 0
    strict = os.environ.get("DWG_BIND_RANGE_STRICT") == "1"
    state = {"calls": 0, "warned": set(), "checks": 0}

    def _range_check():
        rep = hip.range_report()
        ref.hip_range_report = rep
        state["checks"] += 1
        ref.hip_range_checks = state["checks"]
        if rep is None or rep["ok"]:
            return
        if strict:
            raise FloatingPointError("dwg_bind: the f32x plans saturated / produced non-finite values at call %d (DWG_BIND_RANGE_STRICT=1); "
                                     "rerun with DWG_BIND_DTYPE=f32" % state["calls"])
        layers = tuple(sorted({"%s:%s" % (n, d["layer"]) for n in ("denoiser", "vae_forward", "vae_backward") for d in rep[n]["worst"]
                               if d["saturated"] or d["nonfinite"]}))
        if layers not in state["warned"]:
            state["warned"].add(layers)
            import warnings
            warnings.warn("dwg_bind: the f32x (split fp16) plans SATURATED at +-65504 or produced non-finite values in %s -- the reference's fp32 "
                          "pipeline would not have; rerun with DWG_BIND_DTYPE=f32 (exact-f32 MFMA plans, ~2.5x slower)" % (", ".join(layers) or "the weights"),
                          RuntimeWarning, stacklevel=3)

    def _predict(self, latents_model_input, text_embeddings, cond_inputs):
        hip.timestep = self.timestep                       # controlnet.py:83-114 reads self.timestep
        out = hip._predict(latents_model_input, text_embeddings, cond_inputs).to(latents_model_input.dtype)
        state["calls"] += 1
        if check_every > 0 and hip.dtype_name == "f32x" and (state["calls"] <= check_first or state["calls"] % check_every == 0):
            _range_check()
        return out

    def encode_images(self, images):
        if not isinstance(images, torch.Tensor):           # PIL inputs (visualisation only): the reference's own path
            return type(self).encode_images(self, images)
        return hip.encode_images(images)                   # normalise (2x-1) + encoder + posterior sample + scaling factor, differentiable

    def decode_latents(self, latents, output_type='pt'):
        if output_type != 'pt' or not isinstance(latents, torch.Tensor) or not latents.is_cuda:      # PIL / numpy outputs: the reference's own path
            return type(self).decode_latents(self, latents, output_type)
        return hip.decode_latents(latents.float())         # vae.py:42-46: 1 / scaling_factor, decode, postprocess 'pt'

    ref._predict = types.MethodType(_predict, ref)
    ref.encode_images = types.MethodType(encode_images, ref)
    if bind_decoder:
        ref.decode_latents = types.MethodType(decode_latents, ref)
    ref.hip = hip
    keep = keep_modules if keep_modules is not None else os.environ.get("DWG_BIND_KEEP_MODULES") == "1"
    if not keep:
        for m in (unet, cnet):                             # their weights now live in the plans
            if hasattr(m, "to"):
                m.to("cpu")
    setattr(ref, _PATCHED, True)
    return ref


def _patch_guidance_module(mod):
    cls = mod.ControlNetScoreDistillation
    if getattr(cls.__init__, _PATCHED, False):
        return
    orig_init = cls.__init__

    def __init__(self, *args, **kwargs):
        orig_init(self, *args, **kwargs)
        if type(self) is cls:                               # not the SDXL subclass family
            bind_guidance(self)
    setattr(__init__, _PATCHED, True)
    __init__.__wrapped__ = orig_init
    cls.__init__ = __init__


# --------------------------------------------------------------------------------------------------------------------------------------
# post-import hooks
# --------------------------------------------------------------------------------------------------------------------------------------
HOOKS = {"core.system.avatar": _patch_avatar_hooks, "core.system.scene": _patch_scene_module,
         "core.guidance.controlnet": _patch_guidance_module, "core.nerf.nerf_model": _patch_nerf_module,
         "core.trainer": _patch_trainer_module, "core.nerf.to_point_cloud": _patch_pointcloud_module}


class _HookLoader(importlib.abc.Loader):
    def __init__(self, inner, hook):
        self.inner, self.hook = inner, hook

    def create_module(self, spec):
        return self.inner.create_module(spec)

    def exec_module(self, module):
        self.inner.exec_module(module)
        self.hook(module)

    def __getattr__(self, name):
        return getattr(self.inner, name)


class _HookFinder(importlib.abc.MetaPathFinder):
    def __init__(self):
        self.busy = set()

    def find_spec(self, fullname, path, target=None):
        if fullname not in HOOKS or fullname in self.busy:
            return None
        self.busy.add(fullname)
        try:
            spec = None
            for finder in sys.meta_path:
                if finder is self or not hasattr(finder, "find_spec"):
                    continue
                spec = finder.find_spec(fullname, path, target)
                if spec is not None:
                    break
        finally:
            self.busy.discard(fullname)
        if spec is None or spec.loader is None:
            return None
        spec.loader = _HookLoader(spec.loader, HOOKS[fullname])
        return spec


def install():
    """Idempotent.  Modules of HOOKS that are already imported are patched right away, the others right after their import."""
    for d in (_HERE, _ROOT):
        if d not in sys.path:
            sys.path.insert(0, d)
    if not any(isinstance(f, _HookFinder) for f in sys.meta_path):
        sys.meta_path.insert(0, _HookFinder())
    for name, hook in HOOKS.items():
        if name in sys.modules:
            hook(sys.modules[name])
    return True


def uninstall():
    sys.meta_path[:] = [f for f in sys.meta_path if not isinstance(f, _HookFinder)]
    for name in HOOKS:
        mod = sys.modules.get(name)
        if mod is None:
            continue
        for attr in ("build_gaussian_avatar", "build_scene", "build_NeRFNetwork", "find_nearest_triangles", "knn_points", "export_point_cloud",
                     "remove_points_inside_bboxes"):
            f = getattr(mod, attr, None)
            if f is not None and getattr(f, _PATCHED, False):
                setattr(mod, attr, f.__wrapped__)
        cls = getattr(mod, "LBSUtils", None)
        f = getattr(cls.__dict__.get("initialize_lbs_weights"), "__func__", None) if cls is not None else None
        if f is not None and getattr(f, _PATCHED, False):
            cls.initialize_lbs_weights = staticmethod(f.__wrapped__)
        cls = getattr(mod, "ControlNetScoreDistillation", None)
        if cls is not None and getattr(cls.__init__, _PATCHED, False):
            cls.__init__ = cls.__init__.__wrapped__
        cls = getattr(mod, "Trainer", None)
        if cls is not None and getattr(cls.__dict__.get("calc_sigma_loss"), _PATCHED, False):
            cls.calc_sigma_loss = cls.calc_sigma_loss.__wrapped__
        for attr in ("pretrain_forward", "init_losses", "pretrain_nerf2gs_forward"):
            if cls is not None and getattr(cls.__dict__.get(attr), _PATCHED, False):
                setattr(cls, attr, getattr(cls, attr).__wrapped__)
