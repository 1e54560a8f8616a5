"""Mirror of Scene (/root/reference/core/system/scene.py:15-168; SURVEY.md section 8a row R7, boundary B5): avatar_forward
(optional per-avatar scale / translation), multi-avatar merge, the debug overrides, GaussianRenderer.render, and the background
compositing `image + bg (1 - alpha)` for bg_mode in {black, white, gray}, for a video background (background.VideoBackground:
the frames on the device, one launch per frame chain) and for the learned MLP background (boundary B23, background.MLPBackground:
directions, the fused encoding + network + sigmoid, and the composite -- three launches forward; gradients to alpha and to the
background's weights).  Precedence as the reference's (scene.py:153-166): a pure-colour bg_mode, then video, then MLP.  The Gaussian
(.ply) scene background (scene.py:123-132, boundary B24) is a background.GaussianBackground: its activated block is merged with the avatars'
Gaussians in one launch per frame, whatever bg_mode says, before the debug overrides and the rasterizer -- playback and evaluation only,
its parameters are frozen.  With `cull_scene` (boundary B25, off by default) forward_frames merges only the scene Gaussians that may reach
the image under the call's cameras (background.GaussianBackground.culled): the same frames bit for bit.  Every object that is not one of the package's own three background classes is rejected."""
from typing import Iterable, Optional

import contextlib

import torch
import torch.nn as nn

from .avatar import DreamWaltzG, GaussianOutput, merge_gaussians
from . import optim as _optim
from .background import CULL_MAX_CAMERAS, GaussianBackground, MLPBackground, VideoBackground, mlp_composite, scene_merge, video_composite
from .renderer import GaussianRenderer


class PureColorBackground:
    """core/system/background.py:14-57."""
    COLOR_VALUE_MAPPING = {'black': 0.0, 'white': 1.0, 'gray': 0.5}

    def __contains__(self, bg_mode):
        return bg_mode in ('black', 'white', 'gray')

    @staticmethod
    def get_background_like(color: str, image: torch.Tensor) -> torch.Tensor:
        return torch.full_like(image, PureColorBackground.COLOR_VALUE_MAPPING[color])


def downsample_gaussians(gaussians: GaussianOutput, n: int) -> GaussianOutput:
    """gaussian_utils.py downsample_gaussians: a random subset of n Gaussians (debug override use_fixed_n_gaussians)."""
    total = gaussians.positions.shape[0]
    if n >= total:
        return gaussians
    idx = torch.randperm(total, device=gaussians.positions.device)[:n]
    return GaussianOutput(**{k: (gaussians[k][idx] if torch.is_tensor(gaussians[k]) else None) for k in gaussians.keys()})


class Scene(nn.Module):
    def __init__(self, cfg, avatar, background=None, async_pair_count=False, cull_scene=False) -> None:
        """`cull_scene`: forward_frames merges, per call, only the Gaussians of a Gaussian scene background that may reach the image under
        the call's cameras (background.GaussianBackground.culled, boundary B25) -- the same frames bit for bit, fewer rows through the merge
        and the rasterizer.  Off by default; forward_frames(cull_scene=) overrides it per call."""
        super().__init__()
        if (background is not None and not isinstance(background, VideoBackground) and type(background) is not MLPBackground
                and type(background) is not GaussianBackground):
            raise NotImplementedError("Gaussian backgrounds are outside the SDS hot path (scene.py:123-132); a video background is a "
                                      "background.VideoBackground, a learned one a background.MLPBackground and a Gaussian scene for "
                                      "playback a background.GaussianBackground, got %s.%s"
                                      % (type(background).__module__, type(background).__name__))
        self.device = torch.device(cfg.device)
        if isinstance(avatar, DreamWaltzG):
            self.avatar, self.avatars = avatar, None
        else:
            self.avatars = nn.ModuleList(avatar)
            self.avatar = self.avatars[0]
        self.background = background
        self.cull_scene = bool(cull_scene)
        if self.cull_scene and type(background) is not GaussianBackground:
            raise ValueError("cull_scene=True culls a Gaussian scene background (background.GaussianBackground): this scene has none")
        self.pure_colors = PureColorBackground()
        self.renderer = GaussianRenderer(sh_levels=cfg.render.sh_levels, bg_color=cfg.render.bg_color, async_pair_count=async_pair_count)
        r = cfg.render
        self.use_zero_scales = r.use_zero_scales
        self.use_constant_colors = r.use_constant_colors is not None
        self.constant_colors = None if r.use_constant_colors is None else torch.tensor([r.use_constant_colors], device=self.device)
        self.use_constant_opacities = r.use_constant_opacities is not None
        self.constant_opacities = None if r.use_constant_opacities is None else torch.tensor([r.use_constant_opacities], device=self.device)
        self.use_fixed_n_gaussians = r.use_fixed_n_gaussians is not None
        self.fixed_n_gaussians = None if r.use_fixed_n_gaussians is None else int(r.use_fixed_n_gaussians)
        self.avatar_transl = torch.tensor(eval(r.avatar_transl), device=self.device) if r.avatar_transl is not None else None
        self.avatar_scale = torch.tensor(eval(r.avatar_scale), device=self.device) if r.avatar_scale is not None else None

    def avatar_forward(self, smpl_observed_inputs: Optional[dict] = None, avatar=None, avatar_index: Optional[int] = None) -> GaussianOutput:
        if avatar is None:
            avatar = self.avatar
        gaussians = avatar.forward() if smpl_observed_inputs is None else avatar.animate(smpl_observed_inputs=smpl_observed_inputs)
        if self.avatar_scale is not None:
            s = self.avatar_scale
            if s.ndim == 1:
                s = s[avatar_index]
            gaussians.positions = gaussians.positions * s.unsqueeze(0)
            gaussians.scales = gaussians.scales * s.unsqueeze(0)
        if self.avatar_transl is not None:
            t = self.avatar_transl
            if t.ndim == 2:
                t = t[avatar_index]
            gaussians.positions = gaussians.positions + t.unsqueeze(0)
        return gaussians

    def _avatar_parts(self, smpl_observed_inputs) -> list:
        """The avatars' outputs of one frame, unmerged: [avatar_forward(pose)] or, with several avatars, avatar i animated with slice i of
        the [A, ...] inputs (scene.py:107-121)."""
        if self.avatars is None:
            return [self.avatar_forward(smpl_observed_inputs=smpl_observed_inputs)]
        parts = []
        batch_size = smpl_observed_inputs['body_pose'].size(0)
        assert batch_size <= len(self.avatars), f'Assert num_smplx_inputs: {batch_size} <= num_avatars: {len(self.avatars)}'
        for i, avatar in enumerate(self.avatars):
            parts.append(self.avatar_forward({k: v[i:i + 1, ...] for k, v in smpl_observed_inputs.items()}, avatar=avatar, avatar_index=i))
        return parts

    def _avatars_forward(self, smpl_observed_inputs: dict) -> GaussianOutput:
        """scene.py:107-121: avatar i animated with slice i of the [A, ...] inputs (and its scale / translation), the outputs merged."""
        return merge_gaussians(*self._avatar_parts(smpl_observed_inputs))

    @property
    def gaussian_background(self):
        """The static Gaussian scene behind the avatars (background.GaussianBackground), or None."""
        return self.background if type(self.background) is GaussianBackground else None

    def _culled_background(self, cameras):
        """The scene background culled for `cameras` (one camera dict or a list: the union), or the refusal of what culling cannot serve."""
        if self.gaussian_background is None:
            raise ValueError("cull_scene=True culls a Gaussian scene background (background.GaussianBackground): this scene has none")
        if self.use_fixed_n_gaussians:
            raise ValueError("cull_scene with use_fixed_n_gaussians: the random subset would be drawn from the culled set, not from the "
                             "merged set the unculled frame draws it from -- switch one of them off")
        if self.renderer.SCALE_MODIFIER != 1.0:                # the bound of csrc/cull_math.h is stated for the scale modifier the renderer fixes
            raise ValueError("cull_scene needs the renderer's scale_modifier to be 1, got %r" % (self.renderer.SCALE_MODIFIER,))
        many = isinstance(cameras, (list, tuple))
        if many and len(cameras) > CULL_MAX_CAMERAS:
            raise ValueError("cull_scene takes the union over at most %d per-frame cameras, got %d: split the forward_frames call"
                             % (CULL_MAX_CAMERAS, len(cameras)))
        first = cameras[0] if many else cameras
        return self.background.culled(cameras, first['image_height'], first['image_width'])

    def _frames_with_scene(self, data, poses, cull_scene=False):
        """forward_frames with a Gaussian scene: per frame the avatars' rows and the scene's rows go straight into the stacked [F, N, .]
        buffers the frames chain reads (ONE merge launch per frame, no torch.cat and no torch.stack of the scene), then the debug overrides
        on the merged set (scene.py:134-145).  `cull_scene`: the scene's rows are those of the block culled for the call's cameras (their
        union; cached per cameras).  -> the kwargs of renderer.render_frames."""
        bg = self._culled_background(data) if cull_scene else self.background
        datas = list(data) if isinstance(data, (list, tuple)) else None
        bufs, total, F = None, None, len(poses)
        if datas is not None and len(datas) not in (1, F):
            raise ValueError("%d camera dicts for %d frames" % (len(datas), F))
        for f, pose in enumerate(poses):
            parts = self._avatar_parts(pose)
            n = sum(int(g.positions.shape[0]) for g in parts) + bg.n_points
            if bufs is None:
                total = n
                dev = parts[0].positions.device
                bufs = tuple(torch.empty((F, n, w), dtype=torch.float32, device=dev) for w in (3, 1, 3, 3, 4))
            elif n != total:
                raise ValueError("the frames of one forward_frames call share one Gaussian count: frame %d has %d, frame 0 %d" % (f, n, total))
            d = data if datas is None else datas[f if len(datas) > 1 else 0]
            scene_merge(parts, bg, d['c2w'][:, :3, 3], out=tuple(b[f] for b in bufs))
        positions, opacities, colors, scales, quaternions = bufs
        # the stacked buffers are this call's own: the overrides change them in place (the same values as forward()'s `scales * 0.1` and
        # expanded constants, without a second [F, N, .] tensor)
        if self.use_zero_scales:
            scales.mul_(0.1)
        if self.use_constant_colors:
            colors.copy_(self.constant_colors.to(colors.dtype).expand(F, total, -1))
        if self.use_constant_opacities:
            opacities.copy_(self.constant_opacities.to(opacities.dtype).expand(F, total, -1))
        if self.use_fixed_n_gaussians:                         # a random subset per frame, as forward() draws it: frames of their own
            frames = [downsample_gaussians(GaussianOutput(positions=positions[f], opacities=opacities[f], colors=colors[f], scales=scales[f],
                                                          quaternions=quaternions[f]), self.fixed_n_gaussians) for f in range(F)]
            return {'frames': frames}
        return {'frames': None, 'stacked': {'positions': positions, 'opacities': opacities, 'colors': colors, 'scales': scales,
                                            'quaternions': quaternions}}

    def _video_indices(self, data, frame_indices):
        if frame_indices is not None:
            return frame_indices
        if isinstance(data, (list, tuple)):
            idx = [d.get('frame_index') for d in data]
            if any(i is None for i in idx):
                idx = None
            elif any(isinstance(i, torch.Tensor) and i.is_cuda for i in idx):
                idx = torch.cat([i.reshape(-1).to(torch.int32) for i in idx])
        else:
            idx = data.get('frame_index')
        if idx is None:
            raise ValueError("a video background needs one frame index per frame: frame_indices= or data['frame_index']")
        return idx

    @property
    def mlp_background(self):
        """The learned background, or None."""
        return self.background if type(self.background) is MLPBackground else None

    def _mlp_frames_background(self, data, F):
        """image_bg of F playback frames from ONE directions launch and ONE network launch: [F, H, W, 3] for a list of F camera dicts,
        [1, H, W, 3] for one shared camera (computed once)."""
        if isinstance(data, (list, tuple)):
            if len(data) != F:
                raise ValueError("%d camera dicts for %d frames" % (len(data), F))
            H, W = int(data[0]['image_height']), int(data[0]['image_width'])
            if any((int(d['image_height']), int(d['image_width'])) != (H, W) for d in data):
                raise ValueError("the frames of one forward_frames call share one image size")
            data = {'c2w': torch.cat([d['c2w'][:1] for d in data]), 'intrinsics': torch.cat([d['intrinsics'][:1] for d in data]),
                    'image_height': H, 'image_width': W}
        else:
            data = {'c2w': data['c2w'][:1], 'intrinsics': data['intrinsics'][:1], 'image_height': data['image_height'],
                    'image_width': data['image_width']}
        with torch.no_grad():
            return self.background(data)

    def forward_frames(self, data: dict, poses, bg_mode: Optional[str] = None, frozen_avatar: bool = False, frame_indices=None,
                       cull_scene: Optional[bool] = None) -> dict:
        """Playback of F pose frames under one camera (`data`: the loader's dict) or each under its own (`data`: a list of F dicts, as the
        reference's evaluation loader yields them): `animate` per pose, then ONE rasterizer launch chain for all of them
        (renderer.render_frames).  Frame f equals `forward(data, poses[f], use_densifier=False, bg_mode=bg_mode)` bit for bit -- the
        reference's evaluation loop renders such sequences one pose at a time under inference mode (trainer.py:1019-1150).  No gradients.
        With several avatars (`Scene(cfg, [avatar, ...])`) `poses[f]` carries the [A, ...] batch `forward` slices: avatar i is animated
        with slice i and its `avatar_transl` / `avatar_scale`, and the A outputs of a frame are merged before the one launch chain.
        `frozen_avatar`: the avatar's parameters do not change between the frames (a trained avatar playing a motion): the
        pose-independent part of `animate` -- canonical positions, grid encoding, colour / opacity network -- is computed once and kept until
        a parameter changes (avatar.DreamWaltzG.frozen_playback; same bits, 0.3 ms less per 300 k-Gaussian frame).  A video background
        takes one frame index per frame (`frame_indices`: ints or an int32 CUDA tensor; else each data dict's 'frame_index', or a
        single dict's list / tensor of F) and composites all F frames in one launch after the rasterizer chain.  `cull_scene` (default:
        the scene's own switch): merge only the Gaussians of a Gaussian scene background that may reach the image under this call's
        cameras (their union: at most 64 per-frame cameras a call) -- the same frames bit for bit; refused together with
        use_fixed_n_gaussians, without a Gaussian scene, and under a camera dict that carries 'tanfov_dev'.
        -> {'image' | 'image_fg' | 'image_bg' | 'depth' | 'alpha': [F, H, W, C]}."""
        frames = []
        cull = self.cull_scene if cull_scene is None else bool(cull_scene)
        if cull and self.gaussian_background is None:
            raise ValueError("cull_scene=True culls a Gaussian scene background (background.GaussianBackground): this scene has none")
        avatars = [self.avatar] if self.avatars is None else list(self.avatars)
        for avatar in avatars:
            avatar.frozen_playback = bool(frozen_avatar)
        scene_frames = None
        try:
            if self.gaussian_background is not None:
                with torch.no_grad():                           # playback: the rows are written into preallocated buffers
                    scene_frames = self._frames_with_scene(data, list(poses), cull_scene=cull)
                poses = []
            for pose in poses:
                if self.avatars is None:
                    g = self.avatar_forward(smpl_observed_inputs=pose)
                else:
                    g = self._avatars_forward(pose)
                if self.use_zero_scales:
                    g.scales = g.scales * 0.1
                if self.use_constant_colors:
                    g.colors = self.constant_colors.expand(g.colors.size(0), -1)
                if self.use_constant_opacities:
                    g.opacities = self.constant_opacities.expand(g.opacities.size(0), -1)
                if self.use_fixed_n_gaussians:
                    g = downsample_gaussians(g, self.fixed_n_gaussians)
                frames.append(g)
        finally:
            for avatar in avatars:
                avatar.frozen_playback = False
        outputs = self.renderer.render_frames(data=data, frames=frames) if scene_frames is None else self.renderer.render_frames(data=data, **scene_frames)
        if bg_mode in self.pure_colors:
            outputs['image_bg'] = self.pure_colors.get_background_like(bg_mode, outputs['image'])
            outputs['image_fg'] = outputs['image']
            outputs['image'] = outputs['image'] + outputs['image_bg'] * (1 - outputs['alpha'])
        elif isinstance(self.background, VideoBackground):
            image, outputs['image_bg'] = video_composite(outputs['image'], outputs['alpha'], self.background,
                                                         self._video_indices(data, frame_indices))
            outputs['image_fg'] = outputs['image']
            outputs['image'] = image
        elif self.mlp_background is not None:
            with torch.no_grad():
                bg = self._mlp_frames_background(data, len(frames))
                outputs['image_fg'] = outputs['image']
                outputs['image'] = mlp_composite(outputs['image'], outputs['alpha'], bg)
                outputs['image_bg'] = bg if bg.shape[0] == len(frames) else bg.expand(len(frames), -1, -1, -1)
        else:
            outputs['image_fg'] = outputs['image']
        return outputs

    def forward_views(self, datas, poses, bg_mode: Optional[str] = None, streams=None) -> list:
        """The V views of a batched multi-view training step (trainer.train_forward_views): `animate` per view (`poses[v]`: that view's
        smpl inputs, or None for the canonical pose) -- each on its own stream when `streams` is given, they are independent chains of
        small launches -- then ONE differentiable rasterizer launch chain for all of them (renderer.render_frames: forward AND backward on
        (work, V) grids).  View v of the result equals `forward(datas[v], poses[v], use_densifier=False, bg_mode=bg_mode)` bit for bit,
        and so do the gradients it sends back.  Single avatar.  -> a list of V output dicts ([1, H, W, C] tensors)."""
        if self.gaussian_background is not None:
            raise NotImplementedError("forward_views with a GaussianBackground: the Gaussian scene is for playback and evaluation "
                                      "(Scene.forward / forward_frames); the batched multi-view training render does not merge it")
        if self.avatars is not None:
            raise NotImplementedError("forward_views renders one avatar per view")
        if self.mlp_background is not None:
            raise NotImplementedError("forward_views with an MLP background: a step with the learned background is single view "
                                      "(Scene.forward); the batched multi-view render does not composite it")
        main = torch.cuda.current_stream(self.avatar.device) if streams else None
        frames = []
        for v, pose in enumerate(poses):
            if streams:
                streams[v].wait_stream(main)
            with (torch.cuda.stream(streams[v]) if streams else contextlib.nullcontext()):
                g = self.avatar_forward(smpl_observed_inputs=pose)
                if self.use_zero_scales:
                    g.scales = g.scales * 0.1
                if self.use_constant_colors:
                    g.colors = self.constant_colors.expand(g.colors.size(0), -1)
                if self.use_constant_opacities:
                    g.opacities = self.constant_opacities.expand(g.opacities.size(0), -1)
                if self.use_fixed_n_gaussians:
                    g = downsample_gaussians(g, self.fixed_n_gaussians)
            if streams:
                for t in (g.positions, g.opacities, g.colors, g.sh_features, g.scales, g.quaternions):
                    if t is not None:
                        t.record_stream(main)
            frames.append(g)
        if streams:
            for side in streams[:len(frames)]:
                main.wait_stream(side)
        out = self.renderer.render_frames(data=list(datas), frames=frames)
        video = bg_mode not in self.pure_colors and isinstance(self.background, VideoBackground)
        if video:                                          # all V views in one launch; view v's pixels are those of forward()
            composite, bg = video_composite(out['image'], out['alpha'], self.background, self._video_indices(list(datas), None))
        views = []
        for v in range(len(frames)):
            o = {k: t[v:v + 1] for k, t in out.items()}
            if video:
                o['image_bg'] = bg[v]
                o['image_fg'] = o['image']
                o['image'] = composite[v:v + 1]
            elif bg_mode in self.pure_colors:
                o['image_bg'] = self.pure_colors.get_background_like(bg_mode, o['image'])
                o['image_fg'] = o['image']
                o['image'] = o['image'] + o['image_bg'] * (1 - o['alpha'])
            else:
                o['image_fg'] = o['image']
            views.append(o)
        return views

    def forward(self, data: dict, smpl_observed_inputs: Optional[dict] = None, use_densifier: bool = True, bg_mode: Optional[str] = None,
                **kwargs):
        if self.gaussian_background is not None:
            # scene.py:123-132, whatever bg_mode says: the avatars' rows, then the scene's, in one launch (no torch.cat per attribute)
            gaussians = scene_merge(self._avatar_parts(smpl_observed_inputs), self.background, data['c2w'][:, :3, 3])
        elif self.avatars is None:
            gaussians = self.avatar_forward(smpl_observed_inputs=smpl_observed_inputs)
        else:
            gaussians = self._avatars_forward(smpl_observed_inputs)
        if self.use_zero_scales:
            gaussians.scales = gaussians.scales * 0.1
        if self.use_constant_colors:
            gaussians.colors = self.constant_colors.expand(gaussians.colors.size(0), -1)
        if self.use_constant_opacities:
            gaussians.opacities = self.constant_opacities.expand(gaussians.opacities.size(0), -1)
        if self.use_fixed_n_gaussians:
            gaussians = downsample_gaussians(gaussians, self.fixed_n_gaussians)
        outputs = self.renderer.render(data=data, gaussians=gaussians, return_2d_radii=use_densifier)
        if bg_mode in self.pure_colors:
            outputs['image_bg'] = self.pure_colors.get_background_like(bg_mode, outputs['image'])
            outputs['image_fg'] = outputs['image']
            outputs['image'] = outputs['image'] + outputs['image_bg'] * (1 - outputs['alpha'])
        elif isinstance(self.background, VideoBackground):
            # scene.py:157-160: image_bg is the [H, W, 3] frame of data['frame_index'] (an int, or an int32 CUDA tensor of one index)
            image, image_bg = video_composite(outputs['image'], outputs['alpha'], self.background, data['frame_index'])
            outputs['image_bg'] = image_bg[0]
            outputs['image_fg'] = outputs['image']
            outputs['image'] = image
        elif self.mlp_background is not None:
            # scene.py:161-164: image_bg [B, H, W, 3] from the network; the composite sends gradients to alpha and to image_bg
            outputs['image_bg'] = self.background(data)
            outputs['image_fg'] = outputs['image']
            outputs['image'] = mlp_composite(outputs['image'], outputs['alpha'], outputs['image_bg'])
        else:
            outputs['image_fg'] = outputs['image']
        return outputs

    def densify(self, densifiers: dict, render_outputs: dict, spatial_scale: float, train_step: int):
        """scene.py:170-186: the free Gaussians' share of the screen-space gradient / radii goes to the avatar's densifier."""
        if hasattr(self.avatar, 'densification_mask'):
            mask = self.avatar.densification_mask.to(render_outputs['radii'].device)
            viewspace_points = render_outputs['viewspace_points'][mask]
            viewspace_points.grad = render_outputs['viewspace_points'].grad[mask]
            radii = render_outputs['radii'][mask]
        else:
            viewspace_points = render_outputs['viewspace_points']
            radii = render_outputs['radii']
        densifiers['avatar'](viewspace_points=viewspace_points, radii=radii, spatial_extent=spatial_scale, train_step=train_step)

    # -- checkpoints (scene.py:170-208) ---------------------------------------------------------------------------------------
    @staticmethod
    def organize_state_dict(state_dict):
        by_module = {}
        for k, v in state_dict.items():
            module_name = k.split('.')[0]
            by_module.setdefault(module_name, {})[k.replace(f'{module_name}.', '', 1)] = v
        return by_module

    def state_dict(self, *args, **kwargs):
        """Scene.state_dict() of the reference: the avatar under `avatar.` (and `avatars.<i>.` for a multi-avatar scene)."""
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True):
        """scene.py:196-200: resize the per-Gaussian parameters to the checkpoint's count (reset_by_state_dict), then a plain
        load; derived caches / topology of the native path are rebuilt afterwards."""
        by_module = self.organize_state_dict(state_dict)
        if 'avatar' in by_module:
            self.avatar.reset_by_state_dict(by_module['avatar'])
        if 'background' in by_module and self.gaussian_background is not None:
            self.background.reset_by_state_dict(by_module['background'])
        own = set(super().state_dict().keys())
        filtered = {k: v for k, v in state_dict.items() if k in own}
        res = super().load_state_dict(filtered, strict=False)
        if 'avatar.nerf_bound' in state_dict:
            self.avatar._nerf_bound_host = float(state_dict['avatar.nerf_bound'])
        for a in ([self.avatar] if self.avatars is None else list(self.avatars)):
            a.invalidate_caches()
        if any(k.startswith('background.') for k in filtered):
            _optim.PARAM_EPOCH[0] += 1          # the background's weights were written behind the parameter-derived caches' back
        unexpected = [k for k in state_dict.keys() if k not in own]
        if strict and (res.missing_keys or unexpected):
            raise RuntimeError("Scene.load_state_dict: missing %s unexpected %s" % (res.missing_keys, unexpected))
        return res
