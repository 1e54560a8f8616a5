"""The loop body of the reference's Trainer.train() for the NeRF stage (stage I), on the HIP path (boundary B20):

  render(data, bg_mode)      core/trainer.py:680-709                     model.render: 'albedo', or 'normal' under the normal-adapted guidance
  train_forward(data)        trainer.py:933-1017   render -> the planar image -> view-dependent text embedding -> diffusion(**sd_kwargs)
                                                   -> sigma guidance (sigma_guidance.calc_sigma_loss) -> the fused sparsity loss -> total
  train_step(data)           trainer.py:840-896    update_extra_state every update_extra_interval steps, BEFORE the step counter moves;
                                                   forward; zero_grad; backward; the fused Adam step

Method and dictionary-key names are the reference's.  `diffusion` is any callable with the guidance's call signature that returns a
dict with 'diffusion_loss'.  The model is what nerf_model.build_nerf_network(cfg.nerf) returns -- NeRFNetwork, or BackgroundNeRFNetwork
for the learned 'nerf' background (boundary B22: bg_net steps in its own group of the same flat Adam) -- or anything with its surface;
the optimizers are its get_optimizer's flat dict.  Single view, single GPU, as the reference's stage-I loop.

cfg.optim.fp16 (every published stage-I recipe; boundary B21): update_extra_state and the forward run under fp16 autocast, the loss is
scaled by grad_scaler.FlatGradScaler, every optimizer is stepped through it and the scale is updated, all without a host read
(trainer.py:840-896 with torch.cuda.amp.GradScaler).  Without it the step is the fp32 one and `scaler` stays None.
"""
import os
from random import random
from typing import Any, Dict, Optional

import torch

from . import grad_scaler
from . import nerf_model
from . import nerf_view
from . import sigma_guidance
from .text import TextAugmentation


class NeRFSDSTrainer:
    def __init__(self, cfg, model, diffusion, optimizers, text_embeds_dict: Optional[dict] = None, use_controlnet: bool = True,
                 smpl_model=None, max_step: Optional[int] = None):
        if getattr(cfg, "stage", 'nerf') != 'nerf':
            raise RuntimeError("NeRFSDSTrainer is the stage-I ('nerf') trainer, got stage %r (stage II: trainer.SDSTrainer)" % (cfg.stage,))
        nerf_model.check_optimizer_config(cfg.nerf)
        self.cfg, self.model, self.diffusion, self.optimizers = cfg, model, diffusion, optimizers
        self.smpl_model = smpl_model
        self.text_embeds_dict = text_embeds_dict if text_embeds_dict is not None else {}
        self.view_prompt = TextAugmentation(cfg.guide.text, cfg.prompt) if cfg.prompt.text_augmentation else None
        self.use_controlnet = use_controlnet
        self.train_step_index = 0                   # the reference's self.train_step (the name is the loop body's here, as in SDSTrainer)
        self.max_step = cfg.optim.iters if max_step is None else max_step
        self.scaler = None                          # GradScaler(enabled=False) in the fp32 recipes: pass-through
        if getattr(cfg.optim, "fp16", False):
            self.scaler = grad_scaler.FlatGradScaler(device=model.sigma_scale.device)        # GradScaler's defaults (trainer.py:372)
        self.schedulers = {}
        self.losses = {'sparsity': nerf_view.SparsityLoss(cfg.nerf)}
        self.time_to_snapshot = False               # logging is the caller's: calc_sigma_loss reads it (its statistics are host reads)
        self.past_checkpoints = []
        self._unit = None

    # -- checkpoints: as trainer.SDSTrainer writes them ----------------------------------------------------------------------------------
    def save_checkpoint(self, ckpt_dir, full: bool = False, max_keep_ckpts: int = 2):
        """File name step_{train_step:06d}.pth, rolling window of `max_keep_ckpts` files; `full` adds the optimizer states (step counts,
        learning rates and the flat Adam moments) and the render state a resumed step needs (local_step, the occupancy counters)."""
        os.makedirs(ckpt_dir, exist_ok=True)
        state = {'train_step': self.train_step_index, 'checkpoints': self.past_checkpoints}
        if full:
            state['optimizers'] = [optimizer.state_dict() for optimizer in self.optimizers.values()]
            state['scaler'] = self.scaler.state_dict() if self.scaler is not None else {}
            state['render_state'] = {k: getattr(self.model, k) for k in ('local_step', 'mean_count', 'iter_density', 'mean_density')
                                     if hasattr(self.model, k)}
        state['model'] = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        file_path = f"step_{self.train_step_index:06d}.pth"
        if len(self.past_checkpoints) == 0 or file_path != self.past_checkpoints[-1]:
            self.past_checkpoints.append(file_path)
        if len(self.past_checkpoints) > max_keep_ckpts:
            old = os.path.join(ckpt_dir, self.past_checkpoints.pop(0))
            if os.path.exists(old):
                os.unlink(old)
        torch.save(state, os.path.join(ckpt_dir, file_path))
        return os.path.join(ckpt_dir, file_path)

    def load_checkpoint(self, checkpoint, model_only: bool = False, resume: bool = True):
        """The parameters live in the optimizers' flat buffer: load_state_dict copies into it in place."""
        from . import optim as _optim
        d = torch.load(checkpoint, map_location=self.model.sigma_scale.device, weights_only=False)
        if 'model' not in d:
            self.model.load_state_dict(d)
            _optim.PARAM_EPOCH[0] += 1
            return
        self.model.load_state_dict(d['model'], strict=False)
        _optim.PARAM_EPOCH[0] += 1
        self.past_checkpoints = d['checkpoints']
        if resume:
            self.train_step_index = d['train_step']
        if model_only:
            return
        for k, v in d.get('render_state', {}).items():
            setattr(self.model, k, v)
        if self.optimizers is not None and 'optimizers' in d:
            for optimizer, sd in zip(self.optimizers.values(), d['optimizers']):
                optimizer.load_state_dict(sd)
        if self.scaler is not None and d.get('scaler'):
            self.scaler.load_state_dict(d['scaler'])

    # -- the step --------------------------------------------------------------------------------------------------------------------
    def render(self, data, bg_mode=None, **kwargs):
        """trainer.py:680-689.  In training the fused sparsity loss rides on the render's compose (kwargs: render_view's, e.g. noises)."""
        if self.model.training:
            sp = self.losses['sparsity']
            if sp.available:
                kwargs['sparsity'] = sp.terms(current_step=self.train_step_index, max_iteration=self.max_step)
            shading = 'albedo' if getattr(self.cfg.guide, "diffusion", "sd15") != 'normal-adapted' else 'normal'
            return self.model.render(data=data, shading=shading, bg_mode=bg_mode, **kwargs)
        render_outputs = self.model.render(data=data, shading='albedo', bg_mode=bg_mode)
        render_outputs['normal'] = self.model.render(data=data, shading='normal', bg_mode=bg_mode)['image']
        return render_outputs

    def calc_sigma_loss(self, data, render_outputs, sd_inputs, selected_parts, wo_wrist: bool = True, **kwargs):
        return sigma_guidance.calc_sigma_loss(self, data, render_outputs, sd_inputs, selected_parts, wo_wrist=wo_wrist, **kwargs)

    def _select_text(self, data):
        """The reference's prompt selection (trainer.py:939-949): -> (embedding, prompt string).  With text_augmentation the dict must
        hold 'viewed', without it 'pos': a missing entry is a KeyError, as in the reference."""
        if self.cfg.prompt.text_augmentation:
            view_index = self.view_prompt(azim=data['azimuth'], elev=data['elevation']).item()
            return self.text_embeds_dict['viewed'][view_index], self.view_prompt.texts[view_index]
        return self.text_embeds_dict['pos'], self.cfg.guide.text

    def train_forward(self, data: Dict[str, Any], render_kwargs: Optional[dict] = None, **forced):
        """trainer.py:933-1017.  `forced` (timestep=, noise=, ...) goes to the guidance; render_kwargs to the render (noises=)."""
        cfg = self.cfg
        # Render Images: image_nchw IS render_outputs['image'].permute(0, 3, 1, 2).contiguous()
        render_outputs = self.render(data=data, **(render_kwargs or {}))
        sd_inputs = render_outputs['image_nchw']

        # Text Embeddings
        self.text_embeds_dict['text'], text = self._select_text(data)

        sd_kwargs = {'inputs': sd_inputs, 'text_embeds_dict': self.text_embeds_dict, 'train_step': self.train_step_index,
                     'max_iteration': self.max_step, 'grad_viz': bool(getattr(cfg.guide, "grad_viz", False)) and self.time_to_snapshot,
                     'scaler': self.scaler}
        if getattr(cfg.guide, "grad_rgb_clip_mask_guidance", False):
            sd_kwargs['mask_inputs'] = render_outputs['weights_sum'].permute(0, 3, 1, 2).contiguous()
        if self.use_controlnet:
            sd_kwargs['cond_inputs'] = data['cond_images']
        sd_kwargs.update(forced)

        # Diffusion Loss
        sd_outputs = self.diffusion(**sd_kwargs)
        diffusion_loss = sd_outputs['diffusion_loss'] * cfg.guide.lambda_guidance

        # Regularization Loss
        regularizations = {}

        # Regularization - Sigma Loss
        sigma_select_parts = None
        if getattr(cfg, "use_sigma_guidance", False):
            if random() <= cfg.sigma_prob:
                sigma_select_parts = cfg.predefined_body_parts.split(',')
        elif ((getattr(cfg, "use_sigma_hand_guidance", False) and 'hand' in data['body_part']) or
              (getattr(cfg, "use_sigma_face_guidance", False) and 'face' == data['body_part'])):
            sigma_select_parts = data['body_part']
        if sigma_select_parts is not None:
            regularizations.update(self.calc_sigma_loss(data, render_outputs, sd_inputs, selected_parts=sigma_select_parts))

        # Regularization - Sparsity Loss (computed by the render's compose launch)
        if self.losses['sparsity'].available:
            regularizations['sparsity_loss'] = render_outputs['sparsity_loss']

        render_outputs['regularizations'] = regularizations

        # Total Loss
        total_loss = 0.0
        total_loss += diffusion_loss
        for k in regularizations.keys():
            if k.endswith('_loss'):
                total_loss += regularizations[k]

        return total_loss, render_outputs, sd_outputs, text

    def _backward(self, loss):
        """loss.backward() with the constant seed gradient 1 kept per (device, shape)."""
        if loss.numel() != 1 or loss.dtype != torch.float32:
            return loss.backward()
        key = (loss.device, tuple(loss.shape))
        if self._unit is None or self._unit[0] != key:
            self._unit = (key, torch.ones(loss.shape, device=loss.device))
        loss.backward(gradient=self._unit[1])

    def train_step(self, data, render_kwargs: Optional[dict] = None, **forced):
        """One iteration of the loop (trainer.py:840-896): -> (loss, render_outputs, sd_outputs, text)."""
        cfg = self.cfg
        if self.scaler is not None:
            return self._train_step_fp16(data, render_kwargs, forced)
        # Update Density Grid
        if self.model.cuda_ray and self.train_step_index % cfg.nerf.update_extra_interval == 0:
            self.model.update_extra_state()

        # Update Iteration Step
        self.train_step_index += 1

        # Forward
        loss, render_outputs, sd_outputs, text = self.train_forward(data, render_kwargs=render_kwargs, **forced)

        # Optimizer Clear Gradient
        for optimizer in self.optimizers.values():
            optimizer.zero_grad()

        self._backward(loss)

        # Optimizer Step
        for optimizer in self.optimizers.values():
            optimizer.step()

        # Scheduler Step
        for scheduler in self.schedulers.values():
            if scheduler is not None:
                scheduler.step()
        return loss, render_outputs, sd_outputs, text

    def _train_step_fp16(self, data, render_kwargs, forced):
        """train_step under cfg.optim.fp16: the same statements with the reference's autocast region and its scaler calls."""
        cfg = self.cfg
        with torch.autocast('cuda', dtype=torch.float16):
            # Update Density Grid
            if self.model.cuda_ray and self.train_step_index % cfg.nerf.update_extra_interval == 0:
                self.model.update_extra_state()

            # Update Iteration Step
            self.train_step_index += 1

            # Forward
            loss, render_outputs, sd_outputs, text = self.train_forward(data, render_kwargs=render_kwargs, **forced)

        # Optimizer Clear Gradient
        for optimizer in self.optimizers.values():
            optimizer.zero_grad()

        self._backward(self.scaler.scale(loss))

        # Optimizer Step: the check for Inf / NaN, the skip and the unscale are the device's
        for optimizer in self.optimizers.values():
            self.scaler.step(optimizer)
        self.scaler.update()

        # Scheduler Step
        for scheduler in self.schedulers.values():
            if scheduler is not None:
                scheduler.step()
        return loss, render_outputs, sd_outputs, text
