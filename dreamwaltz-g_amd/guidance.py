"""Mirror of the reference's SDS guidance seam on the HIP denoiser (boundary B4/B5).

  ControlNetScoreDistillation.__call__(inputs, text_embeds_dict, train_step, max_iteration, add_noise, grad_viz, **kwargs)
                                            /root/reference/core/guidance/basic.py:778-917 (default branch: loss_type 'sds', CFG
                                            with negative text, weight_type 'sjc', guidance_scale 50)
  .preprocess / .prepare_latents            basic.py:354-383,420-438
  .calc_gradients                           basic.py:546-663
  ._predict(latents, text, cond_inputs)     /root/reference/core/guidance/controlnet.py:83-114 (reads self.timestep)
  .prepare_image / .prepare_condition       controlnet.py:33-72 (PIL -> LANCZOS resize -> float/255 -> NCHW -> repeat)
  .encode_images(images)  (differentiable)  /root/reference/core/guidance/vae.py:34-40
  .decode_latents(latents, 'pt')            vae.py:42-46          } B26, opt-in (decoder=True): sd15.VAEDecoderPlan and
  .get_noise_pred / .get_denoise_pred       basic.py:443-527      } dwg_sds_ddpm_step; losses z0 / z0_final / x0 / x0_final
  latent_to_image(guidance, latent, ch)     core/trainer.py:59-68 } (basic.py:846-880, 896-898), grad_viz outputs (907-915)
  SpecifyGradient                           basic.py:213-226
  TimePrioritizedScheduler.get_timestep     /root/reference/core/guidance/time_prior.py:321-352 ('uniform' / 'constant' / 'linear')
Attributes other code reads (basic.py:334-335,453): scheduler.scale_model_input, alphas_cumprod, vae_scale_factor,
pipe.unet.config.sample_size.  Device RNG draw order per call is the reference's (checklist Q12): VAE posterior noise -> timestep ->
latent noise.  Test-only keyword extensions: noise=, posterior_noise= (fixed draws for parity tests).
"""
import types
from typing import Dict, List, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, sd15
from .configs import GuideConfig
from .pgc import build_grad_hook_func, build_pgc_hook_func


class SpecifyGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input_tensor, gt_grad):
        ctx.save_for_backward(gt_grad)
        return torch.ones([1], device=input_tensor.device, dtype=input_tensor.dtype)

    @staticmethod
    def backward(ctx, grad_scale):
        (gt_grad,) = ctx.saved_tensors
        return gt_grad * grad_scale, None


def _fused_ok(*ts):
    """The one-launch forms of the latent algebra (csrc/sds.hip, include/dwg_sds.h) take fp32 CUDA tensors; CPU and non-fp32
    tensors keep the element-wise torch statements."""
    return all(t is not None and t.is_cuda and t.dtype == torch.float32 for t in ts)


_WEIGHT_CODE = {k: _lib.CONSTANTS["DWG_SDS_WEIGHT_" + n] for k, n in
                {None: "NONE", 'sjc': "NONE", 'dreamfusion': "DREAMFUSION", 'latent-nerf': "LATENT_NERF", 'ism': "ISM"}.items()}


class _PosteriorSample(torch.autograd.Function):
    """vae.py:34-40 after the encoder: DiagonalGaussianDistribution(moments).sample() * scaling_factor with the given noise, one launch each
    way (include/dwg_sds.h dwg_sds_posterior_sample / _backward) instead of seven element-wise statements and their autograd twins."""

    @staticmethod
    def forward(ctx, moments, noise, scale):
        m, e = moments.contiguous(), noise.contiguous()
        V, n = m.shape[0], m[0].numel() // 2
        out = torch.empty_like(e)
        _lib.check(_lib.lib().dwg_sds_posterior_sample(V, n, _lib.ptr(m), _lib.ptr(e), float(scale), _lib.ptr(out), _lib.stream(m)), "dwg_sds_posterior_sample")
        ctx.save_for_backward(m, e)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, g):
        m, e = ctx.saved_tensors
        g = g.contiguous().float()
        gm = torch.empty_like(m)
        _lib.check(_lib.lib().dwg_sds_posterior_sample_backward(m.shape[0], m[0].numel() // 2, _lib.ptr(m), _lib.ptr(e), ctx.scale, _lib.ptr(g),
                                                                _lib.ptr(gm), _lib.stream(m)), "dwg_sds_posterior_sample_backward")
        return gm, None, None


class _VAEEncode(torch.autograd.Function):
    """AutoencoderKL.encode(...).latent_dist moments with the frozen encoder inside the autograd graph."""

    @staticmethod
    def forward(ctx, images, plan):
        ctx.plan = plan
        return plan.encode(images).contiguous()      # (a permuted view of the plan's own buffer: always a copy; NCHW-dense for the posterior kernel)

    @staticmethod
    def backward(ctx, g):
        return ctx.plan.backward(g), None


def sd15_alphas_cumprod(device, n=1000, beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).to(device)


def C(value, current_step=None, max_iteration=None) -> float:
    """time_prior.py:17-33 for plain numbers (the schedule-string forms are not used by the shipped recipes)."""
    if isinstance(value, (int, float)):
        return float(value)
    raise NotImplementedError("scheduled min/max timestep strings")


DENOISING_LOSS_TYPES = ('z0', 'z0_final', 'x0', 'x0_final')        # basic.py:344-345: losses on a denoised prediction, not on the score


def inference_timesteps(num_timesteps=50, num_train_timesteps=1000, steps_offset=1) -> List[int]:
    """DDPMScheduler.set_timesteps ('leading' spacing, SD-1.5's scheduler config): arange(n) * (num_train_timesteps // n), reversed, plus
    steps_offset -- 981, 961, ..., 1 for 50 steps.  A host list, largest first."""
    n = int(num_timesteps)
    if not 1 <= n <= num_train_timesteps:
        raise ValueError("num_timesteps must be in 1..%d, got %r" % (num_train_timesteps, num_timesteps))
    ratio = num_train_timesteps // n
    return [(n - 1 - i) * ratio + int(steps_offset) for i in range(n)]


def latent_to_image(guidance, latent: torch.Tensor, color_channel: int):
    """core/trainer.py:59-68: a latent NeRF's render ([B,h,w,4] when color_channel == 3, else [B,4,h,w]) -> the image the VAE decodes it to,
    in the same layout.  Latents larger than 128 are area-averaged down to 128 x 128 first, as there."""
    if color_channel == 3:
        latent = latent.permute(0, 3, 1, 2).contiguous()
    if latent.shape[-2] > 128 or latent.shape[-1] > 128:
        latent = F.interpolate(latent, (128, 128), mode='area')
    image = guidance.decode_latents(latent)
    if color_channel == 3:
        image = image.permute(0, 2, 3, 1).contiguous()
    return image


class ControlNetScoreDistillation:
    def __init__(self, device, unet_cfg: Optional[sd15.UNetConfig] = None, vae_cfg: Optional[sd15.VAEConfig] = None,
                 unet_sd=None, controlnet_sd=None, vae_sd=None, image_hw=512, guidance_scale=None, min_timestep=None,
                 max_timestep=None, seed=0, cfg: Optional[GuideConfig] = None, text_len=77, dtype="f32x", views=1, share_weights_with=None,
                 decoder=False, vae_decoder_sd=None, steps_offset=1):
        """`views` > 1: ONE call distils that many rendered views at once (inputs [V,3,H,W]; the plans are built for a VAE batch of V and a
        denoiser batch of 2 V -- nothing in the reference to mirror, its call is batch 1: checklist Q11).  `share_weights_with`: another
        guidance object of the same dtype whose kernel-layout weights this one's plans point at (no second copy in HBM).
        `decoder=True` (B26) adds the native VAE decoder (sd15.VAEDecoderPlan, built on demand per (latent_hw, batch), all plans on one
        `Weights` of `vae_decoder_sd` -- `post_quant_conv.*` / `decoder.*`; None: random weights at seed + 3) and with it decode_latents,
        get_noise_pred, get_denoise_pred, the z0 / z0_final / x0 / x0_final losses and the grad_viz outputs.  Off (the default) the object
        allocates and launches what it did before and each of those raises.  `steps_offset`: the inference scheduler's (SD-1.5: 1)."""
        self.device = torch.device(device)
        self.views = int(views)
        self.dtype_name = sd15.dtype_name(dtype)          # precision of the denoiser / VAE plans: "f32x" (default: the reference's fp32 GS-stage
                                                          # results, configs/__init__.py:236,241, on the 16-bit MFMA pipe) | "f32" (exact-f32
                                                          # MFMA) | "f16" (its --guide.dtype fp16) | "bf16" (reduced precision, opt-in only)
        self.cfg = cfg if cfg is not None else GuideConfig()
        self.unet_cfg = unet_cfg or sd15.UNetConfig()
        self.vae_cfg = vae_cfg or sd15.VAEConfig()
        # BasicStableDiffusion.__init__ (basic.py:229-267, 344-345): what is not built is refused before any plan is
        self.loss_type, self.weight_type = self.cfg.sds_loss_type, self.cfg.sds_weight_type
        self.has_decoder = bool(decoder)
        if self.loss_type == 'ism':
            raise NotImplementedError("sds_loss_type 'ism' (interval score matching: a DDIM inversion per step, basic.py:665-776) is not built")
        if self.loss_type in DENOISING_LOSS_TYPES and not self.has_decoder:
            raise NotImplementedError("sds_loss_type %r is a denoising loss: it needs the scheduler step and the native VAE decoder -- construct "
                                      "ControlNetScoreDistillation(..., decoder=True)" % (self.loss_type,))
        if self.loss_type not in ('sds',) + DENOISING_LOSS_TYPES or self.weight_type not in ('sjc', 'dreamfusion', 'latent-nerf', 'ism'):
            raise NotImplementedError("only the score-based 'sds' loss of the shipped recipes is on the hot path")
        self.is_denoising_mode = self.loss_type in DENOISING_LOSS_TYPES
        self.steps_offset = int(steps_offset)
        shared = share_weights_with
        if shared is not None and shared.dtype_name != self.dtype_name:
            raise ValueError("share_weights_with: plans of dtype %s cannot point at %s weights" % (self.dtype_name, shared.dtype_name))
        if shared is None:
            if unet_sd is None:        # random-init weights of the SD-1.5 architecture (no checkpoints offline)
                unet_sd = sd15.random_state_dict(sd15.unet_param_shapes(self.unet_cfg), seed=seed)
            if controlnet_sd is None:
                controlnet_sd = sd15.random_state_dict(sd15.controlnet_param_shapes(self.unet_cfg), seed=seed + 1)
            if vae_sd is None:
                vae_sd = sd15.random_state_dict(sd15.vae_encoder_param_shapes(self.vae_cfg), seed=seed + 2)
        self._decoder_weights, self._decoder_plans = None, {}
        if self.has_decoder:
            if vae_decoder_sd is None and shared is not None and getattr(shared, "_decoder_weights", None) is not None:
                self._decoder_weights = shared._decoder_weights
            else:
                if vae_decoder_sd is None:
                    vae_decoder_sd = sd15.random_state_dict(sd15.vae_decoder_param_shapes(self.vae_cfg), seed=seed + 3)
                for key in sd15.vae_decoder_param_shapes(self.vae_cfg):
                    if key not in vae_decoder_sd:
                        raise KeyError("vae_decoder_sd lacks the decoder key %r" % key)
                self._decoder_weights = sd15.Weights(vae_decoder_sd, self.device, self.dtype_name)      # (copies are made as plans ask for them)
        self.image_hw = image_hw
        down = 2 ** (len(self.vae_cfg.block_out_channels) - 1)
        self.latent_hw = image_hw // down
        # the CFG entries of a view share everything in front of the first cross-attention (sd15.DenoiserPlan `shared_prefix`); the exact-f32
        # plans, whose attention is three dwg_gemm launches over image x head, keep the whole CFG batch
        self.denoiser = sd15.DenoiserPlan(self.unet_cfg, unet_sd, controlnet_sd, self.device, batch=2 * self.views, latent_hw=self.latent_hw,
                                          text_len=text_len, dtype=self.dtype_name, views=self.views, shared_prefix=self.dtype_name != "f32",
                                          weights=shared.denoiser.weights if shared is not None else None)      # CLIP's 77 tokens; static
        self.vae = sd15.VAEEncoderPlan(self.vae_cfg, vae_sd, self.device, image_hw=image_hw, dtype=self.dtype_name, batch=self.views,
                                       weights=shared.vae.weights if shared is not None else None)
        # BasicStableDiffusion.__init__ (basic.py:229-267)
        self.initial_guidance_scale = self.cfg.guidance_scale if guidance_scale is None else guidance_scale
        self.guidance_adjust = self.cfg.guidance_adjust
        self.do_classifier_free_guidance = self.initial_guidance_scale > 1.0
        self.use_negative_text = self.cfg.use_negative_text
        self.input_interpolate = self.cfg.input_interpolate
        self.conditioning_scale = self.cfg.controlnet_scale
        if self.conditioning_scale != 1.0:
            raise NotImplementedError("controlnet_scale != 1")
        self.vae_scale_factor = down
        self.scaling_factor = self.vae_cfg.scaling_factor
        self.default_latent_size = self.latent_hw
        self.default_image_size = self.default_latent_size * self.vae_scale_factor
        self.pipe = types.SimpleNamespace(unet=types.SimpleNamespace(config=types.SimpleNamespace(sample_size=self.latent_hw)))
        self.scheduler = types.SimpleNamespace(scale_model_input=lambda sample, timestep=None: sample)   # DDPM / PNDM: identity
        self.alphas_cumprod = sd15_alphas_cumprod(self.device)
        self.num_train_timesteps = 1000
        self.denoiser.temb_rows = self.num_train_timesteps + 1      # the integer-timestep embedding table covers the scheduler's range
        self.time_sampling = self.cfg.time_sampling
        self.min_step_cfg = self.cfg.min_timestep if min_timestep is None else min_timestep
        self.max_step_cfg = self.cfg.max_timestep if max_timestep is None else max_timestep
        self.timestep, self.guidance_scale = None, self.initial_guidance_scale
        self._side = None                 # side stream of the denoiser's prelude (preprocess)

    # -- plans ---------------------------------------------------------------------------------------------------------
    def plans(self):
        return (self.denoiser.plan, self.vae.fwd, self.vae.bwd)

    def range_report(self, top=8):
        """Where the f32x plans stand against the range of their storage format after the LAST call (round 5; sd15.Plan.range_report): per
        plan -- denoiser, VAE forward, VAE backward -- the count of saturated (+-65504) / below-normal-range / non-finite stored values, the
        largest magnitude and the layers with the most hits, plus the same counts for the packed weights.  `ok` is False when anything
        saturated or went non-finite: the results then left what the reference's fp32 stage (/root/reference/core/guidance/basic.py:233,
        configs/__init__.py:236,241) would have produced and DWG_BIND_DTYPE=f32 (exact-f32 plans) is the fallback.  One stream
        synchronisation and ~10^3 small launches: call it every few hundred steps, not every step.  Plans of other precisions: None."""
        if self.dtype_name != "f32x":
            return None
        names = ("denoiser", "vae_forward", "vae_backward")
        rep = {n: p.range_report(top) for n, p in zip(names, self.plans())}
        w = {}
        for n, ws in (("unet", self.denoiser.weights[0]), ("controlnet", self.denoiser.weights[1]), ("vae", self.vae.weights)):
            w[n] = dict(getattr(ws, "range", {"elements": 0, "saturated": 0, "subnormal": 0, "max_abs": 0.0}))
        rep["weights"] = w
        bad = sum(rep[n]["saturated"] + rep[n]["nonfinite"] for n in names) + sum(v["saturated"] for v in w.values())
        rep["ok"] = bad == 0
        return rep

    def capture_graphs(self):
        for p in self.plans() + (self.denoiser.pre,):
            p.capture()
        self._graphs_captured = True                # decoder plans (B26) built from here on are captured at their first use
        for d in self._decoder_plans.values():
            d.capture()

    def set_use_graphs(self, on: bool):
        for p in self.plans() + (self.denoiser.pre,) + tuple(d.plan for d in self._decoder_plans.values()):
            p.use_graph = bool(on)
        self._use_graphs = bool(on)

    # -- time_prior.py:292-352 ------------------------------------------------------------------------------------------
    @property
    def min_step(self):
        return int(self.num_train_timesteps * C(self.min_step_cfg))

    @property
    def max_step(self):
        return int(self.num_train_timesteps * C(self.max_step_cfg))

    def get_timestep(self, batch_size=1, train_step=None, max_iteration=None, generator=None):
        if self.time_sampling == 'uniform':
            return torch.randint(self.min_step, self.max_step + 1, [batch_size], dtype=torch.long, device=self.device,
                                 generator=generator)                                                                   # RNG draw #2
        if self.time_sampling == 'constant':
            mid = (self.min_step + self.max_step) // 2
            return torch.randint(mid, mid + 1, [batch_size], dtype=torch.long, device=self.device, generator=generator)
        if self.time_sampling == 'linear':
            delta = (self.max_step - self.min_step) / (max_iteration - 1)
            return torch.ones([batch_size], dtype=torch.long, device=self.device) * int(self.max_step - (train_step - 1) * delta)
        raise NotImplementedError(self.time_sampling)

    def add_noise(self, latents, noise, timestep):
        """DDPMScheduler.add_noise [3P-memory]: sqrt(acp_t) x + sqrt(1 - acp_t) eps."""
        if (_fused_ok(latents, noise) and not (latents.requires_grad and torch.is_grad_enabled()) and torch.is_tensor(timestep) and timestep.is_cuda
                and timestep.dtype == torch.long and timestep.numel() == latents.shape[0] and latents[0].numel() % 4 == 0
                and latents.shape == noise.shape):
            x, e = latents.contiguous(), noise.contiguous()
            out = torch.empty_like(x)
            _lib.check(_lib.lib().dwg_sds_add_noise(x.shape[0], x[0].numel(), _lib.ptr(x), _lib.ptr(e), _lib.ptr(self.alphas_cumprod),
                                                    int(self.alphas_cumprod.numel()), _lib.ptr(timestep.contiguous()), _lib.ptr(out), _lib.stream(x)),
                       "dwg_sds_add_noise")
            return out
        a = self.alphas_cumprod[timestep].reshape(-1, 1, 1, 1)
        return a.sqrt() * latents + (1 - a).sqrt() * noise

    def get_guidance_scale(self, train_step, max_iteration):
        """basic.py:404-418."""
        s0 = self.initial_guidance_scale
        if self.guidance_adjust == 'constant':
            return s0
        if self.guidance_adjust == 'uniform':
            return np.random.uniform(7.5, s0)
        if self.guidance_adjust == 'linear':
            return s0 - (train_step - 1) * (s0 - 7.5) / (max_iteration - 1)
        if self.guidance_adjust == 'linear_reverse':
            return 7.5 + (train_step - 1) * (s0 - 7.5) / (max_iteration - 1)
        raise NotImplementedError

    # -- vae.py:34-40 ----------------------------------------------------------------------------------------------------
    def encode_images(self, images: torch.Tensor, posterior_noise: Optional[torch.Tensor] = None, generator=None) -> torch.Tensor:
        moments = _VAEEncode.apply(images, self.vae)
        mean, logvar = moments.chunk(2, dim=1)
        if posterior_noise is None:
            posterior_noise = torch.randn(mean.shape, device=mean.device, dtype=mean.dtype, generator=generator)      # RNG draw #1
        if _fused_ok(moments, posterior_noise) and moments[0].numel() % 8 == 0:
            return _PosteriorSample.apply(moments, posterior_noise, self.scaling_factor)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        return (mean + std * posterior_noise) * self.scaling_factor

    def prepare_latents(self, inputs: torch.Tensor, posterior_noise=None, generator=None):
        """basic.py:354-383 (RGB inputs)."""
        if inputs.size(1) != 3:
            raise NotImplementedError("latent-space inputs")
        default_size = (self.default_image_size, self.default_image_size)
        if self.input_interpolate and tuple(inputs.shape[-2:]) != default_size:
            inputs = F.interpolate(inputs, default_size, mode='bilinear', align_corners=False)
        assert tuple(inputs.shape[-2:]) == default_size, inputs.shape
        return self.encode_images(inputs, posterior_noise, generator=generator), inputs

    def preprocess(self, inputs, train_step, max_iteration, posterior_noise=None, generator=None, **kwargs):
        """basic.py:420-438.  `generator`: the device generator every random draw of the call comes from (None: the default one, as in
        the reference) -- a multi-view step gives each view its own stream.
        Round 6: the two random draws of this stage keep their order (#1 the VAE posterior noise, #2 the timestep), but both are made BEFORE
        the encoder runs -- neither depends on its result -- so that the part of the denoiser that needs only the timestep, the text and the
        condition image (sd15.DenoiserPlan.prefetch: time embeddings, ControlNet hint embedding, text k / v projections) can run on a side
        stream UNDER the VAE encoder (`prefetch`: (text_embeds_dict, cond_inputs) of the call, or None)."""
        batch_size = inputs.size(0)
        prefetch = kwargs.pop('_prefetch', None)
        # (a step being captured into ONE graph keeps the prelude on the capturing stream, in front of the main plan: sd15.DenoiserPlan.run)
        early = (prefetch is not None and inputs.is_cuda and inputs.size(1) == 3 and not torch.cuda.is_current_stream_capturing())
        if early and posterior_noise is None:
            shape = (batch_size, self.vae_cfg.latent_channels, self.latent_hw, self.latent_hw)
            posterior_noise = torch.randn(shape, device=inputs.device, dtype=inputs.dtype, generator=generator)        # RNG draw #1
        if early:
            self.guidance_scale = kwargs.pop('guidance_scale') if 'guidance_scale' in kwargs else self.get_guidance_scale(train_step, max_iteration)
            self.timestep = (kwargs.pop('timestep') if 'timestep' in kwargs
                             else self.get_timestep(batch_size, train_step, max_iteration, generator=generator))
            text_embeds_dict, cond_inputs = prefetch
            if self.do_classifier_free_guidance and torch.is_tensor(cond_inputs):
                with torch.no_grad():
                    text_keys = ('neg', 'text') if self.use_negative_text else ('null', 'text')
                    text = self.prepare_text_embeddings(text_embeds_dict, text_keys)
                    cond = self.prepare_condition(cond_inputs, cond_height=self.latent_hw * self.vae_scale_factor,
                                                  cond_width=self.latent_hw * self.vae_scale_factor, batch_size=self.views, dtype=torch.float32)
                    if self._side is None:
                        self._side = torch.cuda.Stream(device=self.device)
                    self.denoiser.prefetch(self.timestep, text, cond[:self.views], stream=self._side)
        latents, inputs = self.prepare_latents(inputs, posterior_noise, generator=generator)
        if not early:
            self.guidance_scale = kwargs.pop('guidance_scale') if 'guidance_scale' in kwargs else self.get_guidance_scale(train_step, max_iteration)
            self.timestep = (kwargs.pop('timestep') if 'timestep' in kwargs
                             else self.get_timestep(batch_size, train_step, max_iteration, generator=generator))
        return latents, inputs, kwargs

    # -- controlnet.py:33-72 ---------------------------------------------------------------------------------------------
    def prepare_image(self, image, width, height, batch_size, num_images_per_prompt, device, dtype) -> torch.Tensor:
        from PIL import Image
        if isinstance(image, Image.Image):
            image = [image]
        if not isinstance(image, torch.Tensor):
            if isinstance(image[0], Image.Image):
                image = [np.array(i.resize((width, height), resample=Image.Resampling.LANCZOS))[None, :] for i in image]
                image = np.concatenate(image, axis=0)
                image = np.array(image).astype(np.float32) / 255.0
                image = torch.from_numpy(image.transpose(0, 3, 1, 2))
            elif isinstance(image[0], torch.Tensor):
                image = torch.cat(image, dim=0)
        repeat_by = batch_size if image.shape[0] == 1 else num_images_per_prompt
        if repeat_by != 1:                       # (repeat_interleave(1) would still copy the image: one launch per call for nothing)
            image = image.repeat_interleave(repeat_by, dim=0)
        return image.to(device=device, dtype=dtype)

    def prepare_condition(self, cond_inputs, cond_width, cond_height, batch_size, dtype) -> torch.Tensor:
        return self.prepare_image(cond_inputs, width=cond_width, height=cond_height, batch_size=batch_size, num_images_per_prompt=1,
                                  device=self.device, dtype=dtype)

    # -- controlnet.py:83-114 --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _predict(self, latents_model_input, text_embeddings, cond_inputs):
        """latents [2,4,h,w] (or [1,4,h,w]: the shared-prefix plans), text [2,77,768], cond_inputs: list[PIL] | PIL | tensor [1 or 2,3,8h,8w] in [0,1].  The timestep is
        self.timestep, as in the reference."""
        _, _, lh, lw = latents_model_input.shape
        # the reference repeats the condition to the CFG batch (controlnet.py:50-54: batch_size = latents.size(0)); the repeated rows are identical
        # and only the first `views` are read below (the hint embedding is computed once per view and broadcast), so they are not made
        cond = self.prepare_condition(cond_inputs, cond_height=lh * self.vae_scale_factor, cond_width=lw * self.vae_scale_factor,
                                      batch_size=self.views, dtype=torch.float32)
        if self.denoiser.shared_prefix and latents_model_input.shape[0] == 2 * self.views:
            # this seam's caller in the reference hands over its own repeat of the noisy latents (basic.py:570 `torch.cat([latents_noisy] * 2)`):
            # the plan takes one copy per view
            latents_model_input = latents_model_input[:self.views]
        self.denoiser.set_inputs(latents_model_input, self.timestep, text_embeddings, cond[:self.views])
        return self.denoiser.run()

    def prepare_text_embeddings(self, text_embeds_dict: dict, text_keys: tuple):
        embeds = [text_embeds_dict[k] for k in text_keys]
        # the prompts' embeddings are computed once per run (core/trainer.py:232-263) and handed over unchanged every step: the concatenation
        # of the SAME tensors (identity + version counter + storage) is kept instead of being rebuilt twice per call (prefetch + prediction)
        # (never while a stream capture is recording: a captured step must CONTAIN the concatenation of its static text buffers)
        capturing = embeds[0].is_cuda and torch.cuda.is_current_stream_capturing()
        key = tuple((id(e), e._version, e.data_ptr(), tuple(e.shape)) for e in embeds) + (self.views,)
        cache = self.__dict__.setdefault("_text_cat", {})
        hit = None if capturing else cache.get(key)
        if hit is not None and all(a is b for a, b in zip(hit[0], embeds)):
            return hit[1]
        src = embeds
        if self.views > 1:          # one embedding per view; a single one is shared by all views
            embeds = [e.expand(self.views, -1, -1) if e.size(0) == 1 else e for e in embeds]
        out = torch.concat(embeds, dim=0)
        if not capturing:
            if len(cache) >= 16:
                cache.clear()
            cache[key] = (list(src), out)
        return out

    def draw_view_randoms(self, generator=None, train_step=None, max_iteration=None):
        """The three device draws of ONE view's call in the reference's order (checklist Q12): VAE posterior noise [1,4,h,w], timestep [1],
        latent noise [1,4,h,w].  A multi-view call is fed the per-view draws stacked (posterior_noise=, timestep=, noise=), so every view
        sees exactly the numbers its own single-view call would draw from the same generator state."""
        shape = (1, self.vae_cfg.latent_channels, self.latent_hw, self.latent_hw)
        pn = torch.randn(shape, device=self.device, generator=generator)
        t = self.get_timestep(1, train_step, max_iteration, generator=generator)
        n = torch.randn(shape, device=self.device, generator=generator)
        return pn, t, n

    # -- B26: the decoder side (vae.py:42-46, basic.py:443-527) -------------------------------------------------------------
    def _need_decoder(self, what):
        if not self.has_decoder:
            raise RuntimeError("%s needs the native VAE decoder and scheduler step, which this guidance object was built without: construct "
                               "ControlNetScoreDistillation(..., decoder=True)" % what)

    def decoder_plan(self, latent_hw, batch):
        """The decoder plan for [batch, C, latent_hw, latent_hw] latents, built (and captured) at its first use; every plan points at the one
        `Weights` of this object."""
        self._need_decoder("decoder_plan")
        key = (int(latent_hw), int(batch))
        plan = self._decoder_plans.get(key)
        if plan is None:
            plan = sd15.VAEDecoderPlan(self.vae_cfg, None, self.device, latent_hw=key[0], dtype=self.dtype_name, batch=key[1],
                                       weights=self._decoder_weights)
            if getattr(self, "_graphs_captured", False):
                plan.capture()
                plan.plan.use_graph = getattr(self, "_use_graphs", True)
            self._decoder_plans[key] = plan
        return plan

    @torch.no_grad()
    def decode_latents(self, latents, output_type='pt'):
        """vae.py:42-46: latents [B,4,h,h] -> images [B,3,8h,8h] in [0,1] (VaeImageProcessor.postprocess 'pt')."""
        self._need_decoder("decode_latents")
        if output_type != 'pt':
            raise NotImplementedError("decode_latents(output_type=%r): only 'pt' (a [B,3,H,W] tensor in [0,1]) is built" % (output_type,))
        if not torch.is_tensor(latents) or latents.dim() != 4:
            raise ValueError("decode_latents: latents must be a [B,C,h,h] tensor, got %r" % (getattr(latents, "shape", type(latents)),))
        return self.decoder_plan(latents.shape[-1], latents.shape[0]).decode(latents)

    @torch.no_grad()
    def get_noise_pred(self, latents_noisy, text_embeddings, guidance_rescale: float = 0.0, timestep=None, **kwargs):
        """basic.py:443-467: the classifier-free-combined prediction for latents [V,4,h,w].  `timestep` ([V] long; None: self.timestep, as in the
        reference) predicts at another step of the chain without disturbing self.timestep."""
        self._need_decoder("get_noise_pred")
        if not self.do_classifier_free_guidance:
            raise NotImplementedError("guidance_scale <= 1 (no classifier-free guidance): the plans are built for the CFG batch of 2")
        if guidance_rescale > 0.0:
            raise NotImplementedError("guidance_rescale")
        latents_model_input = latents_noisy if self.denoiser.shared_prefix else torch.cat([latents_noisy] * 2, dim=0)
        kept = self.timestep
        if timestep is not None:
            self.timestep = timestep
        try:
            latents_model_input = self.scheduler.scale_model_input(latents_model_input, self.timestep)
            noise_pred = self._predict(latents_model_input, text_embeddings, **kwargs)
        finally:
            self.timestep = kept
        noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
        return noise_pred_uncond + self.guidance_scale * (noise_pred_text - noise_pred_uncond)

    def inference_timesteps(self, num_timesteps=50):
        return inference_timesteps(num_timesteps, self.num_train_timesteps, self.steps_offset)

    def ddpm_step(self, sample, noise_pred, timestep, prev_timestep, noise=None, want_original=True, want_prev=True):
        """One reverse step per view (include/dwg_sds.h dwg_sds_ddpm_step: DDPMScheduler.step, epsilon prediction, fixed_small variance, no
        clipping), one launch, timesteps read on the device.  Returns (pred_original_sample, prev_sample), None for the one not wanted."""
        x, e = sample.contiguous(), noise_pred.contiguous()
        if not (_fused_ok(x, e) and x.shape == e.shape and x[0].numel() % 4 == 0):
            raise ValueError("ddpm_step: sample and noise_pred must be fp32 CUDA tensors of one shape, 4 | elements per view")
        t, tp = timestep.to(torch.long).contiguous(), prev_timestep.to(torch.long).contiguous()
        if not (t.is_cuda and tp.is_cuda and t.numel() == x.shape[0] and tp.numel() == x.shape[0]):
            raise ValueError("ddpm_step: one timestep and one previous timestep per view, on the device")
        z = None
        if want_prev:
            if noise is None or noise.shape != x.shape or not _fused_ok(noise):
                raise ValueError("ddpm_step: prev_sample needs the variance noise, an fp32 CUDA tensor of the sample's shape")
            z = noise.contiguous()
        x0 = torch.empty_like(x) if want_original else None
        prev = torch.empty_like(x) if want_prev else None
        _lib.check(_lib.lib().dwg_sds_ddpm_step(x.shape[0], x[0].numel(), _lib.ptr(x), _lib.ptr(e), _lib.ptr(z), _lib.ptr(self.alphas_cumprod),
                                                int(self.alphas_cumprod.numel()), _lib.ptr(t), _lib.ptr(tp), _lib.ptr(x0), _lib.ptr(prev),
                                                _lib.stream(x)), "dwg_sds_ddpm_step")
        return x0, prev

    @torch.no_grad()
    def get_denoise_pred(self, latents_noisy, noise_pred, text_embeddings, iterative, num_timesteps=50, step_noise=None, generator=None, **kwargs):
        """basic.py:469-527.  The training timestep of each view is moved to the inference grid by the reference's rule (the first grid step that
        is not above it; the grid's first step when all are), one scheduler step from there gives latents_1orig / latents_1step, and with
        `iterative` the rest of the grid is walked down to latents_final, each step predicted at ITS timestep (get_noise_pred's override).
        `step_noise`: the variance noise, a sequence indexed by grid position (step_noise[j] [V,4,h,w] is used by the step taken at grid
        step j); None: drawn on the device from `generator`, one draw per step with t > 0.  Views that start lower on the grid wait, unchanged,
        until the walk reaches them: all views are predicted in one denoiser call per grid step."""
        self._need_decoder("get_denoise_pred")
        bs = latents_noisy.shape[0]
        if bs != self.views:
            raise ValueError("get_denoise_pred: the denoiser plan is built for %d view(s), got a batch of %d" % (self.views, bs))
        grid_host = self.inference_timesteps(num_timesteps)
        n, ratio = len(grid_host), self.num_train_timesteps // len(grid_host)
        grid = torch.tensor(grid_host, device=self.device, dtype=torch.long)
        large_enough_idxs = grid.expand([bs, -1]) > self.timestep[:bs].unsqueeze(-1)
        idxs = (~large_enough_idxs).to(torch.int8).argmax(dim=1)      # first False; 0 when there is none (torch.min over booleans, basic.py:486)
        t = grid[idxs]
        fracs = list((t / self.num_train_timesteps).cpu().numpy())
        idx_host = [int(i) for i in idxs.tolist()]

        def noise_at(j):
            if step_noise is not None:
                return step_noise[j].to(self.device, torch.float32)
            if grid_host[j] > 0:
                return torch.randn(latents_noisy.shape, device=self.device, dtype=torch.float32, generator=generator)
            return torch.zeros(latents_noisy.shape, device=self.device, dtype=torch.float32)      # (never read: the step at t = 0 adds no noise)

        if len(set(idx_host)) == 1:
            z = noise_at(idx_host[0])
        elif step_noise is not None:
            z = torch.cat([noise_at(j)[b:b + 1] for b, j in enumerate(idx_host)])
        else:
            z = torch.randn(latents_noisy.shape, device=self.device, dtype=torch.float32, generator=generator)
        latents_1orig, latents_1step = self.ddpm_step(latents_noisy, noise_pred, t, t - ratio, z)
        step_outputs = {"noise_levels": fracs, "latents_noisy": latents_noisy, "latents_1orig": latents_1orig, "latents_1step": latents_1step}
        if iterative:
            latents = latents_1step
            for j in range(min(idx_host) + 1, n):
                tj = torch.full([bs], grid_host[j], device=self.device, dtype=torch.long)
                pred = self.get_noise_pred(latents_noisy=latents, text_embeddings=text_embeddings, timestep=tj, **kwargs)
                _, nxt = self.ddpm_step(latents, pred, tj, tj - ratio, noise_at(j), want_original=False)
                started = [i < j for i in idx_host]
                latents = nxt if all(started) else torch.where(torch.tensor(started, device=self.device).view(-1, 1, 1, 1), nxt, latents)
            step_outputs["latents_final"] = latents
        return step_outputs

    def calc_gradients(self, latents_noisy, text_embeds_dict, noise, guidance_rescale: float = 0.0, train_step=None, max_iteration=None,
                       **kwargs):
        """basic.py:546-663, the 'sds' branch."""
        if self.do_classifier_free_guidance:
            text_keys = ('neg', 'text') if self.use_negative_text else ('null', 'text')
            text_embeddings = self.prepare_text_embeddings(text_embeds_dict, text_keys)
            # (a shared-prefix plan takes the noisy latents once per view: the repeat of basic.py:570 is what it does not compute twice)
            latents_model_input = latents_noisy if self.denoiser.shared_prefix else torch.cat([latents_noisy] * 2, dim=0)
        else:
            raise NotImplementedError("guidance_scale <= 1 (no classifier-free guidance): the plans are built for the CFG batch of 2")
        latents_model_input = self.scheduler.scale_model_input(latents_model_input, self.timestep)
        noise_pred = self._predict(latents_model_input, text_embeddings, **kwargs)
        plain = not (guidance_rescale > 0.0 or self.cfg.grad_latent_clip or self.cfg.grad_latent_norm) and self.weight_type in _WEIGHT_CODE
        if (plain and _fused_ok(noise_pred, noise) and noise_pred.shape[0] == 2 * noise.shape[0] and noise_pred.shape[1:] == noise.shape[1:]
                and noise[0].numel() % 4 == 0 and torch.is_tensor(self.timestep) and self.timestep.is_cuda and self.timestep.dtype == torch.long
                and self.timestep.numel() == noise.shape[0]):
            # basic.py:602-646 in one launch: classifier-free combination, minus the noise, timestep weight, nan_to_num
            noise_pred, noise = noise_pred.contiguous(), noise.contiguous()       # (the plan hands its output over as a channels-last view)
            gradients, combined = torch.empty_like(noise), torch.empty_like(noise)
            _lib.check(_lib.lib().dwg_sds_gradient(noise.shape[0], noise[0].numel(), _lib.ptr(noise_pred), _lib.ptr(noise), _lib.ptr(self.alphas_cumprod),
                                                   int(self.alphas_cumprod.numel()), _lib.ptr(self.timestep.contiguous()), float(self.guidance_scale),
                                                   _WEIGHT_CODE[self.weight_type], int(bool(self.cfg.grad_latent_nan_to_num)), _lib.ptr(gradients),
                                                   _lib.ptr(combined), _lib.stream(noise)), "dwg_sds_gradient")
            return gradients, combined, text_embeddings
        noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
        noise_pred = noise_pred_uncond + self.guidance_scale * (noise_pred_text - noise_pred_uncond)
        if guidance_rescale > 0.0:
            raise NotImplementedError("guidance_rescale")
        gradients = noise_pred - noise
        if self.weight_type is not None:
            alphas = self.alphas_cumprod[self.timestep]
            if self.weight_type == 'dreamfusion':
                w = 1 - alphas
            elif self.weight_type == 'latent-nerf':
                w = (1 - alphas) * (alphas ** 0.5)
            elif self.weight_type == 'ism':
                w = ((1 - alphas) / alphas) ** 0.5
            else:                                  # 'sjc'
                w = None
            if w is not None:
                gradients = gradients * w.reshape(-1, 1, 1, 1)
        if self.cfg.grad_latent_clip:
            gs = gradients.nan_to_num(0.0, 0.0, 0.0)
            std = ((gs ** 2).sum() / gs.count_nonzero()) ** 0.5 * self.cfg.grad_latent_clip_scale
            gradients = torch.minimum(torch.maximum(gradients, -std), std).nan_to_num(0.0)
        if self.cfg.grad_latent_norm:
            gradients = torch.nn.functional.normalize(gradients.nan_to_num(0.0, 0.0, 0.0), p=2, dim=(1, 2, 3))
        if self.cfg.grad_latent_nan_to_num:
            gradients = torch.nan_to_num(gradients)
        return gradients, noise_pred, text_embeddings

    def __call__(self, inputs: torch.Tensor, text_embeds_dict: Dict[str, torch.Tensor], train_step: int = 0, max_iteration: int = 1,
                 add_noise: bool = True, grad_viz: bool = False, noise=None, posterior_noise=None, generator=None, **kwargs):
        """inputs [V,3,H,W] rendered image(s) in [0,1] (requires grad; V = self.views, 1 in the reference).  Returns the reference's result dict."""
        if inputs.size(0) != self.views:
            raise ValueError("this guidance object's plans are built for %d view(s) per call, got a batch of %d" % (self.views, inputs.size(0)))
        if self.is_denoising_mode and inputs.is_cuda and torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("sds_loss_type %r inside a captured step (step_graph): the scheduler grid is read on the host" % (self.loss_type,))
        if inputs.size(1) == 3:                                            # pixel-wise gradient operations (basic.py:795-817)
            if self.cfg.pgc_clip_rgb >= 0:
                inputs.register_hook(build_pgc_hook_func(self.cfg.pgc_clip_rgb, self.cfg.pgc_suppress_type, kwargs.get('scaler')))
            elif self.cfg.grad_rgb_clip or self.cfg.grad_rgb_norm:
                mask = kwargs.pop('mask_inputs') if 'mask_inputs' in kwargs else None
                inputs.register_hook(build_grad_hook_func(self.cfg.grad_rgb_clip, self.cfg.grad_rgb_norm, self.cfg.grad_rgb_clip_scale,
                                                          scaler=kwargs.get('scaler'), mask=mask))
        kwargs.pop('scaler', None)
        latents, inputs, kwargs = self.preprocess(inputs, train_step, max_iteration, posterior_noise=posterior_noise, generator=generator,
                                                  _prefetch=(text_embeds_dict, kwargs.get('cond_inputs')), **kwargs)
        with torch.no_grad():
            if noise is None:
                noise = torch.randn(latents.shape, device=latents.device, dtype=latents.dtype, generator=generator)   # RNG draw #3
            latents_noisy = self.add_noise(latents, noise, self.timestep) if add_noise else latents
        outputs = {'latents': latents, 'timestep': self.timestep}
        den_kw = {k: kwargs.pop(k) for k in ('num_timesteps', 'step_noise') if k in kwargs}      # get_denoise_pred's own (test / viz extensions)
        if self.is_denoising_mode:                                         # basic.py:846-880, 896-898
            with torch.no_grad():
                text_keys = ('neg', 'text') if self.use_negative_text else ('null', 'text')
                text_embeddings = self.prepare_text_embeddings(text_embeds_dict, text_keys)
                noise_pred = self.get_noise_pred(latents_noisy=latents_noisy, text_embeddings=text_embeddings, **kwargs)
                outputs.update(self.get_denoise_pred(latents_noisy=latents_noisy, noise_pred=noise_pred, text_embeddings=text_embeddings,
                                                     iterative=(self.cfg.grad_viz or self.loss_type.endswith('_final')), generator=generator,
                                                     **den_kw, **kwargs))
                if self.loss_type == 'z0':
                    sources, targets = latents, outputs['latents_1orig']
                elif self.loss_type == 'z0_final':
                    sources, targets = latents, outputs['latents_final']
                elif self.loss_type == 'x0':
                    sources, targets = inputs, self.decode_latents(outputs['latents_1orig'])
                else:                                                      # 'x0_final'
                    sources, targets = inputs, self.decode_latents(outputs['latents_final'])
                gradients = (sources - targets).detach()
            # "SpecifyGradient is not straightforward, use a reparameterization trick instead" (basic.py:897): d loss / d sources = (sources - targets) / B
            diffusion_loss = 0.5 * F.mse_loss(sources, targets, reduction="sum") / sources.size(0)
        else:
            with torch.no_grad():
                gradients, noise_pred, text_embeddings = self.calc_gradients(latents_noisy=latents_noisy, text_embeds_dict=text_embeds_dict, noise=noise,
                                                                             train_step=train_step, max_iteration=max_iteration, **kwargs)
                sources = latents
                targets = (sources - gradients).detach()
            diffusion_loss = SpecifyGradient.apply(sources, gradients)
        outputs['sources'], outputs['targets'], outputs['gradients'] = sources, targets, gradients
        outputs['diffusion_loss'] = diffusion_loss
        # basic.py:907-915.  An object built without the decoder keeps ignoring grad_viz, as it always has
        if grad_viz and self.has_decoder and 'latents_final' not in outputs:
            outputs.update(self.get_denoise_pred(latents_noisy=latents_noisy, noise_pred=noise_pred, text_embeddings=text_embeddings, iterative=True,
                                                 generator=generator, **den_kw, **kwargs))
        return outputs
