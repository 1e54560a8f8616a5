"""The loss scaler of the stage-I step under optim.fp16 (boundary B21): torch.cuda.amp.GradScaler's surface as the reference's loop uses
it (core/trainer.py:840-896: scale(loss).backward(), step(optimizer) for every optimizer, update()) over the flat fused Adam, with the
whole decision on the device (csrc/grad_scaler.hip through include/dwg_grad_scaler.h).

torch's GradScaler.step reads found_inf back to the host at the end of every backward and decides there whether optimizer.step() runs;
the flat optimizer's parameters are stepped through raw pointers and its per-group step counts (bias correction) would have to follow
that host decision.  Here the check (dwg_grads_nonfinite), the skip, the unscale (folded into the Adam kernel's gradient factor), the
step counts and the scale schedule (dwg_scaler_update = torch._amp_update_scale_) live on the device: a step adds four launches and no
host read.

Two differences from torch, on purpose:
  * after step() the flat gradient is still SCALED: the unscale happens inside the Adam launch, the buffer is read once.  There is no
    in-place unscale_(): it raises NotImplementedError by name.
  * (as in torch) get_scale() between step() and update() returns the old scale.

state_dict() / load_state_dict() use torch's keys, so the 'scaler' entry of a checkpoint is interchangeable with the reference's.
"""
import ctypes

import torch

from . import _lib
from .optim import FlatOptimizer


class FlatGradScaler:
    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True, device="cuda"):
        self._enabled = bool(enabled)
        self._device = torch.device(device)
        if not self._enabled:
            return
        if not growth_factor > 1.0:
            raise ValueError("The growth factor must be > 1.0.")
        if not backoff_factor < 1.0:
            raise ValueError("The backoff factor must be < 1.0.")
        if int(growth_interval) < 1:
            raise ValueError("The growth interval must be >= 1.")
        self._growth_factor, self._backoff_factor, self._growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        # dwg_scaler_state: {float scale, int32 growth_tracker, float found_inf, int32 reserved}, one 16-byte block; the members are views
        self._state = torch.zeros(4, dtype=torch.int32, device=self._device)
        self._scale = self._state[0:1].view(torch.float32).reshape(())
        self._growth_tracker = self._state[1:2].reshape(())
        self._found_inf = self._state[2:3].view(torch.float32).reshape(())
        self._scale.fill_(float(init_scale))

    # -- what the guidance's gradient hooks and the loop read ---------------------------------------------------------------------------
    def is_enabled(self):
        return self._enabled

    def _get_scale_async(self):
        """The scale as a 0-dim fp32 device tensor: a view of the state, so it follows update() without a host read."""
        return self._scale if self._enabled else None

    def get_scale(self):
        """The scale as a Python float (a host read; the step does not use it)."""
        return float(self._scale) if self._enabled else 1.0

    def _get_growth_tracker(self):
        return int(self._growth_tracker) if self._enabled else 0

    def state_ptr(self):
        return ctypes.cast(self._state.data_ptr(), ctypes.POINTER(_lib.ScalerStateC))        # a device address: never dereferenced here

    # -- the loop ------------------------------------------------------------------------------------------------------------------------
    def scale(self, loss):
        """loss * scale (one device multiply); the loss itself when disabled."""
        if not self._enabled:
            return loss
        return loss * self._scale

    def unscale_(self, optimizer):
        raise NotImplementedError("FlatGradScaler.unscale_: the flat gradient is unscaled inside the fused Adam launch (it stays scaled in "
                                  "the buffer); clip or inspect gradients with the scale from _get_scale_async() instead")

    def step(self, optimizer, *args, **kwargs):
        """scan -> prepare -> scaled Adam on the optimizer's stream position, no host read (FlatOptimizer.step_scaled)."""
        if not isinstance(optimizer, FlatOptimizer):
            raise TypeError("FlatGradScaler.step needs an optim.FlatOptimizer (the flat fused Adam), got %s" % type(optimizer).__name__)
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        return optimizer.step_scaled(self, *args, **kwargs)

    def update(self, new_scale=None):
        """torch._amp_update_scale_ on the device state (found_inf is cleared for the next step); `new_scale` sets the scale instead."""
        if not self._enabled:
            return
        if new_scale is not None:
            if isinstance(new_scale, torch.Tensor):
                self._scale.copy_(new_scale.reshape(()))
            else:
                self._scale.fill_(float(new_scale))
            self._found_inf.zero_()
            return
        st = _lib.stream(self._device)
        _lib.check(_lib.lib().dwg_scaler_update(self.state_ptr(), self._growth_factor, self._backoff_factor, self._growth_interval, st),
                   "dwg_scaler_update")

    # -- checkpoints: torch.amp.GradScaler's keys -------------------------------------------------------------------------------------
    def state_dict(self):
        if not self._enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._scale.fill_(float(state_dict["scale"]))
        self._growth_tracker.fill_(int(state_dict["_growth_tracker"]))
        self._found_inf.zero_()
