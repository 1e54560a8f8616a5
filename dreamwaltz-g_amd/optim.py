"""Optimizers of the SDS step behind the reference's seam.

The reference builds a dict of named optimizers (`avatar.get_optimizer(cfg)`, /root/reference/core/system/avatar.py:1590-1635):
  'avatar'     GaussianOptimizer (core/gaussian/gaussian_optimizer.py:49-141): Adam(lr=0, eps=1e-15) with groups positions / scales /
               quaternions and `update_learning_rate(spatial_scale, iteration)` (exponential position schedule x spatial_scale,
               scaling_lr x spatial_scale)
  'lbs'        torch.optim.Adam (default eps 1e-8) over _lbs_weights / _betas when learned
  'nerf'       Adam(betas=(0.9, 0.99), eps=1e-15): encoder lr 10 x nerf.lr, both MLPs nerf.lr
  'mesh_<part>' Adam(lr=0, eps=1e-15): bary_coords (position_lr_init), scales (scaling_lr)
and the trainer loops `optimizer.zero_grad()`, `optimizer.update_learning_rate(...)` (when present), `scaler.step(optimizer)` over
them (core/trainer.py:861-890).  Here every one of those objects is a VIEW of one flat fp32 parameter buffer with flat gradient /
first-moment / second-moment buffers next to it: the multi-view step all-reduces ONE tensor over RCCL, and each view's `step()` is
a fused Adam launch per learning-rate group (csrc/adam.hip k_adam through include/dwg_elementwise.h).

The stage-II learned MLP background brings its own optimizer, `MLPBackground.get_optimizer()` (core/system/background.py:86-89): Adan
(core/optim/adan.py).  Here that is FlatAdan (boundary B23): flat buffers of its own and three launches a step (csrc/adan.hip through
include/dwg_adan.h), with the clipping factor and the step counts kept on the device.
"""
import ctypes
import math
import struct
from typing import Dict, List, Optional

import torch

from . import _lib


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """Log-linear learning-rate decay with an optional eased-in start: mirror of core/optim/optim_utils.py:4-38 (host-side
    float arithmetic; pinned against the reference's own function by tests/test_oracle_golden.py)."""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        else:
            delay_rate = 1.0
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay_rate * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return helper


class AdamSpec:
    """What one of the reference's optimizers is made of: param groups (+ Adam hyper-parameters); `gaussian` = the
    OptimizationParams of a GaussianOptimizer (adds update_learning_rate)."""

    def __init__(self, groups: List[dict], betas=(0.9, 0.999), eps=1e-8, gaussian: Optional[dict] = None):
        self.groups, self.betas, self.eps, self.gaussian = groups, betas, eps, gaussian


class FlatBuffers:
    """ONE flat fp32 buffer each for parameters, gradients and the two Adam moments (16-byte aligned slices).  The nn.Parameters
    are re-homed into the flat buffers (`.data` and `.grad` become views).

    Participation: with `.grad` always defined (a view of the flat gradient buffer) an optimizer cannot tell a parameter that took no part
    in this step's backward from one whose gradient is zero -- torch.optim.Adam can (`grad is None` after `zero_grad()`: the parameter, its
    moments and its step count stay as they are; gaussian_optimizer.py:93, trainer.py:861-890).  Every parameter therefore carries a
    post-accumulate hook that records that autograd wrote its slice this step (`touch` for kernels that add into the slice themselves: the
    grid table's in-place gradient), and FlatOptimizer.step() leaves un-touched groups alone.  Callers that fill the flat gradient by hand
    (no backward ran: nothing was recorded) get the plain "step everything" behaviour."""

    def __init__(self, params: List[torch.nn.Parameter], device):
        total, self.slices = 0, []
        for p in params:
            self.slices.append((total, p.numel()))
            total += (p.numel() + 3) // 4 * 4
        self.flat = torch.zeros(total, device=device)
        self.grad = torch.zeros(total, device=device)
        self.m = torch.zeros(total, device=device)
        self.v = torch.zeros(total, device=device)
        self.tracking = False           # some backward has recorded participation since the last zero_grad
        self._hooks = []
        for p, (off, n) in zip(params, self.slices):
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view_as(p.data)
            p.grad = self.grad[off:off + n].view_as(p.data)
            p._dwg_flat = self          # "my .grad is a slice of a flat gradient buffer": what lets a kernel add into it in place
            p._dwg_off = off            # ... namely the one that starts at element `off` (checked by `owns_grad` before any in-place add)
            p._dwg_touched = False
            if p.requires_grad:
                self._hooks.append(p.register_post_accumulate_grad_hook(self.touch))
        self.total = total

    def touch(self, p):
        p._dwg_touched = True
        self.tracking = True

    def owns_grad(self, p) -> bool:
        """True iff a kernel may ADD p's gradient into `p.grad` and report participation through `touch` instead of returning it to autograd:
        p is a trainable leaf this object re-homed and `p.grad` still IS its slice of the flat gradient buffer (same address, shape, dtype) --
        not a tensor a user rebound since, which the fused Adam would never read.  Frozen parameters (requires_grad False) are refused:
        autograd would have dropped their gradient and the optimizer must not see one."""
        g = p.grad
        return (getattr(p, "_dwg_flat", None) is self and p.is_leaf and p.requires_grad and g is not None and g.dtype == torch.float32
                and g.is_contiguous() and g.shape == p.shape and g.data_ptr() == self.grad.data_ptr() + 4 * int(getattr(p, "_dwg_off", -1)))

    def release(self, params):
        """Detach from the parameters (the buffers are being replaced: resize_flat_params)."""
        for h in self._hooks:
            h.remove()
        self._hooks = []
        for p in params:
            if getattr(p, "_dwg_flat", None) is self:
                p._dwg_flat = None


# Bumped by everything that writes parameters behind autograd's back (the fused Adam launches write the flat buffer through a raw pointer:
# no tensor version counter moves): caches of parameter-derived values key on it (avatar.DreamWaltzG._frozen_key).
PARAM_EPOCH = [0]


def _group_slices(buf: FlatBuffers, pg):
    """(n, [param, grad, exp_avg, exp_avg_sq]): a param group's length and the addresses of its four slices of the flat buffers."""
    off = pg["start"] * 4
    return pg["end"] - pg["start"], [t.data_ptr() + off for t in (buf.flat, buf.grad, buf.m, buf.v)]


def _group_c(buf: FlatBuffers, pg, row: int):
    """The group as the grouped launches take it (dwg_adam_group), reading row `row` of the device hyper table."""
    n, ptrs = _group_slices(buf, pg)
    return _lib.AdamGroupC(*ptrs, n, float(pg["betas"][0]), float(pg["betas"][1]), float(pg["eps"]), row)


class FlatOptimizer:
    """One of the named optimizers, as a view [start, end) of the flat buffers: same surface the trainer uses on the reference's
    objects (param_groups, zero_grad, step, state_dict / load_state_dict, and update_learning_rate for 'avatar')."""

    def __init__(self, name, buf: FlatBuffers, spec: AdamSpec, ranges):
        self.name, self.buf, self.spec = name, buf, spec
        self.param_groups = []
        for g, (start, end) in zip(spec.groups, ranges):
            pg = dict(g)
            pg.update(betas=g.get('betas', spec.betas), eps=g.get('eps', spec.eps), start=start, end=end)
            self.param_groups.append(pg)
        self.start = min(r[0] for r in ranges)
        self.end = max(r[1] for r in ranges)
        self.t = 0
        self.current_iteration = 0
        self.grad_scale = 1.0        # 1 / world size for the multi-view step (mean of the all-reduced sum)
        self._dev = None             # step_scaled's device block (step counts, learning rates, hyper rows, found, the scan's slots)
        self._dev_seeded = False     # the device step counts equal the host's pg["t"]
        self._dev_ahead = False      # the device step counts hold steps the host's pg["t"] lack (step_scaled ran since the last sync)
        if spec.gaussian is not None:
            ga = spec.gaussian
            self.num_iterations = ga["iterations"]
            self.default_scaling_lr = ga["scaling_lr"]
            self.position_sheduler_func = get_expon_lr_func(lr_init=ga["position_lr_init"], lr_final=ga["position_lr_final"],
                                                            lr_delay_mult=ga["position_lr_delay_mult"],
                                                            max_steps=ga["position_lr_max_steps"])
            self.update_learning_rate = self._update_learning_rate

    def _update_learning_rate(self, spatial_scale: float, iteration: Optional[int] = None):
        """GaussianOptimizer.update_learning_rate (gaussian_optimizer.py:130-141)."""
        if iteration is None:
            iteration = self.current_iteration
        lr = 0.
        for pg in self.param_groups:
            if pg.get('name') == "positions":
                lr = self.position_sheduler_func(iteration)
                pg['lr'] = lr * spatial_scale
            elif pg.get('name') == "scales":
                lr = self.default_scaling_lr
                pg['lr'] = lr * spatial_scale
        return lr

    def zero_grad(self, set_to_none: bool = False):
        self.buf.grad[self.start:self.end].zero_()
        self.buf.tracking = False
        for pg in self.param_groups:
            for p in pg.get('params', ()):
                p._dwg_touched = False

    def step(self, participation=None):
        """One Adam step of every param group.  Bias correction uses the group's OWN step count (torch.optim.Adam keeps one per parameter):
        a group that sat a step out -- its parameter was just replaced by the densifier, `grad is None` in the reference -- does not age.
        `participation`: one bool per group, decided by the caller (the multi-rank step agrees on it across the ranks, trainer._reduce_and_step)
        instead of this process's own record of which parameters its backward touched."""
        self._host_counts_move("step")
        self.t += 1
        self.current_iteration += 1
        PARAM_EPOCH[0] += 1
        for gi, pg in self._taking_part(participation):
            pg["t"] = pg.get("t", 0) + 1
            self._launch(pg)

    def _taking_part(self, participation=None):
        """Yields (group index, pg) of the groups this step updates, for step() and step_scaled().  Consumes `skip_once`."""
        for gi, pg in enumerate(self.param_groups):
            if pg.pop("skip_once", False):
                # the densifier just replaced this group's parameter: torch.optim.Adam finds `grad is None` on the new Parameter and leaves
                # it (and its moments) alone for this step (gaussian_densifier.py:141-161 + trainer.py:876-890)
                continue
            if pg["end"] <= pg["start"]:
                continue
            if participation is not None:
                if not participation[gi]:
                    continue
            elif self.buf.tracking and pg.get('params') and not any(getattr(p, "_dwg_touched", False) for p in pg['params']):
                # no parameter of this group took part in this step's backward: torch.optim.Adam sees `grad is None` and leaves the
                # parameter, both moments and the step count untouched (no drift on stale momentum, no ageing of the bias correction)
                continue
            yield gi, pg

    # -- the same step in two halves, for a captured graph of the whole avatar-side step (step_graph.GraphedTrainStep) ----------------
    def prepare_step(self, hyper_host: torch.Tensor, base: int):
        """HOST half of step(): step counts and this step's scalars of every group -> rows base, base + 1, ... of the (pinned) hyper table
        {lr / (1 - b1^t), sqrt(1 - b2^t), grad_scale, 0}.  Returns the number of rows used.  (Participation is not consulted: a captured
        step replays the same launches every time.)"""
        self._host_counts_move("prepare_step")
        self.t += 1
        self.current_iteration += 1
        PARAM_EPOCH[0] += 1
        for k, pg in enumerate(self.param_groups):
            pg["t"] = pg.get("t", 0) + 1
            # the statements of adam_hyper_row (csrc/adam_math.h), which dwg_adam_step uses: fp32 hyper-parameters, double arithmetic, one
            # rounding -- a replay of the captured step and an eager step then feed k_adam identical bits
            b1, b2, lr = (struct.unpack("f", struct.pack("f", float(x)))[0] for x in (pg["betas"][0], pg["betas"][1], pg["lr"]))
            hyper_host[base + k, 0] = lr / (1.0 - b1 ** pg["t"])
            hyper_host[base + k, 1] = math.sqrt(1.0 - b2 ** pg["t"])
            hyper_host[base + k, 2] = float(self.grad_scale)
        return len(self.param_groups)

    def launch_step(self, hyper_dev: torch.Tensor, base: int):
        """DEVICE half: one fused Adam launch per group reading its scalars from row base + k of the device hyper table (capturable)."""
        st = _lib.stream(self.buf.flat.device)
        for k, pg in enumerate(self.param_groups):
            n, ptrs = _group_slices(self.buf, pg)
            if n <= 0:
                continue
            _lib.check(_lib.lib().dwg_adam_step_dev(n, *ptrs, ctypes.c_void_p(hyper_dev.data_ptr() + (base + k) * 16), float(pg["betas"][0]),
                                                    float(pg["betas"][1]), float(pg["eps"]), st), "dwg_adam_step_dev")
        return len(self.param_groups)

    # -- the step under a loss scaler (grad_scaler.FlatGradScaler.step): every decision that depends on the gradient's values is the device's -----
    def _host_counts_move(self, what):
        """step() / prepare_step() count steps in pg["t"] on the host; step_scaled() counts them on the device.  Going from the device's
        counts back to the host's needs a sync (state_dict() reads them back, load_state_dict() uploads): without one it is an error."""
        if self._dev_ahead:
            raise RuntimeError("FlatOptimizer %r: %s() after step_scaled() without a sync -- the per-group step counts live on the device "
                               "once a loss scaler steps this optimizer; state_dict() reads them back" % (self.name, what))
        self._dev_seeded = False

    def _device_state(self):
        """The device block of step_scaled, created on first use; the step counts are seeded from the host's pg["t"] whenever those moved."""
        dev = self.buf.flat.device
        if self._dev is None:
            self._dev = {"steps": torch.zeros(_lib.ADAM_MAX_GROUPS, dtype=torch.int32, device=dev),
                         "lr": torch.zeros(_lib.ADAM_MAX_GROUPS, device=dev), "lr_host": None,
                         "hyper": torch.zeros(_lib.ADAM_MAX_GROUPS, 4, device=dev), "found": torch.zeros(1, device=dev),
                         "slots": torch.zeros(_lib.SCALER_MAX_SLOTS, dtype=torch.int32, device=dev)}
        d = self._dev
        if not self._dev_seeded:
            t = [int(pg.get("t", 0)) for pg in self.param_groups]
            d["steps"].copy_(torch.tensor(t + [0] * (_lib.ADAM_MAX_GROUPS - len(t)), dtype=torch.int32))
            self._dev_seeded = True
        lr = [float(pg["lr"]) for pg in self.param_groups]
        if lr != d["lr_host"]:                                               # a changed learning rate is an upload, not a rebuild
            d["lr"].copy_(torch.tensor(lr + [0.0] * (_lib.ADAM_MAX_GROUPS - len(lr)), dtype=torch.float32))
            d["lr_host"] = lr
        return d

    def device_step_counts(self):
        """The per-group step counts as step_scaled keeps them (a host read), None before its first use."""
        return None if self._dev is None or not self._dev_seeded else self._dev["steps"][:len(self.param_groups)].tolist()

    def step_scaled(self, scaler, participation=None):
        """step() under grad_scaler.FlatGradScaler, with no host read: scan this optimizer's gradient range for Inf / NaN, decide on the
        device (dwg_scaler_prepare: found, the groups' step counts, their scalars with grad_scale / scale as the gradient factor, or the
        skip flag), then one fused Adam launch over the participating groups that returns at once on the skip flag.  WHICH groups take part
        is decided here as step() decides it (skip_once, empty groups, the touched-parameters record); WHETHER the step happens is the
        device's.  pg["t"] is not touched: the device counts are authoritative until state_dict() / load_state_dict() sync them.  The flat
        gradient stays scaled."""
        if len(self.param_groups) > _lib.ADAM_MAX_GROUPS:
            raise RuntimeError("step_scaled covers at most %d param groups per optimizer, got %d" % (_lib.ADAM_MAX_GROUPS, len(self.param_groups)))
        self.t += 1
        self.current_iteration += 1
        PARAM_EPOCH[0] += 1
        if self.end <= self.start:
            return
        b = self.buf
        mask, groups = 0, []
        for gi, pg in self._taking_part(participation):
            mask |= 1 << gi
            groups.append(_group_c(b, pg, gi))
        d = self._device_state()
        L = _lib.lib()
        st = _lib.stream(b.flat.device)
        n = self.end - self.start
        _lib.check(L.dwg_grads_nonfinite(n, ctypes.c_void_p(b.grad.data_ptr() + 4 * self.start), _lib.ptr(d["slots"]), st), "dwg_grads_nonfinite")
        G = len(self.param_groups)
        b1 = (ctypes.c_float * G)(*[float(pg["betas"][0]) for pg in self.param_groups])
        b2 = (ctypes.c_float * G)(*[float(pg["betas"][1]) for pg in self.param_groups])
        _lib.check(L.dwg_scaler_prepare(L.dwg_grads_nonfinite_slots(n), _lib.ptr(d["slots"]), scaler.state_ptr(), _lib.ptr(d["found"]), G, mask,
                                        _lib.ptr(d["lr"]), ctypes.cast(b1, ctypes.c_void_p), ctypes.cast(b2, ctypes.c_void_p),
                                        float(self.grad_scale), _lib.ptr(d["steps"]), _lib.ptr(d["hyper"]), st), "dwg_scaler_prepare")
        self._dev_ahead = True
        if groups:
            arr = (_lib.AdamGroupC * len(groups))(*groups)
            _lib.check(L.dwg_adam_step_groups_scaled_dev(len(groups), arr, _lib.ptr(d["hyper"]), st),
                       "dwg_adam_step_groups_scaled_dev")

    def _launch(self, pg):
        """The fused Adam launch of one group over its slice of the flat buffers (csrc/adam.hip k_adam)."""
        n, ptrs = _group_slices(self.buf, pg)
        _lib.check(_lib.lib().dwg_adam_step(n, *ptrs, float(pg["lr"]), float(pg["betas"][0]), float(pg["betas"][1]), float(pg["eps"]),
                                            int(pg["t"]), float(self.grad_scale), _lib.stream(self.buf.flat.device)), "dwg_adam_step")

    def state_dict(self):
        """Same information a torch Adam state_dict carries, flat: step count, per-group hyper-parameters and the two moments.  After
        step_scaled the per-group step counts are read back from the device first (a host read: checkpoint time)."""
        if self._dev_ahead:
            for pg, t in zip(self.param_groups, self._dev["steps"].tolist()):
                pg["t"] = int(t)
            self._dev_ahead = False
        return {"t": self.t, "current_iteration": self.current_iteration,
                "param_groups": [{k: v for k, v in pg.items() if k != 'params'} for pg in self.param_groups],
                "exp_avg": self.buf.m[self.start:self.end].clone(), "exp_avg_sq": self.buf.v[self.start:self.end].clone()}

    def load_state_dict(self, sd):
        self.t, self.current_iteration = int(sd["t"]), int(sd.get("current_iteration", sd["t"]))
        for pg, s in zip(self.param_groups, sd["param_groups"]):
            pg["lr"] = s["lr"]
            pg["t"] = int(s.get("t", sd["t"]))
        self.buf.m[self.start:self.end].copy_(sd["exp_avg"]); self.buf.v[self.start:self.end].copy_(sd["exp_avg_sq"])
        self._dev_ahead, self._dev_seeded = False, False                     # the loaded counts are uploaded by the next step_scaled


class FlatOptimizerDict(dict):
    """The dict `avatar.get_optimizer(cfg)` returns; `.buffers` is the shared flat storage (all-reduce operand)."""
    buffers: FlatBuffers

    def all_grads(self):
        return self.buffers.grad

    def set_grad_scale(self, s: float):
        for o in self.values():
            o.grad_scale = s

    def launch_steps(self, hyper_dev: torch.Tensor):
        """DEVICE half of every named optimizer's step in ONE launch (dwg_adam_step_groups_dev): group k of the dict's k-th optimizer reads
        the row `FlatOptimizer.prepare_step` filled for it (rows are handed out in dict order, as step_graph does).  Falls back to one launch
        per group beyond DWG_ADAM_MAX_GROUPS groups."""
        b = self.buffers
        groups, base = [], 0
        for o in self.values():
            groups += [_group_c(b, pg, base + k) for k, pg in enumerate(o.param_groups) if pg["end"] > pg["start"]]
            base += len(o.param_groups)
        if len(groups) > _lib.ADAM_MAX_GROUPS:
            base = 0
            for o in self.values():
                base += o.launch_step(hyper_dev, base)
            return base
        arr = (_lib.AdamGroupC * max(len(groups), 1))(*groups)
        st = _lib.stream(b.flat.device)
        _lib.check(_lib.lib().dwg_adam_step_groups_dev(len(groups), arr, ctypes.c_void_p(hyper_dev.data_ptr()), st),
                   "dwg_adam_step_groups_dev")
        return base

    def zero_grad(self):
        """`zero_grad()` of every named optimizer with ONE fill: their gradient ranges are disjoint pieces of the one flat buffer."""
        self.buffers.grad.zero_()
        self.buffers.tracking = False
        for p in self.params:
            p._dwg_touched = False


def _group_ranges(specs: Dict[str, AdamSpec], buf: FlatBuffers) -> Dict[str, list]:
    """[start, end) of every param group inside the flat buffers (16-byte aligned ends), in the order the parameters were laid out."""
    i, out = 0, {}
    for name, spec in specs.items():
        ranges = []
        for g in spec.groups:
            if not g['params']:
                ranges.append((buf.slices[i][0] if i < len(buf.slices) else buf.total,) * 2)       # an empty group owns nothing
                continue
            start = buf.slices[i][0]
            for _ in g['params']:
                off, n = buf.slices[i]
                i += 1
            ranges.append((start, (off + n + 3) // 4 * 4))
        out[name] = ranges
    return out


def build_flat_optimizers(specs: Dict[str, AdamSpec], device) -> FlatOptimizerDict:
    params = [p for spec in specs.values() for g in spec.groups for p in g['params']]
    buf = FlatBuffers(params, device)
    out = FlatOptimizerDict()
    out.buffers, out.specs, out.params = buf, specs, params
    for name, ranges in _group_ranges(specs, buf).items():
        out[name] = FlatOptimizer(name, buf, specs[name], ranges)
        out[name].owner = out                    # the dict this named optimizer is a view of (densifier: the buffers resize as a whole)
    return out


def resize_flat_params(opts: FlatOptimizerDict, new_values: Dict[torch.nn.Parameter, tuple]) -> Dict[torch.nn.Parameter, torch.nn.Parameter]:
    """Densification / pruning (gaussian_densifier.py:120-180): some parameters change their first dimension.  `new_values` maps a Parameter
    to (data, exp_avg, exp_avg_sq) of its new shape (moments None = zeros).  The flat parameter / gradient / moment buffers are laid out
    afresh: the untouched Parameters keep their identity and are re-homed (`.data` / `.grad` become views of the new buffers, moments
    carried over); a RESIZED parameter becomes a NEW nn.Parameter object, as in the reference (:131,156) -- a leaf whose `.data` changed
    shape keeps a stale gradient accumulator for as long as anybody holds an output of an earlier step.  Returns {old: new} for the
    resized ones (the caller re-binds its attributes); every named optimizer gets its new ranges.  The all-reduce operand of the
    multi-view step is the new `opts.buffers.grad`."""
    old = opts.buffers
    keep, renamed = {}, {}
    for p, (off, n) in zip(opts.params, old.slices):
        if p in new_values:
            data, m, v = new_values[p]
            data = data.detach().float().clone()
            q = torch.nn.Parameter(data, requires_grad=p.requires_grad)
            renamed[p] = q
            keep[q] = (data, torch.zeros_like(data) if m is None else m.detach().float(), torch.zeros_like(data) if v is None else v.detach().float(), None)
        else:
            keep[p] = (p.data.clone(), old.m[off:off + n].clone(), old.v[off:off + n].clone(), old.grad[off:off + n].clone())
    opts.params = [renamed.get(p, p) for p in opts.params]
    for spec in opts.specs.values():
        for g in spec.groups:
            g['params'] = [renamed.get(p, p) for p in g['params']]
    for o in opts.values():
        for pg in o.param_groups:
            if 'params' in pg:
                pg['params'] = [renamed.get(p, p) for p in pg['params']]
    old.release(list(keep.keys()))
    for p in opts.params:
        p.data = keep[p][0]
        p.grad = None
    touched = {p: bool(getattr(p, "_dwg_touched", False)) for p in opts.params}      # this step's participation survives the re-homing
    buf = FlatBuffers(opts.params, old.flat.device)
    buf.tracking = old.tracking
    for p in opts.params:
        p._dwg_touched = touched[p]
    for p, (off, n) in zip(opts.params, buf.slices):
        buf.m[off:off + n].copy_(keep[p][1].reshape(-1)); buf.v[off:off + n].copy_(keep[p][2].reshape(-1))
        if keep[p][3] is not None:
            buf.grad[off:off + n].copy_(keep[p][3])
    opts.buffers = buf
    resized = set(renamed.values())
    for name, ranges in _group_ranges(opts.specs, buf).items():
        o = opts[name]
        o.buf = buf
        for pg, g, (start, end) in zip(o.param_groups, o.spec.groups, ranges):
            pg["start"], pg["end"] = start, end
            if any(p in resized for p in g['params']):
                pg["skip_once"] = True
        o.start = min(r[0] for r in ranges)
        o.end = max(r[1] for r in ranges)
    return renamed


# ----------------------------------------------------------------------------------------------------------------------------------------
# Adan (boundary B23): the optimizer of the stage-II learned MLP background, fused on flat buffers of its own
# ----------------------------------------------------------------------------------------------------------------------------------------
class AdanSpec:
    """What the reference's Adan (core/optim/adan.py:47-78) is made of: param groups (each may override lr, betas, eps, weight_decay and
    no_prox) and the optimizer-wide max_grad_norm (0: no clipping)."""

    def __init__(self, groups: List[dict], lr=1e-3, betas=(0.98, 0.92, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, no_prox=False):
        if not 0.0 <= max_grad_norm:
            raise ValueError('Invalid Max grad norm: {}'.format(max_grad_norm))
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: {}'.format(lr))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: {}'.format(eps))
        for i in range(3):
            if not 0.0 <= betas[i] < 1.0:
                raise ValueError('Invalid beta parameter at index {}: {}'.format(i, betas[i]))
        self.groups, self.lr, self.betas, self.eps, self.weight_decay = groups, lr, tuple(betas), eps, weight_decay
        self.max_grad_norm, self.no_prox = float(max_grad_norm), bool(no_prox)


class FlatAdan:
    """The reference's Adan on flat fp32 buffers it OWNS: parameters, gradient (FlatBuffers: 16-byte aligned slices, the Parameters re-homed
    so that `.data` / `.grad` are views, a post-accumulate hook recording participation) and the four state buffers exp_avg, exp_avg_sq,
    exp_avg_diff and neg_pre_grad (minus the previous clipped gradient, the reference's sign).  A step is three launches
    (include/dwg_adan.h) and no host read: the sum of squares of the whole gradient, the one-workgroup preparation (clipping factor over
    ALL groups, every group's step count + 1 on the device, the groups' scalars), the update of the participating groups.  The surface is
    what the trainer and a disabled GradScaler use on the reference's object: param_groups, zero_grad, step, state_dict /
    load_state_dict, grad_scale.  The gradient buffer stays as autograd wrote it (the reference scales it in place by the clipping
    factor; nothing reads it before the next zero_grad)."""
    owns_buffers = True          # not a view of a FlatOptimizerDict's buffers: FlatOptimizerDict.zero_grad() does not reach it

    def __init__(self, spec: AdanSpec, device, name: str = "adan"):
        if not spec.groups or len(spec.groups) > _lib.CONSTANTS["DWG_ADAN_MAX_GROUPS"]:
            raise RuntimeError("FlatAdan takes 1..%d param groups, got %d" % (_lib.CONSTANTS["DWG_ADAN_MAX_GROUPS"], len(spec.groups)))
        self.name, self.spec = name, spec
        for g in spec.groups:
            g['params'] = list(g['params'])
        params = [p for g in spec.groups for p in g['params']]
        if any(p.dtype != torch.float32 for p in params):
            raise RuntimeError("FlatAdan steps fp32 parameters")
        self.buf = FlatBuffers(params, device)
        self.exp_avg_diff = torch.zeros(self.buf.total, device=device)
        self.neg_pre_grad = torch.zeros(self.buf.total, device=device)
        self.max_grad_norm = float(spec.max_grad_norm)
        self.param_groups = []
        for g, (start, end) in zip(spec.groups, _group_ranges({name: spec}, self.buf)[name]):
            pg = dict(g)
            pg.update(lr=g.get('lr', spec.lr), betas=tuple(g.get('betas', spec.betas)), eps=g.get('eps', spec.eps),
                      weight_decay=g.get('weight_decay', spec.weight_decay), no_prox=bool(g.get('no_prox', spec.no_prox)),
                      max_grad_norm=self.max_grad_norm, start=start, end=end, step=0, has_prev=False)
            self.param_groups.append(pg)
        G = len(self.param_groups)
        self.grad_scale = 1.0
        self._steps = torch.zeros(G, dtype=torch.int32, device=device)                        # the groups' step counts: authoritative
        self._rows = torch.zeros(G, _lib.CONSTANTS["DWG_ADAN_ROW"], device=device)
        self._partials = torch.zeros(_lib.CONSTANTS["DWG_ADAN_MAX_SLOTS"], dtype=torch.float64, device=device)

    # FlatBuffers' two moment buffers under the reference's names (exp_avg_diff and neg_pre_grad are this object's own)
    exp_avg = property(lambda self: self.buf.m)
    exp_avg_sq = property(lambda self: self.buf.v)

    def zero_grad(self, set_to_none: bool = False):
        self.buf.grad.zero_()
        self.buf.tracking = False
        for pg in self.param_groups:
            for p in pg['params']:
                p._dwg_touched = False

    def participating(self, participation=None):
        """Indices of the groups this step updates, as FlatOptimizer.step decides it: an empty group never; `participation` (one bool per
        group) when the caller decides; else, once some backward recorded participation, the groups with a touched parameter; else all."""
        out = []
        for gi, pg in enumerate(self.param_groups):
            if pg["end"] <= pg["start"]:
                continue
            if participation is not None:
                if not participation[gi]:
                    continue
            elif self.buf.tracking and not any(getattr(p, "_dwg_touched", False) for p in pg['params']):
                continue
            out.append(gi)
        return out

    def step(self, participation=None):
        """One Adan step.  Every group ages (the reference counts a group's step whether or not any of its parameters had a gradient,
        adan.py:143-146); a group none of whose parameters took part is otherwise untouched."""
        took_part = self.participating(participation)
        PARAM_EPOCH[0] += 1
        b = self.buf
        if b.total == 0:
            return
        L = _lib.lib()
        st = _lib.stream(b.flat.device)
        nslots = 0
        if self.max_grad_norm > 0:
            nslots = int(L.dwg_adan_sumsq_slots(b.total))
            _lib.check(L.dwg_adan_sumsq(b.total, _lib.ptr(b.grad), _lib.ptr(self._partials), st), "dwg_adan_sumsq")
        G = len(self.param_groups)
        hyper = (_lib.STRUCTS["dwg_adan_hyper"] * G)()
        first_mask = 0
        for gi, pg in enumerate(self.param_groups):
            h = hyper[gi]
            h.lr, h.eps, h.weight_decay, h.no_prox = float(pg["lr"]), float(pg["eps"]), float(pg["weight_decay"]), int(bool(pg["no_prox"]))
            h.beta1, h.beta2, h.beta3 = (float(x) for x in pg["betas"])
            if not pg["has_prev"]:
                first_mask |= 1 << gi
        _lib.check(L.dwg_adan_prepare(nslots, _lib.ptr(self._partials) if nslots else None, G, hyper, first_mask, self.max_grad_norm,
                                      float(self.grad_scale), _lib.ptr(self._steps), _lib.ptr(self._rows), st), "dwg_adan_prepare")
        if not took_part:
            return
        groups = (_lib.STRUCTS["dwg_adan_group"] * len(took_part))()
        for k, gi in enumerate(took_part):
            pg = self.param_groups[gi]
            n, off = pg["end"] - pg["start"], pg["start"] * 4
            a = groups[k]
            a.param, a.grad, a.exp_avg, a.exp_avg_sq = b.flat.data_ptr() + off, b.grad.data_ptr() + off, b.m.data_ptr() + off, b.v.data_ptr() + off
            a.exp_avg_diff, a.neg_pre_grad = self.exp_avg_diff.data_ptr() + off, self.neg_pre_grad.data_ptr() + off
            a.n, a.hyper_row = n, gi
            pg["has_prev"] = True
        _lib.check(L.dwg_adan_step_groups_dev(len(took_part), groups, _lib.ptr(self._rows), st), "dwg_adan_step_groups_dev")

    def step_scaled(self, scaler, participation=None):
        raise NotImplementedError("FlatAdan.step_scaled: the Adan step under a loss scaler is not built (stage II never runs under optim.fp16)")

    def device_step_counts(self):
        """The per-group step counts (a host read)."""
        return [int(t) for t in self._steps.tolist()]

    def state_dict(self):
        """The reference's state, flat: per group its hyper-parameters and `step` (read back from the device here: checkpoint time), and
        the four state buffers under the reference's keys."""
        for pg, t in zip(self.param_groups, self.device_step_counts()):
            pg["step"] = t
        b = self.buf
        return {"max_grad_norm": self.max_grad_norm,
                "param_groups": [{k: v for k, v in pg.items() if k != 'params'} for pg in self.param_groups],
                "exp_avg": b.m.clone(), "exp_avg_sq": b.v.clone(), "exp_avg_diff": self.exp_avg_diff.clone(), "neg_pre_grad": self.neg_pre_grad.clone()}

    def load_state_dict(self, sd):
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("FlatAdan.load_state_dict: %d param groups in the state, %d here" % (len(sd["param_groups"]), len(self.param_groups)))
        self.max_grad_norm = float(sd.get("max_grad_norm", self.max_grad_norm))
        for pg, s in zip(self.param_groups, sd["param_groups"]):
            for k in ("lr", "betas", "eps", "weight_decay", "no_prox"):
                if k in s:
                    pg[k] = tuple(s[k]) if k == "betas" else s[k]
            pg["step"] = int(s.get("step", 0))
            pg["has_prev"] = bool(s.get("has_prev", pg["step"] > 0))
            pg["max_grad_norm"] = self.max_grad_norm
        b = self.buf
        for dst, key in ((b.m, "exp_avg"), (b.v, "exp_avg_sq"), (self.exp_avg_diff, "exp_avg_diff"), (self.neg_pre_grad, "neg_pre_grad")):
            dst.copy_(sd[key])
        self._steps.copy_(torch.tensor([pg["step"] for pg in self.param_groups], dtype=torch.int32))
