"""AdamW over the flat gradient arena as ONE call into libofx_hip.so (ofx_adamw_step, outfitx_amd/csrc/optim.hip): gradient-norm
clipping, the AdamW update of every parameter and the zeroing of the gradient, two launches instead of torch's
vector_norm -> mul_ -> multi-tensor AdamW -> zero_ (36 bytes per arena float instead of 44; 52 with the mean over ranks, which
`grad_scale` folds in).

`FlatAdamW` is a torch.optim.Optimizer, so OneCycleLR drives its lr and beta1 and the optimizer-step hooks fire; its state_dict has
torch.optim.AdamW's layout in both directions.  A step whose gradient norm is not finite is skipped on the device: the gradient is zeroed,
parameters, moments and the step count stay as they were, and `skipped` reads 1.  There is no CPU path.

`FlatAdamW(loss_scaling=True)` adds torch.amp.GradScaler's dynamic loss scale for f16 training, state machine included, to that same
call (ofx_adamw_step_scaled): multiply the loss by the scale before the backward (`scale(loss)`), and step() unscales the arena, clips,
updates, zeroes and then backs the scale off after a skipped step or grows it after `growth_interval` good ones - all on the device,
still two launches, nothing read back.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import _lib as L
from . import engine


def segment_table(params: Sequence[torch.Tensor], offsets: Sequence[int]) -> torch.Tensor:
    """int64 [n, 3] HOST rows (param data_ptr, arena offset, numel), sorted by offset: the layout of ofx_opt_segment."""
    rows = sorted((int(o), int(p.data_ptr()), int(p.numel())) for p, o in zip(params, offsets))
    return torch.tensor([[ptr, o, n] for o, ptr, n in rows], dtype=torch.int64).reshape(-1, 3)


class FlatAdamW(torch.optim.Optimizer):
    """clip_grad_norm_(max_norm) + torch.optim.AdamW(lr, betas, eps, weight_decay) + zeroing over `flat_grads` (trainer.FlatGrads), one
    ofx_adamw_step per step().  Owns the two moment arenas (`exp_avg`, `exp_avg_sq`: the arena's layout, padding zero), the device step
    count `step_t`, the device segment table, the workspace, and the outputs of the last step: `grad_norm` (0-d fp32, the norm BEFORE
    clipping) and `skipped` (0-d int32).  `grad_scale` (default 1.0) multiplies the gradient before the norm is taken.

    step() reads lr and betas from param_groups[0] on every call (OneCycleLR cycles both), launches on the current stream and never
    synchronises; it also leaves the gradient arena zero, so no zero_grad() is needed after it.

    loss_scaling=True (off by default; the four arguments after it are torch.amp.GradScaler()'s defaults, which the reference's trainers
    construct): the arena is taken to hold `loss_scale` x the gradient - `scale(loss).backward()` puts it there - and step() is one
    ofx_adamw_step_scaled call: unscale, norm (`grad_norm` is the UNSCALED norm), clip, AdamW, zero, and the scaler's update of the device
    tensors `loss_scale` (0-d fp32) and `growth_tracker` (0-d int32).  state_dict() then carries "scale" and "growth_tracker" beside
    torch's keys; load_state_dict() takes them when they are there and keeps the current ones when they are not."""

    def __init__(self, flat_grads, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
                 max_norm: float = 1.0, loss_scaling: bool = False, init_scale: float = 65536.0, growth_factor: float = 2.0,
                 backoff_factor: float = 0.5, growth_interval: int = 2000):
        flat = flat_grads.flat
        if flat.device.type != "cuda":
            raise L.OfxError("FlatAdamW needs the gradient arena on a HIP device; there is no CPU path")
        for i, p in enumerate(flat_grads.params):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.data_ptr() % 16 or p.device != flat.device:
                raise ValueError(f"FlatAdamW: parameter {i} {tuple(p.shape)} must be fp32, contiguous, 16-byte aligned and on {flat.device}")
        if not 1 <= len(flat_grads.params) <= 1024:
            raise ValueError(f"FlatAdamW: {len(flat_grads.params)} parameters; ofx_adamw_step takes 1 to 1024 segments")
        if loss_scaling and not (init_scale > 0.0 and growth_factor >= 1.0 and 0.0 < backoff_factor <= 1.0 and growth_interval >= 1):
            raise ValueError(f"FlatAdamW: loss scaling needs init_scale > 0, growth_factor >= 1, 0 < backoff_factor <= 1 and growth_interval >= 1; "
                             f"got {init_scale}, {growth_factor}, {backoff_factor}, {growth_interval}")
        # torch.optim.AdamW's own defaults, taken from the installed torch on purpose: the param_groups keys of a state_dict are then
        # exactly the ones its load_state_dict / step expect, whichever keys that version has (foreach, fused, capturable, ...)
        defaults = dict(torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        self.flat_grads = flat_grads
        self.max_norm = float(max_norm)
        self.grad_scale = 1.0
        dev = flat.device
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.step_t = torch.zeros((), dtype=torch.float32, device=dev)
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self.skipped = torch.zeros((), dtype=torch.int32, device=dev)
        self.loss_scaling = bool(loss_scaling)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        if self.loss_scaling:
            self.loss_scale = torch.full((), float(init_scale), dtype=torch.float32, device=dev)
            self.growth_tracker = torch.zeros((), dtype=torch.int32, device=dev)
        self.ws = torch.empty(max(engine.adamw_step_ws_bytes(flat.numel()), 16), dtype=torch.uint8, device=dev)
        self._ptrs = [p.data_ptr() for p in flat_grads.params]
        self.segments = segment_table(flat_grads.params, flat_grads.offsets).to(dev)
        super().__init__(flat_grads.params, defaults)
        for p, o in zip(flat_grads.params, flat_grads.offsets):         # torch's state layout, as views of the arenas
            self.state[p] = {"step": torch.zeros((), dtype=torch.float32), "exp_avg": self.exp_avg[o:o + p.numel()].view_as(p),
                             "exp_avg_sq": self.exp_avg_sq[o:o + p.numel()].view_as(p)}

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("FlatAdamW has one param group: the parameters of its gradient arena")
        super().add_param_group(param_group)

    def _refresh_segments(self) -> None:
        """A parameter whose storage moved (p.data = ..., module.to()) gets its new address into the table, in place.  The rebuild is a
        blocking host-to-device copy: fine in eager mode, not inside a stream capture - capture only while the parameters stay put."""
        ptrs = [p.data_ptr() for p in self.flat_grads.params]
        if ptrs != self._ptrs:
            if any(q % 16 for q in ptrs):
                raise ValueError("FlatAdamW: a parameter moved to storage that is not 16-byte aligned")
            self.segments.copy_(segment_table(self.flat_grads.params, self.flat_grads.offsets))
            self._ptrs = ptrs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FlatAdamW: amsgrad / maximize are not implemented")
        self._refresh_segments()
        b1, b2 = g["betas"]
        if self.loss_scaling:
            engine.adamw_step_scaled(self.segments, self.flat_grads.flat, self.exp_avg, self.exp_avg_sq, self.step_t, float(g["lr"]), float(b1),
                                     float(b2), float(g["eps"]), float(g["weight_decay"]), self.max_norm, self.grad_scale, self.loss_scale,
                                     self.growth_tracker, self.growth_factor, self.backoff_factor, self.growth_interval, self.grad_norm,
                                     self.skipped, self.ws)
            return loss
        engine.adamw_step(self.segments, self.flat_grads.flat, self.exp_avg, self.exp_avg_sq, self.step_t, float(g["lr"]), float(b1), float(b2),
                          float(g["eps"]), float(g["weight_decay"]), self.max_norm, self.grad_scale, self.grad_norm, self.skipped, self.ws)
        return loss

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """GradScaler.scale: loss x the current scale, a device multiply (nothing is read back).  Needs loss_scaling=True."""
        if not self.loss_scaling:
            raise ValueError("FlatAdamW.scale: this optimizer was built with loss_scaling=False")
        return loss * self.loss_scale

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Zero the arena and keep every p.grad a view of it (step() already leaves it zero)."""
        self.flat_grads.zero_()

    def state_dict(self):
        """torch.optim.AdamW's layout: per-parameter step / exp_avg / exp_avg_sq and its param_groups keys.  Reads the step count back."""
        t = self.step_t.detach().cpu()
        for p in self.flat_grads.params:
            self.state[p]["step"] = t.clone()
        sd = super().state_dict()
        if self.loss_scaling:                                           # GradScaler.state_dict()'s names for the two
            sd["scale"], sd["growth_tracker"] = float(self.loss_scale), int(self.growth_tracker)
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """From a torch.optim.AdamW (or FlatAdamW) state_dict over the same parameters in the same order.  Copies INTO the arenas; the
        `step` values of the parameters that have state must all be equal (one step count serves the arena), else ValueError; a
        parameter without a state entry gets zero moments.  Optimizer's load_state_dict pre / post hooks are not run: the base
        implementation they belong to would replace the state tensors instead of filling the arenas."""
        groups, state = state_dict["param_groups"], state_dict["state"]
        n = len(self.flat_grads.params)
        if len(groups) != 1 or len(groups[0]["params"]) != n:
            raise ValueError(f"FlatAdamW.load_state_dict: expected one param group of {n} parameters")
        ids = list(groups[0]["params"])
        # torch.optim.AdamW creates a parameter's state at its first gradient: tensors that never had one (off the task's path in the
        # reference's checkpoints) have no entry.  They take zero moments here and share the arena's one step count.
        steps = {float(state[i]["step"]) for i in ids if i in state}
        if len(steps) > 1:
            raise ValueError(f"FlatAdamW.load_state_dict: per-parameter step values differ ({sorted(steps)}); the arena has one step count")
        for i, p in zip(ids, self.flat_grads.params):
            for key in ("exp_avg", "exp_avg_sq"):
                if i in state and tuple(state[i][key].shape) != tuple(p.shape):
                    raise ValueError(f"FlatAdamW.load_state_dict: {key} of parameter {i} is {tuple(state[i][key].shape)}, not {tuple(p.shape)}")
        for i, p in zip(ids, self.flat_grads.params):
            for key in ("exp_avg", "exp_avg_sq"):
                if i in state:
                    self.state[p][key].copy_(state[i][key])
                else:
                    self.state[p][key].zero_()
        self.step_t.fill_(steps.pop() if steps else 0.0)
        self.param_groups[0].update({k: v for k, v in groups[0].items() if k != "params"})
        if self.loss_scaling and "scale" in state_dict:                 # a state_dict from before loss scaling (or torch's own) has neither
            self.loss_scale.fill_(float(state_dict["scale"]))
            self.growth_tracker.fill_(int(state_dict.get("growth_tracker", 0)))
