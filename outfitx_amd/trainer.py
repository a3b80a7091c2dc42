"""Data-parallel CP training loop over the HIP training step (BASELINE config 5).

Counterpart of the reference's `CompatibilityPredictionTrainer.train_epoch` step
(src/trains/trainers/compatibility_prediction_trainer.py:57-81) and its `build_metrics` all-gather (:372-405), written
for one process per GPU over RCCL/xGMI rather than DistributedDataParallel:

  forward (tape, bf16 operands) -> FocalLoss(.75, 2, mean) -> / accumulation_steps [-> x loss scale] -> backward (hand-written HIP)
  every `accumulation_steps` micro-batches:  ONE all-reduce of the flat gradient arena (mean over ranks)
                                             [-> unscale] -> clip_grad_norm_(1.0) -> AdamW(lr) [-> scaler update] -> OneCycleLR step -> zero
  The bracketed steps are torch.amp.GradScaler's (scale / unscale_ / step / update, what the reference wraps its step in), run with
  `loss_scaling=True` in the config: for f16 operands, whose backward keeps activation gradients in f16 and would lose the small ones.
  epoch end: all-gather logits / labels / loss -> AUC, accuracy, precision, recall, F1 (same formulas as :406-436).

Differences from DDP by design (MI355X / xGMI, point-to-point links, per-link bound rings):
  * gradients live in ONE contiguous fp32 arena (`FlatGrads`; every p.grad is a view): the clip norm is one reduction over the
    arena instead of 75 per-tensor norms, and the all-reduce goes out as one contiguous slice per encoder layer (34 MB each,
    6 + 1 collectives for the 205 MB) STARTED WHILE THE BACKWARD STILL RUNS: `ofx_train_arm_layer_events` makes the hand-written
    backward record a HIP event when layer l's gradients are final (layers finish last-to-first), and the slice's RCCL
    all-reduce is enqueued on a side stream behind that event - 5/6 of the reduction overlaps the backward of the layers below
    (xGMI is point-to-point: 34 MB slices are still bandwidth-, not latency-bound per link);
  * the all-reduce runs once per OPTIMIZER step; DDP without no_sync() (what the reference does) reduces on every
    micro-batch, 4x the traffic at accumulation_steps = 4;
  * no per-step all_gather_object / barrier pair (reference C4/C5): error propagation is the job of the
    launcher (torchrun tears the group down when a rank raises).

`CIRTrainer` is the same loop for the reference's other training job, complementary item retrieval
(src/trains/trainers/complementary_item_retrieval_trainer.py:66-116): model(CIR batch) -> SetWiseRankingLoss(margin 2; one fused kernel
pass on HIP tensors) -> / accumulation_steps -> the hand-written CIR backward, then the identical boundary step.  Both trainers share
`FlatGradTrainer` below (arena, gradient sink, per-layer slices, armed layer events, overlapped reduction, clip, AdamW, OneCycleLR).

Evaluation: `CPTrainer.valid_epoch` / `test_epoch` (compatibility_prediction_trainer.py:131-239), `CIRTrainer.valid_epoch` (loss + grouped
recall@k) and `FITBEvaluator` (fill_in_the_blank_trainer.py:37-64) run in eval mode without gradients, touch neither parameters nor
optimizer, scheduler or arena, and sum their metrics over the ranks.

The loop itself is device-agnostic torch host code (the CPU tests drive it with a stub module over gloo); the model it is
meant for, `outfitx_amd.OutfitX` in train() mode, only runs on a HIP device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch
import torch.distributed as dist


@dataclass
class CPTrainConfig:
    """Defaults = the reference's CompatibilityPredictionTrainConfig / BaseTrainConfig (src/trains/configs)."""
    learning_rate: float = 2e-5
    accumulation_steps: int = 4
    n_epochs: int = 200
    max_grad_norm: float = 1.0
    focal_alpha: float = 0.75
    focal_gamma: float = 2.0
    pct_start: float = 0.3
    div_factor: float = 25.0
    final_div_factor: float = 1e4
    fused_optimizer: bool = True      # torch.optim.AdamW(fused=True): one multi-tensor kernel per step
    hip_optimizer: bool = False       # optim.FlatAdamW: clip + AdamW + zero over the arena as one ofx_adamw_step call (HIP devices only)
    loss_scaling: bool = False        # torch.amp.GradScaler's dynamic loss scale around the step (the reference's trainers; for train_precision="f16")
    init_scale: float = 65536.0       # torch.amp.GradScaler()'s defaults, these four
    growth_factor: float = 2.0
    backoff_factor: float = 0.5
    growth_interval: int = 2000


@dataclass
class CIRTrainConfig:
    """Defaults = the reference's ComplementaryItemRetrievalTrainConfig (src/trains/configs/complementary_item_retrieval_train_config.py;
    its per-GPU batch is 3072 with 10 negatives per query) and the OneCycleLR settings of its trainer."""
    learning_rate: float = 2e-5
    accumulation_steps: int = 4
    n_epochs: int = 300
    max_grad_norm: float = 1.0
    margin: float = 2.0
    pct_start: float = 0.3
    div_factor: float = 25.0
    final_div_factor: float = 1e4
    fused_optimizer: bool = True
    hip_optimizer: bool = False       # as CPTrainConfig.hip_optimizer
    loss_scaling: bool = False        # as CPTrainConfig.loss_scaling, and the four below it
    init_scale: float = 65536.0
    growth_factor: float = 2.0
    backoff_factor: float = 0.5
    growth_interval: int = 2000


class FlatGrads:
    """One contiguous fp32 arena holding every trainable parameter's gradient; p.grad are views into it, so autograd
    accumulates in place and reductions / norms / zeroing are single kernels over the arena."""

    def __init__(self, params: Sequence[torch.nn.Parameter]):
        self.params = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + 63) // 64 * 64
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        for p, o in zip(self.params, self.offsets):
            p.grad = self.flat[o:o + p.numel()].view_as(p)

    def zero_(self):
        self.flat.zero_()
        for p, o in zip(self.params, self.offsets):      # re-attach views an optimizer's zero_grad(set_to_none=True) dropped
            if p.grad is None or p.grad.data_ptr() != self.flat.data_ptr() + 4 * o:
                p.grad = self.flat[o:o + p.numel()].view_as(p)

    def all_reduce_mean_(self, group=None):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group)
            self.flat.div_(dist.get_world_size(group))

    def slices(self, groups: Sequence[Sequence[torch.nn.Parameter]]):
        """groups: lists of parameters, each list contiguous in the arena (an encoder layer's 12 tensors) -> ([(lo, hi)] per group,
        [(lo, hi)] of everything not covered), in floats."""
        off = {id(p): (o, o + (p.numel() + 63) // 64 * 64) for p, o in zip(self.params, self.offsets)}
        out = []
        for g in groups:
            rs = sorted(off[id(p)] for p in g if id(p) in off)
            if not rs or any(a[1] != b[0] for a, b in zip(rs, rs[1:])):
                raise ValueError("a gradient bucket must be a contiguous run of the arena")
            out.append((rs[0][0], rs[-1][1]))
        rest, cur = [], 0
        for lo, hi in sorted(out):
            if lo > cur:
                rest.append((cur, lo))
            cur = max(cur, hi)
        if cur < self.flat.numel():
            rest.append((cur, self.flat.numel()))
        return out, rest

    def clip_norm_(self, max_norm: float) -> torch.Tensor:
        """torch.nn.utils.clip_grad_norm_ semantics (L2, eps 1e-6, coefficient clamped to 1); stays on the device."""
        total = torch.linalg.vector_norm(self.flat)
        self.flat.mul_(torch.clamp(max_norm / (total + 1e-6), max=1.0))
        return total


def cp_metrics(y_hats: torch.Tensor, labels: torch.Tensor) -> Dict[str, float]:
    """Accuracy / Precision / Recall / F1 / AUC of compatibility logits (cp_trainer:406-436).  AUC by the rank statistic
    (ties get the average rank) — what sklearn.metrics.roc_auc_score returns — without leaving torch."""
    probs = torch.sigmoid(y_hats.float()).detach().cpu().double()
    lab = labels.detach().cpu().int()
    n_pos, n_neg = int((lab == 1).sum()), int((lab == 0).sum())
    if n_pos and n_neg:
        order = torch.argsort(probs)
        sp = probs[order]
        ranks = torch.arange(1, len(sp) + 1, dtype=torch.float64)
        uniq, inv, cnt = torch.unique_consecutive(sp, return_inverse=True, return_counts=True)
        ends = torch.cumsum(cnt, 0).double()
        avg = ends - (cnt.double() - 1) / 2
        ranks = avg[inv]
        r = torch.empty_like(ranks); r[order] = ranks
        auc = float((r[lab == 1].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))
    else:
        auc = 0.0
    pred = (probs > 0.5).int()
    tp = int(((pred == 1) & (lab == 1)).sum()); fp = int(((pred == 1) & (lab == 0)).sum()); fn = int(((pred == 0) & (lab == 1)).sum())
    precision = tp / (tp + fp) if tp + fp else 0.0
    recall = tp / (tp + fn) if tp + fn else 0.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return {"Accuracy": float((pred == lab).float().mean()), "Precision": precision, "Recall": recall, "F1": f1, "AUC": auc}


def gather_epoch(local_y: torch.Tensor, local_labels: torch.Tensor, local_loss: torch.Tensor, batch_count: float, group=None):
    """cp_trainer:372-405: all-gather every rank's epoch logits / labels / summed loss -> global metrics on every rank.
    Ranks may hold different sample counts (the reference assumes equal ones): sizes are gathered first.
    'loss' = mean over the ranks of their summed losses / batch_count.  batch_count is the number of batches PER RANK: the reference
    passes len(dataloader), the same on every rank.  Where the ranks hold different counts, pass all ranks' batches / world size - it
    need not be whole (CPTrainer.valid_epoch does): the result is then the summed loss of all ranks / the number of all batches."""
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    if world > 1:
        n = torch.tensor([local_y.numel()], dtype=torch.int64, device=local_y.device)
        sizes = [torch.zeros_like(n) for _ in range(world)]
        dist.all_gather(sizes, n, group=group)
        mx = int(max(int(s) for s in sizes))
        def gat(t):
            pad = torch.zeros(mx, dtype=t.dtype, device=t.device); pad[: t.numel()] = t.reshape(-1)
            out = [torch.empty_like(pad) for _ in range(world)]
            dist.all_gather(out, pad, group=group)
            return torch.cat([o[: int(s)] for o, s in zip(out, sizes)])
        ys, ls = gat(local_y.detach().float()), gat(local_labels.detach().float())
        losses = [torch.empty_like(local_loss) for _ in range(world)]
        dist.all_gather(losses, local_loss.detach(), group=group)
        loss = torch.stack(losses).mean() / batch_count
    else:
        ys, ls, loss = local_y.detach().float(), local_labels.detach().float(), local_loss.detach() / batch_count
    return {"loss": float(loss), **cp_metrics(ys, ls)}


class FlatGradTrainer:
    """What the CP and the CIR loop share: the flat gradient arena, gradient-sink mode of the HIP model, per-layer gradient slices,
    the overlapped mean over the ranks, and the accumulation-boundary step ([unscale ->] clip -> AdamW [-> scaler update] -> OneCycleLR
    -> zero).  `cfg` carries learning_rate, accumulation_steps, n_epochs, max_grad_norm, pct_start, div_factor, final_div_factor,
    fused_optimizer, hip_optimizer, and loss_scaling with init_scale, growth_factor, backoff_factor, growth_interval.

    cfg.loss_scaling: the loss is multiplied by a dynamic scale before every backward and the boundary undoes it, as torch.amp.GradScaler
    does: a window whose gradient is not finite is skipped and multiplies the scale by backoff_factor, growth_interval windows in a row
    that are not multiply it by growth_factor.  With the torch optimizer the boundary IS a torch.amp.GradScaler (`self.scaler`: unscale_
    -> clip -> scaler.step -> scaler.update -> zero; scaler.step reads the found-inf flag back); with hip_optimizer the scale and its
    tracker are device tensors of FlatAdamW (`optimizer.loss_scale`, `optimizer.growth_tracker`), the whole boundary stays the one call
    and nothing is read back.  Losses are reported unscaled and `last_grad_norm` is the unscaled norm either way.  No collective is
    added: the ranks sum their arenas before the boundary, so every rank sees the same non-finite norm and the same scale.

    cfg.hip_optimizer: the optimizer is optim.FlatAdamW over the arena - norm, clip, AdamW and the zeroing are ONE ofx_adamw_step call
    (two launches), and the division by the world size rides in it as grad_scale.  `last_grad_norm` is then the kernel's norm tensor and
    `last_step_skipped` its flag (1: the norm was not finite, the gradient was dropped and parameters, moments and step count were left
    alone); both stay on the device.  The OneCycleLR schedule advances whether or not the step was skipped: the schedule counts
    accumulation windows, and finding out would cost a host synchronisation per step."""

    head = "cp"                   # the model head this trainer's backward runs through (outfit_x.HEAD_OFF_PATH): what sink_ready() is asked about

    def __init__(self, model: torch.nn.Module, steps_per_epoch: int, cfg, loss_fn: Callable,
                 params: Optional[Iterable[torch.nn.Parameter]] = None, group=None):
        self.model, self.cfg, self.group = model, cfg, group
        if hasattr(model, "_check_trainable_width"):
            model._check_trainable_width()          # a width that scores only (d_model 1536): refuse before anything is allocated
        c = self.cfg
        ps = list(params) if params is not None else self._default_params(model)
        self.grads = FlatGrads(ps)
        self.loss_fn = loss_fn
        dev = self.grads.flat.device
        fused = c.fused_optimizer and dev.type == "cuda"
        self.hip_optimizer = bool(getattr(c, "hip_optimizer", False))
        self.loss_scaling = bool(getattr(c, "loss_scaling", False))
        self.scaler = None                                   # loss_scaling with the torch optimizer: the torch.amp.GradScaler
        scaler_args = ({"init_scale": c.init_scale, "growth_factor": c.growth_factor, "backoff_factor": c.backoff_factor,
                        "growth_interval": c.growth_interval} if self.loss_scaling else {})
        if self.hip_optimizer:
            from .optim import FlatAdamW                     # raises on a CPU arena: no quiet fall-back to torch's AdamW
            self.optimizer = FlatAdamW(self.grads, lr=c.learning_rate, max_norm=c.max_grad_norm, loss_scaling=self.loss_scaling, **scaler_args)
        else:
            self.optimizer = torch.optim.AdamW(self.grads.params, lr=c.learning_rate, **({"fused": True} if fused else {}))
            if self.loss_scaling:
                self.scaler = torch.amp.GradScaler(dev.type, **scaler_args)
        self.scheduler = torch.optim.lr_scheduler.OneCycleLR(
            optimizer=self.optimizer, max_lr=c.learning_rate, epochs=c.n_epochs,
            steps_per_epoch=math.ceil(steps_per_epoch / c.accumulation_steps), pct_start=c.pct_start, anneal_strategy="cos",
            div_factor=c.div_factor, final_div_factor=c.final_div_factor)
        self.steps_per_epoch = steps_per_epoch
        self.last_grad_norm: Optional[torch.Tensor] = None
        self.last_step_skipped: Optional[torch.Tensor] = None       # hip_optimizer only: 0-d int32 on the device
        # outfitx_amd.OutfitX: let the backward kernels add straight into the arena views (no per-tensor accumulate kernels);
        # valid because nothing here relies on autograd hooks (DDP would)
        if hasattr(model, "sink_ready"):
            model.grad_sink = True
        # per-layer gradient slices for the overlapped reduction (None: the model has no encoder-layer structure -> one all-reduce)
        self.layer_slices = self.rest_slices = None
        layers = getattr(getattr(model, "transformer_encoder", None), "layers", None)
        if layers is not None:
            try:
                self.layer_slices, self.rest_slices = self.grads.slices([[p for p in l.parameters() if p.requires_grad] for l in layers])
            except ValueError:
                self.layer_slices = None
        self.overlap_reduce = True
        self._layer_events = None
        self._comm_stream = None

    @staticmethod
    def _default_params(model: torch.nn.Module) -> List[torch.nn.Parameter]:
        return [p for p in model.parameters() if p.requires_grad]

    def _world(self) -> int:
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def _inputs(self, batch: dict) -> dict:
        """batch['input_dict'] with every tensor on the arena's device (the task class passes through)."""
        dev = self.grads.flat.device
        return {k: (v if k == "task" else v.to(dev, non_blocking=True)) for k, v in batch["input_dict"].items()}

    def _rank_mean(self, total: torch.Tensor, n: int) -> float:
        """Summed micro-batch loss / number of batches, averaged over the ranks."""
        total = total / max(n, 1)
        if self._world() > 1:
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self.group)
            total = total / self._world()
        return float(total)

    def _arm_overlap(self) -> bool:
        """Before the backward of an accumulation window's LAST micro-batch: arm the per-layer completion events (HIP model only)."""
        if not (self.overlap_reduce and self.layer_slices and self._world() > 1 and hasattr(self.model, "arm_bwd_layer_events")
                and self.grads.flat.is_cuda):
            return False
        # the events mean "final in the arena" only on the gradient-sink path; any tensor whose .grad is not the arena view (detached,
        # non-contiguous, not fp32) sends the backward through autograd's accumulation, which runs AFTER the events: plain reduction then
        if hasattr(self.model, "sink_ready") and not self.model.sink_ready(self.head):
            return False
        if self._layer_events is None:
            self._layer_events = [torch.cuda.Event() for _ in self.layer_slices]
            for e in self._layer_events:
                e.record()                                   # materialises the HIP handle
            self._comm_stream = torch.cuda.Stream(self.grads.flat.device)
        self.model.arm_bwd_layer_events(self._layer_events)
        return True

    def _reduce_mean(self, overlapped: bool) -> None:
        """Mean of the gradient arena over the ranks.  overlapped: layer l's slice is reduced on the side stream as soon as its event
        fires (the backward of the layers below is still running on the main stream); else slice by slice after the backward (CPU /
        gloo, stub models) or as one collective when the model has no layer structure.  Same sums either way.  With hip_optimizer only
        the SUM is formed here: FlatAdamW applies 1 / world as its grad_scale."""
        world = self._world()
        if world <= 1:
            return
        flat = self.grads.flat
        if not self.layer_slices:
            if self.hip_optimizer:
                dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
            else:
                self.grads.all_reduce_mean_(self.group)
            return
        works = []
        if overlapped:
            main, comm = torch.cuda.current_stream(flat.device), self._comm_stream
            for l in reversed(range(len(self.layer_slices))):
                lo, hi = self.layer_slices[l]
                comm.wait_event(self._layer_events[l])
                with torch.cuda.stream(comm):
                    works.append(dist.all_reduce(flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            comm.wait_stream(main)                           # heads / tokens: final only when the whole backward is done
            with torch.cuda.stream(comm):
                for lo, hi in self.rest_slices:
                    works.append(dist.all_reduce(flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            for w in works:
                w.wait()
            main.wait_stream(comm)
        else:
            for lo, hi in list(reversed(self.layer_slices)) + list(self.rest_slices):
                dist.all_reduce(flat[lo:hi], op=dist.ReduceOp.SUM, group=self.group)
        if not self.hip_optimizer:
            flat.div_(world)

    def _backward_and_step(self, loss: torch.Tensor, step: int) -> None:
        """(loss / accumulation_steps).backward(), through the loss scale when cfg.loss_scaling (scaler.scale(loss).backward()); on every
        accumulation_steps-th micro-batch or the epoch's last: mean over the ranks, clip, optimizer and scheduler step, zero
        (cp_trainer:70-80 = cir_trainer:89-99)."""
        c = self.cfg
        boundary = (step + 1) % c.accumulation_steps == 0 or step + 1 == self.steps_per_epoch
        overlapped = boundary and self._arm_overlap()
        loss = loss / c.accumulation_steps
        if self.loss_scaling:
            loss = self.optimizer.scale(loss) if self.hip_optimizer else self.scaler.scale(loss)
        loss.backward()
        if boundary:
            self._boundary_step(overlapped)

    def _boundary_step(self, overlapped: bool) -> None:
        """The end of an accumulation window, on whatever the arena holds: mean over the ranks -> clip -> optimizer step -> scheduler
        step -> zero -> the model re-packs its operand copies on its next forward.  hip_optimizer: clip, step and zero are FlatAdamW's
        one call; the scheduler steps even when that call skipped a non-finite gradient (class docstring).  loss_scaling: the arena holds
        scale x the gradient; FlatAdamW's call unscales it and updates the scale itself, the torch form goes through the GradScaler."""
        self._reduce_mean(overlapped)
        if self.hip_optimizer:
            self.optimizer.grad_scale = 1.0 / self._world()
            self.optimizer.step()
            self.last_grad_norm, self.last_step_skipped = self.optimizer.grad_norm, self.optimizer.skipped
            self.scheduler.step()
        elif self.scaler is not None:
            self.scaler.unscale_(self.optimizer)
            self.last_grad_norm = self.grads.clip_norm_(self.cfg.max_grad_norm)
            self.scaler.step(self.optimizer)
            self.scaler.update()
            self.scheduler.step()
            self.grads.zero_()
        else:
            self.last_grad_norm = self.grads.clip_norm_(self.cfg.max_grad_norm)
            self.optimizer.step()
            self.scheduler.step()
            self.grads.zero_()
        getattr(self.model, "mark_weights_changed", lambda: None)()         # fused optimizers do not bump tensor versions


class CPTrainer(FlatGradTrainer):
    """model(task=CP, outfit_embedding=..., outfit_mask=...) -> [B,1] logits; batches are dicts like the reference's
    collate output: {'input_dict': {'task', 'outfit_embedding', 'outfit_mask'}, 'label'}."""

    def __init__(self, model: torch.nn.Module, steps_per_epoch: int, cfg: Optional[CPTrainConfig] = None,
                 loss_fn: Optional[Callable] = None, params: Optional[Iterable[torch.nn.Parameter]] = None, group=None):
        cfg = cfg or CPTrainConfig()
        if loss_fn is None:
            from .losses import FocalLoss
            loss_fn = FocalLoss(alpha=cfg.focal_alpha, gamma=cfg.focal_gamma, reduction="mean")
        super().__init__(model, steps_per_epoch, cfg, loss_fn, params, group)

    def micro_step(self, batch: dict, step: int):
        """One micro-batch: forward, loss / accumulation_steps, backward; optimizer step on the accumulation boundary.
        Returns (detached loss, detached logits)."""
        labels = batch["label"].to(self.grads.flat.device, non_blocking=True)
        y_hat = self.model(**self._inputs(batch)).squeeze(dim=-1)
        loss = self.loss_fn(y_hat=y_hat, y_true=labels)
        self._backward_and_step(loss, step)
        return loss.detach(), y_hat.detach(), labels

    def train_epoch(self, batches: Iterable[dict]) -> Dict[str, float]:
        self.model.train()
        self.grads.zero_()
        total = torch.zeros((), dtype=torch.float32, device=self.grads.flat.device)
        ys: List[torch.Tensor] = []; ls: List[torch.Tensor] = []
        n = 0
        for step, batch in enumerate(batches):
            loss, y, lab = self.micro_step(batch, step)
            total += loss; ys.append(y); ls.append(lab); n += 1
        return gather_epoch(torch.cat(ys), torch.cat(ls), total, max(n, 1), self.group)

    def _eval_epoch(self, batches: Iterable[dict], with_loss: bool) -> Dict[str, float]:
        """This rank's batches in eval mode without gradients -> gather_epoch over the ranks.  Only the model's forward and the loss run:
        parameters, optimizer state, scheduler and the gradient arena are not touched; the model's training flag is left as it was."""
        was_training = self.model.training
        self.model.eval()
        dev = self.grads.flat.device
        total = torch.zeros((), dtype=torch.float32, device=dev)
        ys: List[torch.Tensor] = []; ls: List[torch.Tensor] = []
        n = 0
        try:
            with torch.no_grad():
                for batch in batches:
                    labels = batch["label"].to(dev, non_blocking=True)
                    y_hat = self.model(**self._inputs(batch)).squeeze(dim=-1)
                    if with_loss:
                        total += self.loss_fn(y_hat=y_hat, y_true=labels).detach()
                    ys.append(y_hat.detach()); ls.append(labels); n += 1
                # gather_epoch returns mean over the ranks of the summed losses / batch_count: the reference's formula, whose ranks hold
                # equal batch counts.  With batches per rank = all batches / world it is the summed loss / number of batches whatever
                # the ranks hold - one small all-reduce for the count
                batch_count = float(max(n, 1))
                if with_loss and self._world() > 1:
                    count = torch.tensor([n], dtype=torch.int64, device=dev)
                    dist.all_reduce(count, op=dist.ReduceOp.SUM, group=self.group)
                    batch_count = max(int(count), 1) / self._world()
                empty = torch.empty(0, dtype=torch.float32, device=dev)            # a rank without batches still joins the all-gathers
                return gather_epoch(torch.cat(ys) if ys else empty, torch.cat(ls) if ls else empty, total, batch_count, self.group)
        finally:
            self.model.train(was_training)

    def valid_epoch(self, batches: Iterable[dict]) -> Dict[str, float]:
        """CompatibilityPredictionTrainer.valid_epoch (compatibility_prediction_trainer.py:131-182, without checkpointing and logging):
        eval mode, no gradients, per batch the forward and the loss; at the end the logits, labels and summed loss of all ranks ->
        {'loss': summed batch loss / number of batches, 'Accuracy', 'Precision', 'Recall', 'F1', 'AUC'} (the reference keeps its
        `best_AUC` checkpoint from this).  Dense or indexed batches, as train_epoch takes them."""
        return self._eval_epoch(batches, with_loss=True)

    def test_epoch(self, batches: Iterable[dict]) -> Dict[str, float]:
        """CompatibilityPredictionTrainer.test (:197-239, without the checkpoint load): valid_epoch without the loss ->
        {'Accuracy', 'Precision', 'Recall', 'F1', 'AUC'}.  The reference tests on one rank; here every rank may hold a share of the split,
        the metrics are those of all ranks' logits."""
        metrics = self._eval_epoch(batches, with_loss=False)
        del metrics["loss"]
        return metrics


class FITBEvaluator:
    """The fill-in-the-blank test (FillInTheBlankTrainer.test, fill_in_the_blank_trainer.py:37-64): per batch y_hat = model(question),
    the candidate nearest to it in L2, and a hit when that is `answer_index`; `test_epoch` -> {'Accuracy': correct / total}.

    Batches are the FITB collate dicts.  Dense ones ({'input_dict', 'candidate_item_embedding' [B, C, D], 'answer_index' [B]}) go through
    `engine.fitb_argmin`.  Index-form ones ({'input_dict', 'candidate_item_index' int32 [B, C], 'answer_index'}:
    processor.OutfitXIndexedProcessor(..., fitb_candidates='index') or sampler.FITBDeviceSplit) go through `engine.fitb_argmin_indexed`, which
    reads the candidates straight from the embedding table - `embedding_table=` here, else `model.embedding_table` - and adds its hits to
    ONE device counter that is read once, after the last batch: with FITBDeviceSplit batches an epoch runs without a host synchronisation.
    Both forms can be mixed.  `argmin_fn(y_hat, cand [B, C, D]) -> idx [B]` replaces the HIP calls (index batches are then gathered from the
    table); it is what a CPU run needs.  (correct, total) are summed over the ranks of `group` with one all-reduce: unlike the reference,
    which refuses a distributed test, every rank may hold a share of the questions."""

    def __init__(self, model: torch.nn.Module, embedding_table: Optional[torch.Tensor] = None, group=None, argmin_fn: Optional[Callable] = None):
        self.model, self.group, self.argmin_fn = model, group, argmin_fn
        p = next(model.parameters(), None)
        self.device = p.device if p is not None else torch.device("cpu")
        self.embedding_table = None if embedding_table is None else embedding_table.to(self.device)

    def _table(self) -> torch.Tensor:
        table = self.embedding_table if self.embedding_table is not None else getattr(self.model, "embedding_table", None)
        if table is None:
            raise ValueError("index-form FITB batches need an embedding table: pass embedding_table= or call model.set_embedding_table()")
        return table

    def test_epoch(self, batches: Iterable[dict]) -> Dict[str, float]:
        dev = self.device
        was_training = self.model.training
        self.model.eval()
        hits = torch.zeros(1, dtype=torch.int32, device=dev)          # every batch adds into it; read once below
        total = 0
        try:
            with torch.no_grad():
                for batch in batches:
                    y_hat = self.model(**{k: (v if k == "task" else v.to(dev, non_blocking=True)) for k, v in batch["input_dict"].items()})
                    answer = batch["answer_index"].to(dev, non_blocking=True).reshape(-1)
                    total += answer.numel()
                    indexed = "candidate_item_index" in batch
                    if indexed and self.argmin_fn is None:
                        from .engine import fitb_argmin_indexed
                        fitb_argmin_indexed(self._table(), batch["candidate_item_index"], y_hat, answer=answer, n_correct=hits)
                        continue
                    if indexed:
                        cand = self._table()[:, : y_hat.shape[-1]][batch["candidate_item_index"].to(dev).long()]
                    else:
                        cand = batch["candidate_item_embedding"].to(dev, non_blocking=True)
                    if self.argmin_fn is not None:
                        idx = self.argmin_fn(y_hat, cand)
                    else:
                        from .engine import fitb_argmin
                        idx = fitb_argmin(y_hat, cand)
                    hits += (idx.reshape(-1) == answer).sum().to(torch.int32)
                counts = torch.cat([hits.to(torch.int64), torch.tensor([total], dtype=torch.int64, device=dev)])
                if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
                    dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group)
                correct, total = (int(v) for v in counts.tolist())
        finally:
            self.model.train(was_training)
        return {"Accuracy": correct / total if total else 0.0}


class CIRTrainer(FlatGradTrainer):
    """model(task=CIR, outfit_embedding=..., outfit_mask=..., target_item_text_embedding=...) -> [B, d_embed] target-item embeddings;
    batches are the reference's collate dicts (complementary_item_retrieval_trainer.py:73-87):
    {'input_dict': {...CIR task tensors...}, 'pos_item_embedding' [B,D], 'neg_items_embedding' [B,K,D], 'neg_items_mask' [B,K] bool}.
    Replaces ComplementaryItemRetrievalTrainer.train_epoch (:66-116) and, as `valid_epoch`, its validation loop with the recall@k inside
    the target's category pool (:122-249; validation batches additionally carry 'pos_item_group' [B] and 'pos_item_row' [B], the
    positive's category and its row inside that category's pool).  Checkpoints and logging stay with the caller; so does negative sampling
    for batches made on the host - `sampler.CIRDeviceDataset` draws whole training batches on the device instead (below).

    Index-form batches (processor.OutfitXIndexedProcessor with the CIR task) carry table rows instead of embeddings:
    {'input_dict': {'task', 'item_index', 'cu_seqlens', 'target_item_index'}, 'pos_item_index' [B] int32, 'neg_items_index' [B,K] int32,
    negative = padded}.  A batch that has 'pos_item_index' takes the loss's `forward_indexed`, which reads the positives and the negatives
    straight from the embedding table - `embedding_table=` here, else `model.embedding_table` (OutfitX.set_embedding_table) - so a step is
    fed by a few hundred KB of int32 and no [B,K,D] tensor exists on host or device; same bits as the dense batch gathered from those rows.
    Both forms can be mixed freely.  The index form's tensors may already live on the device: `train_epoch(ds.epoch(batch_size, epoch))`
    with a `sampler.CIRDeviceDataset` gets every batch from one kernel call (positive, shuffled and truncated remainder, K negatives;
    `ds.set_pools` is the easy -> hard switch) with no host tensor, H2D copy or synchronisation per step.  Nothing here changes for that:
    `Engine.stage_set` trusts device-side index tensors, takes B from `cu_seqlens` and hands `item_index` over by address, so the
    dataset's over-allocated `item_index` [B * max_length] (compact up to cu_seqlens[B]) is read exactly as far as a host-built one;
    tests/test_gpu_cir_sampler.py holds losses and parameters to the bits of the same batches fed from host tensors."""

    head = "cir"

    def __init__(self, model: torch.nn.Module, steps_per_epoch: int, cfg: Optional[CIRTrainConfig] = None,
                 loss_fn: Optional[Callable] = None, params: Optional[Iterable[torch.nn.Parameter]] = None, group=None,
                 embedding_table: Optional[torch.Tensor] = None):
        cfg = cfg or CIRTrainConfig()
        self.embedding_table = None
        if loss_fn is None:
            from .losses import SetWiseRankingLoss
            loss_fn = SetWiseRankingLoss(margin=cfg.margin)
        super().__init__(model, steps_per_epoch, cfg, loss_fn, params, group)
        if embedding_table is not None:
            self.embedding_table = embedding_table.to(self.grads.flat.device)

    @staticmethod
    def _default_params(model: torch.nn.Module) -> List[torch.nn.Parameter]:
        """Every trainable parameter except OutfitX's outfit_token and CP head: they never receive a CIR gradient, and the reference's
        AdamW skips parameters whose .grad is None - inside the arena their gradient would be a zero VIEW, and AdamW's weight
        decay would shrink them on every step."""
        off = [t for t in (getattr(model, "outfit_token", None),) if isinstance(t, torch.nn.Parameter)]
        head = getattr(model, "cp_ffn", None)
        if isinstance(head, torch.nn.Module):
            off += list(head.parameters())
        off_ids = {id(t) for t in off}
        return [p for p in model.parameters() if p.requires_grad and id(p) not in off_ids]

    def _loss(self, batch: dict, y_hat: torch.Tensor) -> torch.Tensor:
        dev = self.grads.flat.device
        if "pos_item_index" in batch:
            table = self.embedding_table if self.embedding_table is not None else getattr(self.model, "embedding_table", None)
            if table is None:
                raise ValueError("index-form CIR batches need an embedding table: pass embedding_table= or call model.set_embedding_table()")
            return self.loss_fn.forward_indexed(batch_y_hat=y_hat, table=table, pos_index=batch["pos_item_index"].to(dev, non_blocking=True),
                                                neg_index=batch["neg_items_index"].to(dev, non_blocking=True))
        return self.loss_fn(batch_y=batch["pos_item_embedding"].to(dev, non_blocking=True), batch_y_hat=y_hat,
                            batch_negative_samples=batch["neg_items_embedding"].to(dev, non_blocking=True),
                            batch_negative_mask=batch["neg_items_mask"].to(dev, non_blocking=True))

    def micro_step(self, batch: dict, step: int):
        """One micro-batch (:73-99): forward, loss / accumulation_steps, backward; optimizer step on the accumulation boundary.
        Returns (detached loss, detached y_hat)."""
        y_hat = self.model(**self._inputs(batch))
        loss = self._loss(batch, y_hat)
        self._backward_and_step(loss, step)
        return loss.detach(), y_hat.detach()

    def train_epoch(self, batches: Iterable[dict]) -> Dict[str, float]:
        """-> {'loss': summed micro-batch loss / number of batches (:100, :114), averaged over the ranks}."""
        self.model.train()
        self.grads.zero_()
        total = torch.zeros((), dtype=torch.float32, device=self.grads.flat.device)
        n = 0
        for step, batch in enumerate(batches):
            total += self.micro_step(batch, step)[0]
            n += 1
        return {"loss": self._rank_mean(total, n)}

    def valid_epoch(self, batches: Iterable[dict], pools, top_k_list: Sequence[int] = (1, 5, 10, 15, 30, 50), with_recall: bool = True,
                    topk_fn: Optional[Callable] = None) -> Dict[str, float]:
        """valid_epoch (:122-191, without checkpointing and logging) + compute_recall_metrics (:192-249) on this rank's batches:
        eval mode, no gradients; per batch the forward and the loss; at the end ONE grouped retrieval of all collected y_hat, each against
        the pool of its positive's category, and parallel.grouped_recall over the ranks.
        pools = (P [n_rows, D], pool_offsets [G + 1] host ints): all category pools concatenated, replicated on every rank.
        topk_fn(Q, group_of_query, P, pool_offsets, k, gt=...) -> (idx, dist, gt_pos): Engine.l2_topk_grouped of the model's engine by
        default (HIP only); k = max(top_k_list) as in the reference.  with_recall=False: the loss only (the reference computes recall
        every fifth epoch).  -> {'loss': as train_epoch, 'Recall@K': ...}; the model's training flag is left as it was."""
        was_training = self.model.training
        self.model.eval()
        dev = self.grads.flat.device
        total = torch.zeros((), dtype=torch.float32, device=dev)
        ys: List[torch.Tensor] = []; groups: List[torch.Tensor] = []; rows: List[torch.Tensor] = []
        n = 0
        try:
            with torch.no_grad():
                for batch in batches:
                    y_hat = self.model(**self._inputs(batch))
                    total += self._loss(batch, y_hat).detach()
                    n += 1
                    if with_recall:
                        ys.append(y_hat.detach())
                        groups.append(torch.as_tensor(batch["pos_item_group"], device="cpu").to(torch.int64).reshape(-1))
                        rows.append(torch.as_tensor(batch["pos_item_row"], device="cpu").to(torch.int64).reshape(-1))
                metrics = {"loss": self._rank_mean(total, n)}
                if with_recall:
                    from .parallel import grouped_recall
                    P, offsets = pools
                    k = max(int(K) for K in top_k_list)
                    if topk_fn is None:
                        if not hasattr(self.model, "_engine"):
                            from ._lib import OfxError
                            raise OfxError("valid_epoch: the grouped retrieval runs on a HIP model's engine only; pass topk_fn otherwise")
                        topk_fn = self.model._engine().l2_topk_grouped
                    if ys:
                        grp = torch.cat(groups)
                        gt = torch.as_tensor(offsets, device="cpu").to(torch.int64)[grp] + torch.cat(rows)
                        gt_pos = topk_fn(torch.cat(ys), grp, P, offsets, k, gt=gt)[2]
                    else:
                        gt_pos = torch.empty(0, dtype=torch.int32, device=dev)           # a rank without batches still joins the all-reduce
                    metrics.update(grouped_recall(gt_pos, k, top_k_list, self.group))
        finally:
            self.model.train(was_training)
        return metrics
