"""FocalLoss — drop-in for the reference's `src.losses.FocalLoss` (src/losses/focal_loss.py:8-41), fused: loss value and
d loss / d logits come from ONE kernel (ofx_focal_loss_ex; reduction 'mean' | 'sum' | 'none' as focal_loss.py:36-41) instead of
~12 eager elementwise launches.  Used by the CP
trainer as `FocalLoss(alpha=0.75, gamma=2, reduction='mean')` (compatibility_prediction_trainer.py:369-370).
No CPU path: HIP tensors only.

SetWiseRankingLoss — drop-in for `src.losses.SetWiseRankingLoss` (src/losses/set_wise_ranking_loss.py:5-39), the CIR trainer's loss:
on HIP tensors the value and d loss / d y_hat come from one pass over the negatives (ofx_set_rank_loss); everywhere else (CPU
tensors, other dtypes, gradients wanted into the positives or the negatives) it is the torch expression.  `forward_indexed` is the same loss
with the positives and the negatives named by row of a device-resident embedding table (ofx_set_rank_loss_indexed)."""
from __future__ import annotations

import torch
from torch import nn

from .engine import focal_loss, set_rank_loss, set_rank_loss_indexed


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat, y_true, alpha, gamma, reduction):
        loss, dl = focal_loss(y_hat, y_true, alpha, gamma, 1.0, need_grad=y_hat.requires_grad, reduction=reduction)
        ctx.save_for_backward(dl)
        ctx.shape = y_hat.shape
        return loss.view(y_hat.shape) if reduction == "none" else loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl * g.reshape(-1) if g.dim() else dl * g).view(ctx.shape), None, None, None, None


class FocalLoss(nn.Module):
    def __init__(self, gamma=2, alpha=0.5, reduction="mean"):
        super().__init__()
        assert gamma >= 0, f"Invalid Value for arg 'gamma': '{gamma}' \n Gamma should be non-negative"
        assert 0 <= alpha <= 1, f"Invalid Value for arg 'alpha': '{alpha}' \n Alpha should be in range [0, 1]"
        assert reduction in ["none", "mean", "sum"], f"Invalid Value for arg 'reduction': '{reduction}'"
        self.gamma, self.alpha, self.reduction = gamma, alpha, reduction

    def forward(self, y_hat: torch.Tensor, y_true: torch.Tensor) -> torch.Tensor:
        return _FocalFn.apply(y_hat, y_true, float(self.alpha), float(self.gamma), self.reduction)


class _SetRankFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat, y, neg, neg_mask, margin):
        loss, dy = set_rank_loss(y, y_hat, neg, neg_mask, margin, 1.0, need_grad=y_hat.requires_grad)
        ctx.save_for_backward(dy)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dy,) = ctx.saved_tensors
        return dy * g, None, None, None, None


class _SetRankIndexedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat, table, pos_index, neg_index, margin):
        loss, dy = set_rank_loss_indexed(table, pos_index, neg_index, y_hat, margin, 1.0, need_grad=y_hat.requires_grad)
        ctx.save_for_backward(dy)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dy,) = ctx.saved_tensors
        return dy * g, None, None, None, None


class SetWiseRankingLoss(nn.Module):
    """Drop-in for the reference's `src.losses.SetWiseRankingLoss` (src/losses/set_wise_ranking_loss.py:5-39), the CIR trainer's
    loss (complementary_item_retrieval_trainer.py:79-88): with d+ = ||y_hat - y||, d-_k = ||y_hat - neg_k||,
        L_all  = sum over valid negatives of relu(d+ - d-_k + margin) / max(#valid, 1)
        L_hard = mean_b relu(d+ - min_k d-_k + margin)            (padded negatives count as +inf)
    returned as L_all + L_hard; `pairwise_distance`'s eps = 1e-6 is kept.  With all four tensors on a HIP device, y_hat in fp32 and no
    gradient wanted into batch_y / batch_negative_samples (the trainer feeds precomputed embeddings) it is ONE fused kernel pass
    (outfitx_amd/csrc/rank_loss.hip: the [B,K,D] difference tensor is never materialised; d loss / d y_hat is saved for backward, which
    the HIP backward of the CIR path consumes).  Anything else - CPU tensors, other dtypes, a gradient into the positives or the
    negatives - runs the torch expression below, unchanged."""

    def __init__(self, margin: float = 2.0):
        super().__init__()
        self.margin = margin

    @staticmethod
    def _fused_ok(batch_y, batch_y_hat, batch_negative_samples, batch_negative_mask) -> bool:
        ts = (batch_y, batch_y_hat, batch_negative_samples, batch_negative_mask)
        return (all(isinstance(t, torch.Tensor) and t.device.type == "cuda" for t in ts) and batch_y_hat.dtype == torch.float32
                and batch_y.dtype == torch.float32 and batch_negative_samples.dtype == torch.float32
                and batch_negative_mask.dtype == torch.bool
                and not batch_y.requires_grad and not batch_negative_samples.requires_grad
                and batch_y_hat.dim() == 2 and batch_negative_samples.dim() == 3 and batch_y.shape == batch_y_hat.shape
                and batch_negative_mask.shape == batch_negative_samples.shape[:2] and batch_negative_samples.shape[0] == batch_y_hat.shape[0]
                and batch_negative_samples.shape[2] == batch_y_hat.shape[1] and batch_y_hat.shape[0] >= 1
                and batch_y_hat.shape[1] % 4 == 0 and 4 <= batch_y_hat.shape[1] <= 4096)

    def forward(self, batch_y, batch_y_hat, batch_negative_samples, batch_negative_mask):
        if self._fused_ok(batch_y, batch_y_hat, batch_negative_samples, batch_negative_mask):
            return _SetRankFn.apply(batch_y_hat, batch_y, batch_negative_samples, batch_negative_mask, float(self.margin))
        d_pos = torch.linalg.vector_norm(batch_y_hat - batch_y + 1e-6, dim=-1)                 # F.pairwise_distance adds eps to the difference
        d_neg = torch.linalg.vector_norm(batch_y_hat[:, None, :] - batch_negative_samples, dim=-1)
        valid = ~batch_negative_mask
        n_valid = valid.sum().clamp(min=1)
        hinge_all = torch.relu(d_pos[:, None] - d_neg + self.margin) * valid
        hardest = d_neg.masked_fill(batch_negative_mask, float("inf")).amin(dim=1)
        return hinge_all.sum() / n_valid + torch.relu(d_pos - hardest + self.margin).mean()

    def forward_indexed(self, batch_y_hat, table, pos_index, neg_index):
        """forward(table[pos_index], batch_y_hat, table[neg_index], neg_index < 0) without the gathered tensors: table [n, >= D] holds
        the item embeddings (OutfitX.embedding_table), pos_index [B] and neg_index [B, K] name rows of it, a negative neg_index is a padded
        slot (processor.OutfitXIndexedProcessor's CIR collate).  HIP tensors, fp32 y_hat and table, int32 indices: ONE fused call that
        reads the rows straight from the table - same bits as forward() on the gathered rows.  Anything else (CPU, other dtypes): the
        rows are gathered and forward() runs on them."""
        ts = (batch_y_hat, table, pos_index, neg_index)
        if (all(isinstance(t, torch.Tensor) and t.device.type == "cuda" for t in ts) and batch_y_hat.dtype == torch.float32
                and table.dtype == torch.float32 and pos_index.dtype == torch.int32 and neg_index.dtype == torch.int32
                and not table.requires_grad and batch_y_hat.dim() == 2 and table.dim() == 2 and table.stride(1) == 1
                and table.stride(0) % 4 == 0 and table.shape[0] >= 1
                and pos_index.shape == batch_y_hat.shape[:1] and neg_index.dim() == 2 and neg_index.shape[0] == batch_y_hat.shape[0]
                and batch_y_hat.shape[0] >= 1 and batch_y_hat.shape[1] % 4 == 0 and 4 <= batch_y_hat.shape[1] <= min(4096, table.shape[1])):
            return _SetRankIndexedFn.apply(batch_y_hat, table, pos_index, neg_index, float(self.margin))
        D = batch_y_hat.shape[-1]
        rows = table[:, :D]
        return self.forward(rows[pos_index.long()], batch_y_hat, rows[neg_index.clamp(min=0).long()], neg_index < 0)
