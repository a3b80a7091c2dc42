"""CPU checks of the CIR training loop (outfitx_amd/trainer.py::CIRTrainer, the counterpart of the reference's
ComplementaryItemRetrievalTrainer.train_epoch, complementary_item_retrieval_trainer.py:66-116): the loop's host logic - loss /
accumulation_steps, boundary on every accumulation_steps-th micro-batch or the last, clip 1.0, AdamW, OneCycleLR, epoch loss - driven
by a small plain-torch stand-in module and the eager SetWiseRankingLoss, step for step against a plain-torch loop and, over a
world_size-2 gloo group, against a single-process run on the concatenated batches.  (The real model and the fused loss only run on a HIP
device: tests/test_gpu_rank_loss.py.)"""
import os
import socket
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT

_COMMON = r'''
import numpy as np, torch

class Stub(torch.nn.Module):                 # stands in for OutfitX on the CIR path: same call signature, plain torch, CPU
    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.a = torch.nn.Linear(16 + 8, 12, bias=False)
        # parts of OutfitX that are NOT on the CIR path: CIRTrainer leaves them out of its arena and its optimizer
        self.outfit_token = torch.nn.Parameter(torch.randn(16))
        self.cp_ffn = torch.nn.Sequential(torch.nn.Dropout(0.0), torch.nn.Linear(16, 1))
        self.transformer_encoder = torch.nn.Module()
        self.transformer_encoder.layers = torch.nn.ModuleList([torch.nn.Linear(16, 16) for _ in range(3)])
    def forward(self, task, outfit_embedding, outfit_mask, target_item_text_embedding):
        keep = (~outfit_mask).float().unsqueeze(-1)
        x = outfit_embedding
        for l in self.transformer_encoder.layers:
            x = x + torch.tanh(l(x))
        pooled = (x * keep).sum(1) / keep.sum(1).clamp(min=1)
        return self.a(torch.cat([pooled, target_item_text_embedding], -1))

def batches(lo, hi, n_steps, bsz, K=5):
    """Micro-batches in the reference's collate layout (cir_trainer:73-87).  Both halves of a batch carry the same number of valid
    negatives, so the mean over two ranks of the per-rank losses IS the loss of the concatenated batch (n_valid is batch-global)."""
    g = np.random.default_rng(5)
    out = []
    for s in range(n_steps):
        emb = torch.from_numpy(g.standard_normal((bsz, 6, 16)).astype(np.float32))
        n = g.integers(1, 7, bsz)
        mask = torch.from_numpy(np.arange(6)[None, :] >= n[:, None])
        txt = torch.from_numpy(g.standard_normal((bsz, 8)).astype(np.float32))
        pos = torch.from_numpy(g.standard_normal((bsz, 12)).astype(np.float32))
        neg = torch.from_numpy(g.standard_normal((bsz, K, 12)).astype(np.float32))
        half = g.random((bsz // 2, K)) < 0.3
        half[0] = True                                                                     # one row without a valid negative
        nm = torch.from_numpy(np.concatenate([half, np.roll(half, 1, axis=0)[:, ::-1]]))
        out.append({"input_dict": {"task": None, "outfit_embedding": emb[lo:hi], "outfit_mask": mask[lo:hi], "target_item_text_embedding": txt[lo:hi]},
                    "pos_item_embedding": pos[lo:hi], "neg_items_embedding": neg[lo:hi], "neg_items_mask": nm[lo:hi]})
    return out

def reference_loop(ref, loss_fn, lr, epochs, steps, bsz, accum):
    """complementary_item_retrieval_trainer.py:66-116 in plain torch (no AMP) on the full batches."""
    opt = torch.optim.AdamW(ref.parameters(), lr=lr)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=lr, epochs=epochs, steps_per_epoch=-(-steps // accum), pct_start=0.3,
                                              anneal_strategy="cos", div_factor=25, final_div_factor=1e4)
    trace = []
    for ep in range(epochs):
        opt.zero_grad()
        tot = 0.0
        for step, b in enumerate(batches(0, bsz, steps, bsz)):
            y = ref(**b["input_dict"])
            loss = loss_fn(batch_y=b["pos_item_embedding"], batch_y_hat=y, batch_negative_samples=b["neg_items_embedding"],
                           batch_negative_mask=b["neg_items_mask"])
            (loss / accum).backward()
            tot += float(loss)
            if (step + 1) % accum == 0 or step + 1 == steps:
                torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=1.0); opt.step(); opt.zero_grad(); sch.step()
            trace.append((float(loss), [p.detach().clone() for p in ref.parameters()]))
    return trace, tot / steps, sch
'''


def test_cir_train_config_defaults_are_the_reference_config():
    """src/trains/configs/complementary_item_retrieval_train_config.py:15-19 (learning_rate 2e-5, n_epochs 300, accumulation_steps 4,
    margin 2.0) and the trainer's constants (clip 1.0, cir_trainer:94; OneCycleLR pct_start 0.3 / div 25 / final div 1e4 as the CP loop)."""
    from outfitx_amd.trainer import CIRTrainConfig, CPTrainConfig
    c, p = CIRTrainConfig(), CPTrainConfig()
    assert (c.learning_rate, c.accumulation_steps, c.n_epochs, c.margin, c.max_grad_norm) == (2e-5, 4, 300, 2.0, 1.0)
    assert (c.pct_start, c.div_factor, c.final_div_factor, c.fused_optimizer) == (p.pct_start, p.div_factor, p.final_div_factor, p.fused_optimizer)


def test_cir_trainer_equals_a_plain_torch_loop_step_for_step():
    ns = {}
    exec(_COMMON, ns)
    from outfitx_amd.losses import SetWiseRankingLoss
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer, CPTrainer, FlatGradTrainer
    assert issubclass(CIRTrainer, FlatGradTrainer) and issubclass(CPTrainer, FlatGradTrainer)
    STEPS, BSZ, ACC, LR = 5, 8, 2, 1e-2               # 5 micro-steps: the last optimizer step closes a short accumulation window
    loss_fn = SetWiseRankingLoss(margin=2.0)          # CPU tensors: the torch expression
    m, ref = ns["Stub"](), ns["Stub"]()
    tr = CIRTrainer(m, steps_per_epoch=STEPS, cfg=CIRTrainConfig(learning_rate=LR, accumulation_steps=ACC, n_epochs=2), loss_fn=loss_fn)
    # the arena holds exactly the parameters on the CIR path; the CP head and outfit_token keep .grad = None and are never stepped
    off = [m.outfit_token, *m.cp_ffn.parameters()]
    assert all(p.grad is None for p in off) and len(tr.grads.params) == len(list(m.parameters())) - len(off)
    assert tr.layer_slices is not None and len(tr.layer_slices) == 3 and tr.rest_slices
    trace, want_epoch_loss, sch = ns["reference_loop"](ref, loss_fn, LR, 2, STEPS, BSZ, ACC)
    i = 0
    for ep in range(2):
        tr.model.train(); tr.grads.zero_()
        for step, b in enumerate(ns["batches"](0, BSZ, STEPS, BSZ)):
            loss, y = tr.micro_step(b, step)
            want_loss, want_params = trace[i]; i += 1
            assert y.shape == (BSZ, 12) and abs(float(loss) - want_loss) <= 2e-5 * abs(want_loss) + 1e-6, (ep, step, float(loss), want_loss)
            for a, w in zip(m.parameters(), want_params):
                assert torch.allclose(a, w, rtol=2e-5, atol=1e-6), (ep, step, (a - w).abs().max())
    assert abs(tr.scheduler.get_last_lr()[0] - sch.get_last_lr()[0]) < 1e-12
    assert all(torch.equal(a, b) for a, b in zip(off, [ref.outfit_token, *ref.cp_ffn.parameters()]))
    # train_epoch: the same loop, returning the epoch loss (summed micro-batch loss / number of batches)
    m2 = ns["Stub"]()
    tr2 = CIRTrainer(m2, steps_per_epoch=STEPS, cfg=CIRTrainConfig(learning_rate=LR, accumulation_steps=ACC, n_epochs=2), loss_fn=loss_fn)
    for ep in range(2):
        out = tr2.train_epoch(ns["batches"](0, BSZ, STEPS, BSZ))
    assert set(out) == {"loss"} and abs(out["loss"] - want_epoch_loss) <= 2e-5 * abs(want_epoch_loss)
    for a, w in zip(m2.parameters(), m.parameters()):
        assert torch.equal(a, w)


def test_set_wise_ranking_loss_cpu_path_is_the_torch_expression_and_feeds_every_input():
    """CPU tensors never reach the kernel: value = the reference's composition (set_wise_ranking_loss.py:21-36), and gradients flow into
    y_hat, the positives and the negatives alike."""
    from outfitx_amd.losses import SetWiseRankingLoss
    g = torch.Generator().manual_seed(3)
    y, yh, neg = (torch.randn(6, 16, generator=g, requires_grad=True), torch.randn(6, 16, generator=g, requires_grad=True),
                  torch.randn(6, 4, 16, generator=g, requires_grad=True))
    nm = torch.rand(6, 4, generator=g) < 0.3
    nm[2] = True
    loss = SetWiseRankingLoss(margin=2.0)(batch_y=y, batch_y_hat=yh, batch_negative_samples=neg, batch_negative_mask=nm)
    import torch.nn.functional as F
    pos_dist = F.pairwise_distance(yh, y)
    neg_d = torch.norm(yh.unsqueeze(1) - neg, dim=2)
    valid = (~nm).float()
    want = (F.relu(pos_dist.unsqueeze(1) - neg_d + 2.0) * valid).sum() / valid.sum().clamp(min=1) \
        + F.relu(pos_dist - neg_d.masked_fill(nm, torch.inf).min(dim=1).values + 2.0).mean()
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want))
    loss.backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().sum() > 0 for t in (y, yh, neg))


_WORKER = _COMMON + r'''
import os, sys
import torch.distributed as dist
sys.path.insert(0, os.environ["OFX_ROOT"])
from outfitx_amd.losses import SetWiseRankingLoss
from outfitx_amd.trainer import CIRTrainer, CIRTrainConfig

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
STEPS, BSZ, ACC, LR = 5, 8, 2, 1e-2
half = BSZ // world
loss_fn = SetWiseRankingLoss(margin=2.0)
m = Stub()
tr = CIRTrainer(m, steps_per_epoch=STEPS, cfg=CIRTrainConfig(learning_rate=LR, accumulation_steps=ACC, n_epochs=2), loss_fn=loss_fn)
for ep in range(2):
    out = tr.train_epoch(batches(rank * half, (rank + 1) * half, STEPS, BSZ))
ref = Stub()
trace, want_loss, sch = reference_loop(ref, loss_fn, LR, 2, STEPS, BSZ, ACC)
for a, b in zip(m.parameters(), ref.parameters()):
    assert torch.allclose(a, b, rtol=2e-5, atol=1e-6), (a - b).abs().max()
assert abs(tr.scheduler.get_last_lr()[0] - sch.get_last_lr()[0]) < 1e-12
assert abs(out["loss"] - want_loss) < 1e-5 * abs(want_loss), (out, want_loss)
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_cir_trainer_world2_gloo_matches_single_process(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFX_ROOT=ROOT, OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
