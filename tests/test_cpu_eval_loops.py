"""CPU checks of the evaluation loops (outfitx_amd/trainer.py: CPTrainer.valid_epoch / test_epoch, the counterparts of the reference's
CompatibilityPredictionTrainer.valid_epoch / test, compatibility_prediction_trainer.py:131-239, and FITBEvaluator, the counterpart of
FillInTheBlankTrainer.test, fill_in_the_blank_trainer.py:37-64), of the index-form FITB collate (processor.OutfitXIndexedProcessor with
fitb_candidates='index') and of the new C entry in header and ctypes table.  The loops are host code: plain-torch stand-in modules drive
them here, single-process and over a world_size-2 gloo group whose ranks hold different batch counts.  (The scoring kernel and the real
model only run on a HIP device: tests/test_gpu_fitb_indexed.py.)"""
import os
import pickle
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

_COMMON = r'''
import numpy as np, torch

class CPStub(torch.nn.Module):               # stands in for OutfitX on the CP path: same call signature, plain torch, CPU
    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.a = torch.nn.Linear(16, 8); self.b = torch.nn.Linear(8, 1)
        self.drop = torch.nn.Dropout(0.5)    # eval mode must switch it off: a valid_epoch run in train mode would not repeat
    def forward(self, task, outfit_embedding, outfit_mask):
        keep = (~outfit_mask).float().unsqueeze(-1)
        pooled = (self.drop(outfit_embedding) * keep).sum(1) / keep.sum(1).clamp(min=1)
        return self.b(torch.nn.functional.mish(self.a(pooled)))

def focal(y_hat, y_true):                    # src/losses/focal_loss.py:26-41 in torch ops (the fused kernel needs a HIP device)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(y_hat, y_true, reduction="none")
    p = torch.sigmoid(y_hat); pt = p * y_true + (1 - p) * (1 - y_true)
    return ((0.75 * y_true + 0.25 * (1 - y_true)) * ce * (1 - pt) ** 2).mean()

def cp_batches(sizes=(8, 8, 5)):
    g = np.random.default_rng(5)
    out = []
    for bsz in sizes:
        emb = torch.from_numpy(g.standard_normal((bsz, 6, 16)).astype(np.float32))
        n = g.integers(1, 7, bsz)
        mask = torch.from_numpy(np.arange(6)[None, :] >= n[:, None])
        lab = torch.from_numpy((g.random(bsz) < 0.5).astype(np.float32))
        out.append({"input_dict": {"task": None, "outfit_embedding": emb, "outfit_mask": mask}, "label": lab})
    return out

def cp_reference(model, batches, with_loss):
    """compatibility_prediction_trainer.py:131-182 / :197-233 restated: eval mode, no gradients, summed batch loss / number of batches,
    the metrics of the concatenated logits."""
    from outfitx_amd.trainer import cp_metrics
    model.eval()
    ys, ls, tot = [], [], 0.0
    with torch.no_grad():
        for b in batches:
            y = model(**b["input_dict"]).squeeze(dim=-1)
            if with_loss:
                tot += float(focal(y, b["label"]))
            ys.append(y); ls.append(b["label"])
    m = cp_metrics(torch.cat(ys), torch.cat(ls))
    return {"loss": tot / len(batches), **m} if with_loss else m

D, NROWS, C = 12, 40, 4

class FITBStub(torch.nn.Module):             # stands in for OutfitX on the CIR / FITB path, dense and indexed input alike
    def __init__(self):
        super().__init__()
        torch.manual_seed(2)
        self.a = torch.nn.Linear(D + D // 2, D, bias=False)
        self.embedding_table = torch.randn(NROWS, D, generator=torch.Generator().manual_seed(3))
    def forward(self, task, outfit_embedding=None, outfit_mask=None, target_item_text_embedding=None, item_index=None, cu_seqlens=None,
                target_item_index=None):
        T = self.embedding_table
        if item_index is not None:
            cu = cu_seqlens.tolist()
            pooled = torch.stack([T[item_index[a:b].long()].sum(0) / max(b - a, 1) for a, b in zip(cu, cu[1:])])
        else:
            keep = (~outfit_mask).float().unsqueeze(-1)
            pooled = (outfit_embedding * keep).sum(1) / keep.sum(1).clamp(min=1)
        if target_item_index is not None:
            target_item_text_embedding = T[target_item_index.long(), D // 2:]
        return self.a(torch.cat([pooled, target_item_text_embedding], -1))

def fitb_batches(model, sizes=(6, 6, 3)):
    """-> (index-form batches, dense batches gathered from the same rows, the hand count of hits, the number of questions).  The answer's
    text embedding enters the model, so an answer is chosen by trying all C: even questions take one the model then picks (a hit) where
    there is one, odd questions one it does not pick (a miss) - the accuracy lies strictly between 0 and 1."""
    g = np.random.default_rng(11)
    T = model.embedding_table
    ind, den, hits, total = [], [], 0, 0
    for bsz in sizes:
        n = g.integers(1, 7, bsz)
        cu = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        rows = g.integers(0, NROWS, int(cu[-1])).astype(np.int32)
        cand = np.stack([g.permutation(NROWS)[:C] for _ in range(bsz)]).astype(np.int32)
        emb = torch.zeros(bsz, 6, D); mask = torch.ones(bsz, 6, dtype=torch.bool)
        for b in range(bsz):
            emb[b, :n[b]] = T[torch.from_numpy(rows[cu[b]:cu[b + 1]]).long()]
            mask[b, :n[b]] = False
        t = torch.from_numpy
        rows_of = T[t(cand).long()].double().numpy()
        pick = np.empty((bsz, C), np.int64)                  # pick[b, a]: the nearest candidate when candidate a is the target
        for a in range(C):
            with torch.no_grad():
                y = model(None, emb, mask, T[t(cand[:, a]).long(), D // 2:]).double().numpy()
            pick[:, a] = ((y[:, None, :] - rows_of) ** 2).sum(-1).argmin(-1)
        ans = np.empty(bsz, np.int64)
        for b in range(bsz):
            good = [a for a in range(C) if pick[b, a] == a]
            bad = [a for a in range(C) if pick[b, a] != a]
            first, second = (good, bad) if (total + b) % 2 == 0 else (bad, good)
            ans[b] = (first or second)[0]
        target = cand[np.arange(bsz), ans]
        ib = {"input_dict": {"task": None, "item_index": t(rows), "cu_seqlens": t(cu), "target_item_index": t(target.astype(np.int32))},
              "candidate_item_index": t(cand), "answer_index": t(ans.astype(np.int64))}
        db = {"input_dict": {"task": None, "outfit_embedding": emb, "outfit_mask": mask,
                             "target_item_text_embedding": T[t(target).long(), D // 2:].clone()},
              "candidate_item_embedding": T[t(cand).long()].clone(), "answer_index": t(ans.astype(np.int64))}
        with torch.no_grad():
            y = model(**db["input_dict"]).double().numpy()
        d2 = ((y[:, None, :] - T[t(cand).long()].double().numpy()) ** 2).sum(-1)
        hits += int((d2.argmin(-1) == ans).sum()); total += bsz
        ind.append(ib); den.append(db)
    return ind, den, hits, total

def cdist_argmin(y_hat, cand):               # fill_in_the_blank_trainer.py:50-53
    return torch.cdist(y_hat.unsqueeze(1), cand, p=2).squeeze(1).argmin(dim=-1)
'''


def common():
    ns = {}
    exec(_COMMON, ns)
    return ns


def test_header_and_ctypes_table_carry_the_indexed_fitb_entry_at_abi_6():
    from outfitx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"\bint ofx_fitb_argmin_indexed\s*\(const float\* table, int ld, long long n_table, const int\* cand_index,\s*"
                     r"const float\* y_hat, int B, int C, int D,\s*const int64_t\* answer, int64_t\* idx, float\* dist, int\* n_correct,\s*"
                     r"ofx_stream stream\);", hdr)
    assert int(re.search(r"#define OFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    res, args = _lib.SIGNATURES["ofx_fitb_argmin_indexed"]
    import ctypes as C
    assert res is C.c_int and len(args) == 13 and args[2] is C.c_longlong and args[1] is C.c_int and args[5:8] == [C.c_int] * 3
    lib = _lib.load()
    assert hasattr(lib, "ofx_fitb_argmin_indexed") and lib.ofx_abi_version() == 6


def test_engine_wrapper_has_no_cpu_path():
    from outfitx_amd import _lib
    from outfitx_amd.engine import fitb_argmin_indexed
    with pytest.raises(_lib.OfxError):
        fitb_argmin_indexed(torch.zeros(5, 8), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 8))


def test_indexed_fitb_collate_names_rows_and_the_default_mode_is_unchanged():
    from outfitx_amd.datatypes import (FashionItem, OutfitComplementaryItemRetrievalTask as CIR, OutfitFillInTheBlankTask as FITB)
    from outfitx_amd.embedding_store import EmbeddingTable
    from outfitx_amd.processor import OutfitXIndexedProcessor
    g = np.random.default_rng(3)
    n_items, d = 60, 1024
    ids = g.permutation(np.arange(1000, 1000 + 7 * n_items, 7))[:n_items]              # shuffled and sparse: id != row
    table = EmbeddingTable(ids, g.standard_normal((n_items, d)).astype(np.float32))
    rows = table.index()

    def item(item_id):
        e = table.embeddings[table.rows([item_id])[0]]
        return FashionItem(item_id=int(item_id), embedding=e, text_embedding=e[d // 2:])
    outfits = [[item(j) for j in g.choice(table.ids, n)] for n in (3, 0, 18, 1)]
    cand_ids = [[int(j) for j in g.choice(table.ids, 4)] for _ in outfits]
    cand_ids[2][3] = cand_ids[2][0]                                                    # a row twice within a question
    answers = [1, 0, 3, 2]
    queries = [FITB(outfit=o, target_item=item(c[a])) for o, c, a in zip(outfits, cand_ids, answers)]     # the dataset's target: the answer
    want_idx = torch.tensor([rows[it.item_id] for o in outfits for it in o[:16]], dtype=torch.int32)
    want_cu = torch.tensor(np.concatenate([[0], np.cumsum([min(len(o), 16) for o in outfits])]), dtype=torch.int32)
    proc = pickle.loads(pickle.dumps(OutfitXIndexedProcessor(FITB, id_to_row=rows, fitb_candidates="index")))
    out = proc([(q, c, a) for q, c, a in zip(queries, cand_ids, answers)])
    assert set(out) == {"input_dict", "candidate_item_index", "answer_index"}
    ind = out["input_dict"]
    assert set(ind) == {"task", "item_index", "cu_seqlens", "target_item_index"} and ind["task"] is CIR
    assert all(ind[k].dtype == torch.int32 for k in ("item_index", "cu_seqlens", "target_item_index"))
    assert torch.equal(ind["item_index"], want_idx) and torch.equal(ind["cu_seqlens"], want_cu)
    ci, ans = out["candidate_item_index"], out["answer_index"]
    assert ci.dtype == torch.int32 and ci.shape == (4, 4) and ci.tolist() == [[rows[j] for j in c] for c in cand_ids]
    assert ans.dtype == torch.long and ans.tolist() == answers
    assert torch.equal(ind["target_item_index"], ci[torch.arange(4), ans])             # the answer candidate's row
    # the default mode: today's output, from the reference dataset's samples (candidate embeddings)
    cand_emb = [np.stack([table.embeddings[rows[j]] for j in c]) for c in cand_ids]
    for p in (OutfitXIndexedProcessor(FITB, id_to_row=rows), OutfitXIndexedProcessor(FITB, id_to_row=rows, fitb_candidates="embedding")):
        dense = p([(q, e, a) for q, e, a in zip(queries, cand_emb, answers)])
        assert set(dense) == {"input_dict", "candidate_item_embedding", "answer_index"}
        dd = dense["input_dict"]
        assert set(dd) == {"task", "item_index", "cu_seqlens", "target_item_text_embedding"} and dd["task"] is CIR
        assert torch.equal(dd["item_index"], want_idx) and torch.equal(dd["cu_seqlens"], want_cu)
        assert dense["candidate_item_embedding"].dtype == torch.float32 and dense["answer_index"].tolist() == answers
        # the index batch names exactly what the dense batch carries
        T = torch.from_numpy(np.ascontiguousarray(table.embeddings))
        assert torch.equal(T[ci.long()], dense["candidate_item_embedding"])
        assert torch.equal(T[ind["target_item_index"].long(), d // 2:], dd["target_item_text_embedding"])
    # ragged candidate lists: the reference's torch.stack fails there too
    with pytest.raises(ValueError):
        proc([(queries[0], cand_ids[0], 1), (queries[1], cand_ids[1][:3], 0)])
    with pytest.raises(ValueError):
        OutfitXIndexedProcessor(FITB, id_to_row=rows, fitb_candidates="ids")


def test_cp_valid_and_test_epoch_equal_the_reference_loop_and_change_nothing():
    ns = common()
    from outfitx_amd.trainer import CPTrainConfig, CPTrainer
    m, ref = ns["CPStub"](), ns["CPStub"]()
    tr = CPTrainer(m, steps_per_epoch=3, cfg=CPTrainConfig(learning_rate=1e-2, accumulation_steps=2, n_epochs=2), loss_fn=ns["focal"])
    batches = ns["cp_batches"]()
    tr.train_epoch(batches)                               # optimizer state exists, the scheduler has moved
    ref.load_state_dict(m.state_dict())
    tr.grads.flat.copy_(torch.arange(tr.grads.flat.numel(), dtype=torch.float32))          # a gradient arena in the middle of a window
    snap = lambda: ([p.detach().clone() for p in m.parameters()], tr.grads.flat.clone(),
                    [v.clone() for s in tr.optimizer.state.values() for v in s.values() if isinstance(v, torch.Tensor)],
                    tr.scheduler.state_dict()["last_epoch"], tr.scheduler.get_last_lr())
    before = snap()
    assert before[2], "no optimizer state to guard"
    for training in (True, False):
        m.train(training)
        valid, test = tr.valid_epoch(batches), tr.test_epoch(iter(batches))
        assert m.training is training                     # the flag is restored
        want_v, want_t = ns["cp_reference"](ref, batches, True), ns["cp_reference"](ref, batches, False)
        assert list(valid) == ["loss", "Accuracy", "Precision", "Recall", "F1", "AUC"] and list(test) == list(valid)[1:]
        assert abs(valid["loss"] - want_v["loss"]) <= 1e-6 * abs(want_v["loss"])
        for k in test:
            assert valid[k] == want_v[k] and test[k] == want_t[k], (k, valid[k], test[k], want_v[k])
        assert 0.0 < valid["AUC"] < 1.0
    after = snap()
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0])) and torch.equal(before[1], after[1])
    assert len(before[2]) == len(after[2]) and all(torch.equal(a, b) for a, b in zip(before[2], after[2]))
    assert before[3:] == after[3:]
    assert all(p.grad.data_ptr() == tr.grads.flat.data_ptr() + 4 * o for p, o in zip(tr.grads.params, tr.grads.offsets))


@pytest.mark.parametrize("form", ["dense", "index", "mixed"])
def test_fitb_evaluator_accuracy_equals_the_hand_count(form):
    ns = common()
    from outfitx_amd.trainer import FITBEvaluator
    m = ns["FITBStub"]()
    ind, den, hits, total = ns["fitb_batches"](m)
    assert 0 < hits < total and total == 15
    batches = {"dense": den, "index": ind, "mixed": [ind[0], den[1], ind[2]]}[form]
    for training in (True, False):
        m.train(training)
        out = FITBEvaluator(m, argmin_fn=ns["cdist_argmin"]).test_epoch(iter(batches))
        assert out == {"Accuracy": hits / total} and m.training is training
    # the table handed to the evaluator instead of the model's
    table = m.embedding_table
    ev = FITBEvaluator(m, embedding_table=table, argmin_fn=ns["cdist_argmin"])
    assert ev.test_epoch(batches) == {"Accuracy": hits / total}
    # without argmin_fn the scoring is a HIP call: CPU tensors are refused, nothing falls back to torch
    from outfitx_amd import _lib
    with pytest.raises(_lib.OfxError):
        FITBEvaluator(m).test_epoch(batches)
    assert not m.training


_WORKER = _COMMON + r'''
import os, sys
import torch.distributed as dist
sys.path.insert(0, os.environ["OFX_ROOT"])
from outfitx_amd.trainer import CPTrainer, CPTrainConfig, FITBEvaluator

dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
mine = lambda bs: bs[:2] if rank == 0 else bs[2:]          # rank 0 holds two batches, rank 1 one (and a smaller one)
m = CPStub()
tr = CPTrainer(m, steps_per_epoch=3, cfg=CPTrainConfig(learning_rate=1e-2, accumulation_steps=2, n_epochs=2), loss_fn=focal)
batches = cp_batches()
valid, test = tr.valid_epoch(mine(batches)), tr.test_epoch(mine(batches))
want_v, want_t = cp_reference(CPStub(), batches, True), cp_reference(CPStub(), batches, False)
assert set(valid) == set(want_v) and set(test) == set(want_t)
for k in want_t:                              # rank-sharded samples arrive in another order, which the metrics do not depend on
    assert abs(valid[k] - want_v[k]) < 1e-12 and abs(test[k] - want_t[k]) < 1e-12, (k, valid[k], test[k], want_v[k])
assert abs(valid["loss"] - want_v["loss"]) <= 1e-6 * abs(want_v["loss"]), (valid["loss"], want_v["loss"])
f = FITBStub()
ind, den, hits, total = fitb_batches(f)
for bs in (ind, den):
    out = FITBEvaluator(f, argmin_fn=cdist_argmin).test_epoch(mine(bs))
    assert out == {"Accuracy": hits / total}, (out, hits, total)
# a rank without a single batch still joins the collectives
out = FITBEvaluator(f, argmin_fn=cdist_argmin).test_epoch(ind if rank == 0 else [])
assert out == {"Accuracy": hits / total}
v = tr.valid_epoch(batches if rank == 1 else [])
assert abs(v["AUC"] - want_v["AUC"]) < 1e-12 and abs(v["loss"] - want_v["loss"]) <= 1e-6 * abs(want_v["loss"])
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_eval_loops_world2_gloo_with_unequal_batch_counts_match_single_process(tmp_path):
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
