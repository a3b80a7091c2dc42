"""CPU checks of index-form CIR batches: the indexed collate (processor.OutfitXIndexedProcessor with the CIR task) against the dense CIR
processor on the same samples, SetWiseRankingLoss.forward_indexed's gather path against forward() on the gathered tensors, CIRTrainer fed
by index batches against the same trainer fed by the dense batches gathered from those indices (a plain-torch stand-in module in the style
of tests/test_cpu_cir_trainer.py), and the new C entry in header and ctypes table.  Everything is compared bit for bit: an index batch
names the rows a dense batch carries, so nothing may differ.  (The fused kernel only runs on a HIP device: tests/test_gpu_cir_indexed.py.)"""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from outfitx_amd.configs import ItemEncoderConfig, OutfitXConfig
from outfitx_amd.datatypes import (FashionItem, OutfitCompatibilityPredictionTask as CP, OutfitComplementaryItemRetrievalTask as CIR,
                                   OutfitFillInTheBlankTask as FITB)
from outfitx_amd.embedding_store import EmbeddingTable
from outfitx_amd.processor import OutfitXComplementaryItemRetrievalTaskProcessor, OutfitXIndexedProcessor

N_ITEMS, D = 60, 1024


def make_table(seed=3):
    """An EmbeddingTable whose ids are shuffled and sparse, so id != row anywhere it matters."""
    g = np.random.default_rng(seed)
    ids = g.permutation(np.arange(1000, 1000 + 7 * N_ITEMS, 7))[:N_ITEMS]
    return EmbeddingTable(ids, g.standard_normal((N_ITEMS, D)).astype(np.float32))


def item(table, item_id):
    e = table.embeddings[table.rows([item_id])[0]]
    return FashionItem(item_id=int(item_id), embedding=e, text_embedding=e[D // 2:])      # polyvore_item_dataset.py:75


def cir_samples(table, neg_counts, seed=4, outfit_lens=None):
    """(dense samples, indexed samples): the same queries; negatives as embeddings (the reference dataset) and as ids."""
    g = np.random.default_rng(seed)
    dense, indexed = [], []
    for i, nk in enumerate(neg_counts):
        n = int(g.integers(0, 7)) if outfit_lens is None else outfit_lens[i]
        q = CIR(outfit=[item(table, j) for j in g.choice(table.ids, n)], target_item=item(table, g.choice(table.ids)))
        neg_ids = [int(j) for j in g.choice(table.ids, nk)]                    # with replacement: rows repeat
        if nk > 2:
            neg_ids[1] = q.target_item.item_id                                  # a negative may equal the positive
        dense.append((q, [table.embeddings[table.rows([j])[0]] for j in neg_ids]))
        indexed.append((q, neg_ids))
    return dense, indexed


def gather_outfits(emb, idx, cu):
    """[total, D] rows + cu_seqlens -> list of per-outfit [n, D] blocks."""
    return [emb[idx[cu[b]:cu[b + 1]].long()] for b in range(len(cu) - 1)]


@pytest.mark.parametrize("padding,counts,lens", [("max_length", [3, 0, 20, 16, 1], [2, 0, 18, 16, 5]), ("longest", [3, 0, 5, 1], None),
                                                ("longest", [3, 0, 20, 1], [1, 17, 3, 0])])
@pytest.mark.parametrize("run_mode", ["train", "valid", "test"])
def test_indexed_cir_collate_names_the_rows_the_dense_collate_carries(run_mode, padding, counts, lens):
    """Ragged negative lists with an empty one and one longer than cfg.max_length = 16 (truncated by both collates), outfits longer than
    max_length too; keys, dtypes, shapes; table rows gathered by the emitted indices == the dense processor's tensors, bit for bit;
    neg_items_index < 0 == neg_items_mask; the collate survives a pickle round trip."""
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))          # 512 + 512: the rows of make_table
    cfg.padding = padding
    table = make_table()
    T = torch.from_numpy(np.ascontiguousarray(table.embeddings))
    dense_s, idx_s = cir_samples(table, counts, outfit_lens=lens)
    dense = OutfitXComplementaryItemRetrievalTaskProcessor(run_mode=run_mode, cfg=cfg)(dense_s)
    proc = pickle.loads(pickle.dumps(OutfitXIndexedProcessor(CIR, cfg, table.index(), run_mode=run_mode)))
    out = proc(idx_s)
    B = len(counts)
    want_keys = {"train": {"input_dict", "pos_item_index", "neg_items_index"},
                 "valid": {"input_dict", "pos_item_index", "neg_items_index", "pos_item_id"}, "test": {"input_dict", "pos_item_id"}}[run_mode]
    assert set(out) == want_keys
    ind = out["input_dict"]
    assert set(ind) == {"task", "item_index", "cu_seqlens", "target_item_index"} and ind["task"] is CIR
    assert all(ind[k].dtype == torch.int32 for k in ("item_index", "cu_seqlens", "target_item_index"))
    assert ind["cu_seqlens"].shape == (B + 1,) and ind["target_item_index"].shape == (B,)
    assert ind["item_index"].shape == (int(ind["cu_seqlens"][-1]),)
    # the outfit set: valid positions of the dense tensor, outfit by outfit (the dense collate pads to its own L; both truncate at 16)
    dd = dense["input_dict"]
    for b, rows in enumerate(gather_outfits(T, ind["item_index"], ind["cu_seqlens"])):
        valid = ~dd["outfit_mask"][b]
        assert int(valid.sum()) == len(rows) and torch.equal(dd["outfit_embedding"][b][valid], rows), b
    assert torch.equal(T[ind["target_item_index"].long(), D // 2:], dd["target_item_text_embedding"])
    if run_mode != "train":
        assert out["pos_item_id"] == dense["pos_item_id"]
    if run_mode == "test":
        return
    pos, neg = out["pos_item_index"], out["neg_items_index"]
    assert pos.dtype == torch.int32 and neg.dtype == torch.int32 and pos.shape == (B,)
    assert neg.shape == dense["neg_items_mask"].shape == dense["neg_items_embedding"].shape[:2]              # the same K
    assert torch.equal(T[pos.long()], dense["pos_item_embedding"])
    assert torch.equal(neg < 0, dense["neg_items_mask"])
    assert torch.equal(T[neg.clamp(min=0).long()] * (neg >= 0)[..., None], dense["neg_items_embedding"])     # dense pad rows are zeros
    assert torch.equal(pos, ind["target_item_index"])


def test_indexed_cir_collate_needs_a_run_mode_and_cp_fitb_output_is_unchanged():
    table = make_table()
    rows = table.index()
    for bad in (None, "eval"):
        with pytest.raises(ValueError):
            OutfitXIndexedProcessor(CIR, id_to_row=rows, run_mode=bad)
    g = np.random.default_rng(9)
    outfits = [[item(table, j) for j in g.choice(table.ids, n)] for n in (3, 0, 18, 1)]
    want_idx = torch.tensor([rows[it.item_id] for o in outfits for it in o[:16]], dtype=torch.int32)
    want_cu = torch.tensor(np.concatenate([[0], np.cumsum([min(len(o), 16) for o in outfits])]), dtype=torch.int32)
    # CP: the dict built by hand as the task does today; run_mode is ignored
    cp_batch = [(CP(outfit=o), float(i % 2)) for i, o in enumerate(outfits)]
    for proc in (OutfitXIndexedProcessor(CP, id_to_row=rows), OutfitXIndexedProcessor(CP, id_to_row=rows, run_mode="train")):
        out = proc(cp_batch)
        assert set(out) == {"input_dict", "label"} and set(out["input_dict"]) == {"task", "item_index", "cu_seqlens"}
        assert out["input_dict"]["task"] is CP and torch.equal(out["label"], torch.tensor([0.0, 1.0, 0.0, 1.0]))
        for k, w in (("item_index", want_idx), ("cu_seqlens", want_cu)):
            assert out["input_dict"][k].dtype == torch.int32 and torch.equal(out["input_dict"][k], w)
    # FITB
    cands = [g.standard_normal((4, D)).astype(np.float32) for _ in outfits]
    fitb_batch = [(FITB(outfit=o, target_item=item(table, table.ids[i])), cands[i], i % 4) for i, o in enumerate(outfits)]
    for proc in (OutfitXIndexedProcessor(FITB, id_to_row=rows), OutfitXIndexedProcessor(FITB, id_to_row=rows, run_mode="test")):
        out = proc(fitb_batch)
        assert set(out) == {"input_dict", "candidate_item_embedding", "answer_index"}
        ind = out["input_dict"]
        assert set(ind) == {"task", "item_index", "cu_seqlens", "target_item_text_embedding"} and ind["task"] is CIR
        assert torch.equal(ind["item_index"], want_idx) and torch.equal(ind["cu_seqlens"], want_cu)
        assert torch.equal(ind["target_item_text_embedding"], torch.from_numpy(np.stack([table.embeddings[i, D // 2:] for i in range(4)])))
        assert torch.equal(out["candidate_item_embedding"], torch.from_numpy(np.stack(cands)))
        assert out["answer_index"].dtype == torch.long and out["answer_index"].tolist() == [0, 1, 2, 3]


def index_batch_parts(seed, B, K, n_rows, d):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(n_rows, d, generator=g)
    pos = torch.randint(0, n_rows, (B,), generator=g, dtype=torch.int32)
    neg = torch.randint(0, n_rows, (B, K), generator=g, dtype=torch.int32)
    neg[torch.rand(B, K, generator=g) < 0.3] = -1
    neg[B // 2] = -1                                                            # one row without a valid negative
    neg[0, 0] = pos[0]                                                          # a negative equal to the positive
    return table, pos, neg


def test_forward_indexed_on_cpu_is_forward_on_the_gathered_tensors():
    from outfitx_amd.losses import SetWiseRankingLoss
    fn = SetWiseRankingLoss(margin=2.0)
    table, pos, neg = index_batch_parts(11, 6, 5, 30, 16)
    y1 = torch.randn(6, 16, generator=torch.Generator().manual_seed(12), requires_grad=True)
    y2 = y1.detach().clone().requires_grad_(True)
    got = fn.forward_indexed(y1, table, pos, neg)
    want = fn(table[pos.long()], y2, table[neg.clamp(min=0).long()], neg < 0)
    assert torch.equal(got, want)
    got.backward(); want.backward()
    assert y1.grad is not None and y1.grad.abs().sum() > 0 and torch.equal(y1.grad, y2.grad)
    # a table wider than y_hat: a row's first D floats are the embedding; int64 indices are taken as well
    wide = torch.cat([table, torch.full((30, 4), 7.0)], 1)
    assert torch.equal(fn.forward_indexed(y1.detach(), wide, pos.long(), neg.long()), want.detach())


class Stub(torch.nn.Module):
    """Stands in for OutfitX on the CIR path in both input forms: plain torch, CPU.  The indexed form gathers what the dense form is
    handed, so the two forms run the same arithmetic on the same values."""

    def __init__(self, table=None):
        super().__init__()
        torch.manual_seed(1)
        self.a = torch.nn.Linear(16 + 8, 16, bias=False)
        self.outfit_token = torch.nn.Parameter(torch.randn(16))                # not on the CIR path, as in OutfitX
        self.cp_ffn = torch.nn.Sequential(torch.nn.Dropout(0.0), torch.nn.Linear(16, 1))
        self.transformer_encoder = torch.nn.Module()
        self.transformer_encoder.layers = torch.nn.ModuleList([torch.nn.Linear(16, 16) for _ in range(2)])
        if table is not None:
            self.embedding_table = table

    def forward(self, task, outfit_embedding=None, outfit_mask=None, target_item_text_embedding=None, item_index=None, cu_seqlens=None,
                target_item_index=None, table=None):
        table = table if table is not None else getattr(self, "embedding_table", None)
        if item_index is not None:
            outfit_embedding, outfit_mask = pad_sets(table, item_index, cu_seqlens)
        if target_item_index is not None:
            target_item_text_embedding = table[target_item_index.long(), 8:]
        keep = (~outfit_mask).float().unsqueeze(-1)
        x = outfit_embedding
        for l in self.transformer_encoder.layers:
            x = x + torch.tanh(l(x))
        pooled = (x * keep).sum(1) / keep.sum(1).clamp(min=1)
        return self.a(torch.cat([pooled, target_item_text_embedding], -1))


def pad_sets(table, item_index, cu_seqlens, L=6):
    B = len(cu_seqlens) - 1
    emb, mask = torch.zeros(B, L, table.shape[1]), torch.ones(B, L, dtype=torch.bool)
    for b in range(B):
        lo, hi = int(cu_seqlens[b]), int(cu_seqlens[b + 1])
        emb[b, :hi - lo] = table[item_index[lo:hi].long()]
        mask[b, :hi - lo] = False
    return emb, mask


def both_forms(table, steps, B=8, K=5):
    """Index batches and the dense batches gathered from the same indices."""
    g = torch.Generator().manual_seed(21)
    indexed, dense = [], []
    for s in range(steps):
        n = torch.randint(1, 7, (B,), generator=g)
        cu = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)]).int()
        idx = torch.randint(0, len(table), (int(cu[-1]),), generator=g, dtype=torch.int32)
        _, pos, neg = index_batch_parts(100 + s, B, K, len(table), 16)
        indexed.append({"input_dict": {"task": None, "item_index": idx, "cu_seqlens": cu, "target_item_index": pos.clone()},
                        "pos_item_index": pos, "neg_items_index": neg})
        emb, mask = pad_sets(table, idx, cu)
        dense.append({"input_dict": {"task": None, "outfit_embedding": emb, "outfit_mask": mask, "target_item_text_embedding": table[pos.long(), 8:]},
                      "pos_item_embedding": table[pos.long()], "neg_items_embedding": table[neg.clamp(min=0).long()], "neg_items_mask": neg < 0})
    return indexed, dense


def test_cir_trainer_on_index_batches_equals_the_trainer_on_the_gathered_dense_batches():
    from outfitx_amd.losses import SetWiseRankingLoss
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    STEPS, ACC, LR = 5, 2, 1e-2
    table = torch.randn(40, 16, generator=torch.Generator().manual_seed(20))
    indexed, dense = both_forms(table, STEPS)
    cfg = lambda: CIRTrainConfig(learning_rate=LR, accumulation_steps=ACC, n_epochs=2)
    runs = {}
    # the table from the model's attribute, from the constructor argument, and the dense batches
    for name, model, kw, batches in (("model_table", Stub(table), {}, indexed), ("ctor_table", Stub(), {"embedding_table": table}, indexed),
                                     ("dense", Stub(), {}, dense)):
        tr = CIRTrainer(model, steps_per_epoch=STEPS, cfg=cfg(), loss_fn=SetWiseRankingLoss(margin=2.0), **kw)
        if name == "ctor_table":                                # the stand-in's forward needs the rows too: hand them to every call
            batches = [dict(b, input_dict=dict(b["input_dict"], table=table)) for b in batches]
        losses = []
        for ep in range(2):
            model.train(); tr.grads.zero_()
            losses += [tr.micro_step(b, step)[0] for step, b in enumerate(batches)]
        runs[name] = (torch.stack(losses), [p.detach().clone() for p in model.parameters()])
    for name in ("model_table", "ctor_table"):
        assert torch.equal(runs[name][0], runs["dense"][0]), (name, runs[name][0], runs["dense"][0])
        assert all(torch.equal(a, b) for a, b in zip(runs[name][1], runs["dense"][1])), name
    assert float(runs["dense"][0].min()) > 0 and not torch.equal(runs["dense"][1][0], Stub().a.weight)       # it trained
    # train_epoch / valid_epoch take the same batches
    tr = CIRTrainer(Stub(table), steps_per_epoch=STEPS, cfg=cfg(), loss_fn=SetWiseRankingLoss(margin=2.0))
    td = CIRTrainer(Stub(), steps_per_epoch=STEPS, cfg=cfg(), loss_fn=SetWiseRankingLoss(margin=2.0))
    assert tr.train_epoch(indexed) == td.train_epoch(dense)
    assert tr.valid_epoch(indexed, None, with_recall=False) == td.valid_epoch(dense, None, with_recall=False)
    # no table anywhere: ValueError, from the loss step (the stand-in is handed its rows per call)
    bare = CIRTrainer(Stub(), steps_per_epoch=STEPS, cfg=cfg(), loss_fn=SetWiseRankingLoss(margin=2.0))
    with pytest.raises(ValueError, match="embedding table"):
        bare.micro_step(dict(indexed[0], input_dict=dict(indexed[0]["input_dict"], table=table)), 0)


def test_header_and_ctypes_table_carry_the_indexed_entry():
    from outfitx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert re.search(r"\bint ofx_set_rank_loss_indexed\s*\(const float\* table, int ld, long long n_table,", hdr)
    assert "ofx_set_rank_loss_indexed" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["ofx_set_rank_loss_indexed"]
    assert len(args) == 18 and len(args) == len(_lib.SIGNATURES["ofx_set_rank_loss"][1]) + 2
    assert int(re.search(r"#define OFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert hasattr(_lib.load(), "ofx_set_rank_loss_indexed")
