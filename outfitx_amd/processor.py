"""Collate processors: task objects -> the tensor dict that OutfitX.forward consumes.  They run in
DataLoader worker processes, so they stay picklable and CPU-only (the reference's inline test
checks exactly that: outfit_x_processor_factory.py:38-79).

Reference: src/models/processor/outfit_x/outfit_x_base_processor.py:13-81 and the CP / FITB / CIR /
PE processors next to it.  Same outputs (keys, shapes, dtypes, zero pad rows, mask True on pads);
the padding is one numpy copy per outfit instead of a torch.cat/stack chain per item.
"""
from __future__ import annotations

from typing import List, Literal, Optional, Sequence, Type

import numpy as np
import torch

from .configs import OutfitXConfig
from .datatypes import (OutfitCompatibilityPredictionTask, OutfitComplementaryItemRetrievalTask,
                        OutfitFillInTheBlankTask, OutfitPrecomputeEmbeddingTask)


class OutfitXBaseProcessor:
    def __init__(self, cfg: OutfitXConfig):
        self.cfg = cfg
        self.text_pad = ""
        self.pad_emb = torch.zeros(self.cfg.item_encoder.dim_per_modality * 2)

    def _get_max_length(self, sequences) -> int:
        """base_processor.py:45-55"""
        if self.cfg.padding == "max_length":
            return self.cfg.max_length
        longest = max(len(s) for s in sequences)
        return min(self.cfg.max_length, longest) if self.cfg.truncation else longest

    def _to_tensor_and_padding(self, sequences: Sequence[Sequence[np.ndarray]], pad_value=None):
        """base_processor.py:20-43,57-81 -> (embeddings [B,L,D] float32, mask [B,L] bool, True = pad)."""
        L = self._get_max_length(sequences)
        pad = self.pad_emb if pad_value is None else pad_value
        D = int(pad.shape[-1])
        emb = np.empty((len(sequences), L, D), np.float32)
        emb[:] = pad.numpy() if isinstance(pad, torch.Tensor) else np.asarray(pad, np.float32)
        mask = np.ones((len(sequences), L), bool)
        for i, seq in enumerate(sequences):
            n = min(len(seq), L)
            if n:
                emb[i, :n] = np.asarray(seq[:n], dtype=np.float32)
            mask[i, :n] = False
        return torch.from_numpy(emb), torch.from_numpy(mask)

    def _build_input_dict(self, queries):
        """CIR / FITB input dict (complementary_item_retrieval_processor.py:95-114)."""
        emb, mask = self._to_tensor_and_padding([[it.embedding for it in q.outfit] for q in queries])
        txt = torch.from_numpy(np.stack([np.asarray(q.target_item.text_embedding, np.float32) for q in queries]))
        return {"task": OutfitComplementaryItemRetrievalTask, "outfit_embedding": emb, "outfit_mask": mask,
                "target_item_text_embedding": txt}


class OutfitXCompatibilityPredictionTaskProcessor(OutfitXBaseProcessor):
    """compatibility_prediction_task_processor.py:6-22"""

    def __call__(self, batch):
        queries, labels = zip(*batch)
        emb, mask = self._to_tensor_and_padding([[it.embedding for it in q.outfit] for q in queries])
        return {"input_dict": {"task": OutfitCompatibilityPredictionTask, "outfit_embedding": emb, "outfit_mask": mask},
                "label": torch.tensor(labels, dtype=torch.float)}


class OutfitXFillInTheBlankTaskProcessor(OutfitXBaseProcessor):
    """fill_in_the_blank_task_processor.py:7-40 (emits the CIR task class on purpose, :36)."""

    def __call__(self, batch):
        queries, cands, answers = zip(*batch)
        return {"input_dict": self._build_input_dict(list(queries)),
                "candidate_item_embedding": torch.stack([torch.as_tensor(c) for c in cands]),
                "answer_index": torch.tensor(answers, dtype=torch.long)}


class OutfitXComplementaryItemRetrievalTaskProcessor(OutfitXBaseProcessor):
    """complementary_item_retrieval_processor.py:7-114"""

    def __init__(self, run_mode: Literal["train", "valid", "test"], *args, **kwargs):
        super().__init__(*args, **kwargs)
        if run_mode not in ("train", "valid", "test"):
            raise ValueError(f"unknown run_mode {run_mode!r}")
        self.run_mode = run_mode

    def __call__(self, batch):
        if self.run_mode == "test":
            queries, _ = zip(*batch)
            return {"input_dict": self._build_input_dict(list(queries)),
                    "pos_item_id": [q.target_item.item_id for q in queries]}
        queries, negs = zip(*batch)
        out = {"input_dict": self._build_input_dict(list(queries))}
        if self.run_mode == "valid":
            out["pos_item_id"] = [q.target_item.item_id for q in queries]
        out["pos_item_embedding"] = torch.from_numpy(np.stack([np.asarray(q.target_item.embedding, np.float32) for q in queries]))
        out["neg_items_embedding"], out["neg_items_mask"] = self._to_tensor_and_padding([list(n) for n in negs])
        return out


class OutfitXPrecomputeEmbeddingTaskProcessor(OutfitXBaseProcessor):
    """precompute_embedding_processor.py:7-16"""

    def __call__(self, batch: List[OutfitPrecomputeEmbeddingTask]):
        return {"input_dict": {"task": OutfitPrecomputeEmbeddingTask,
                               "images": [[t.fashion_item.image] for t in batch],
                               "texts": [[t.fashion_item.category] for t in batch]},
                "item_id": [t.fashion_item.item_id for t in batch]}


class OutfitXIndexedProcessor:
    """Index-emitting collate: the item embeddings stay in a device-resident table
    (`OutfitX.set_embedding_table`), a batch is `item_index` int32 [total items] + `cu_seqlens` int32 [B+1] — a few KB
    instead of the reference's padded fp32 [B, 16, 1024] (outfit_x_base_processor.py:20-81).  Outfits are truncated
    to cfg.max_length items exactly like `_get_max_length` does with truncation=True; the encoder result is identical
    to the padded form (padding never reaches the arithmetic: pad-free sets).  Picklable, CPU-only.

    CIR (`run_mode` 'train' | 'valid' | 'test', required for this task and ignored for CP / FITB): a sample is
    `(query, negative_item_ids)` - the negatives are item IDS where the reference dataset's `__getitem__` returns their embeddings
    (a dataset that samples negatives has the ids in hand before it looks the embeddings up).  Everything the batch names is a table
    row: `input_dict = {task, item_index, cu_seqlens, target_item_index}` (the target's text embedding is the second half of its row,
    polyvore_item_dataset.py:75; `OutfitX` gathers it on the device), plus `pos_item_index` int32 [B] and `neg_items_index` int32 [B, K]
    for 'train' / 'valid', plus `pos_item_id` for 'valid' / 'test'.  K and the padding are those of
    `OutfitXComplementaryItemRetrievalTaskProcessor` on the same samples (`_get_max_length`, truncation included); a padded slot holds
    -1 where that processor's `neg_items_mask` is True.  The trainer's loss reads the rows from the table
    (`SetWiseRankingLoss.forward_indexed`): a batch is a few hundred KB of int32 instead of hundreds of MB of fp32.

    FITB (`fitb_candidates` 'embedding' | 'index', ignored for CP / CIR): 'embedding', the default, takes the reference dataset's samples
    `(query, candidate_embeddings [C, D], answer_index)` and ships `candidate_item_embedding` fp32 [B, C, D] and a dense
    `target_item_text_embedding` beside the indexed outfit.  'index' takes `(query, candidate_item_ids, answer_index)` - the ids the
    reference dataset holds before it looks the embeddings up (polyvore_fill_in_the_blank_dataset.py:36-43) - and everything the batch
    names is a table row: `input_dict = {task (the CIR class, as the reference's FITB processor emits), item_index, cu_seqlens,
    target_item_index}` with `target_item_index` the row of `query.target_item` (the answer candidate, :37-40), `candidate_item_index`
    int32 [B, C] and `answer_index` long [B]; `trainer.FITBEvaluator` scores such a batch straight from the table.  Unequal candidate
    counts inside a batch raise ValueError (the reference's torch.stack fails there too).

    id_to_row: item_id -> row of the table (embedding_store.EmbeddingTable.index)."""

    def __init__(self, task: Type, cfg: Optional[OutfitXConfig] = None, id_to_row=None,
                 run_mode: Optional[Literal["train", "valid", "test"]] = None,
                 fitb_candidates: Literal["embedding", "index"] = "embedding"):
        self.task, self.cfg = task, cfg if cfg is not None else OutfitXConfig()
        self.id_to_row = id_to_row
        if task is OutfitComplementaryItemRetrievalTask and run_mode not in ("train", "valid", "test"):
            raise ValueError(f"the indexed CIR collate needs run_mode 'train' | 'valid' | 'test', got {run_mode!r}")
        if fitb_candidates not in ("embedding", "index"):
            raise ValueError(f"fitb_candidates must be 'embedding' or 'index', got {fitb_candidates!r}")
        self.run_mode = run_mode
        self.fitb_candidates = fitb_candidates

    def _row(self, item_id) -> int:
        return int(item_id) if self.id_to_row is None else int(self.id_to_row[item_id])

    def _rows(self, items) -> List[int]:
        ids = [it.item_id for it in items][: self.cfg.max_length]
        return [self._row(i) for i in ids]

    def _neg_index(self, negs) -> torch.Tensor:
        """Ragged lists of negative item ids -> int32 [B, K] rows, -1 on the padded slots; K by OutfitXBaseProcessor._get_max_length."""
        K = OutfitXBaseProcessor._get_max_length(self, negs)
        out = np.full((len(negs), K), -1, np.int32)
        for i, ids in enumerate(negs):
            n = min(len(ids), K)
            out[i, :n] = [self._row(j) for j in ids[:n]]
        return torch.from_numpy(out)

    def _index(self, outfits):
        rows = [self._rows(o) for o in outfits]
        cu = np.zeros(len(rows) + 1, np.int32)
        cu[1:] = np.cumsum([len(r) for r in rows])
        flat = np.fromiter((i for r in rows for i in r), np.int32, count=int(cu[-1]))
        return torch.from_numpy(flat), torch.from_numpy(cu)

    def __call__(self, batch):
        if self.task is OutfitCompatibilityPredictionTask:
            queries, labels = zip(*batch)
            idx, cu = self._index([q.outfit for q in queries])
            return {"input_dict": {"task": OutfitCompatibilityPredictionTask, "item_index": idx, "cu_seqlens": cu},
                    "label": torch.tensor(labels, dtype=torch.float)}
        if self.task is OutfitFillInTheBlankTask:
            queries, cands, answers = zip(*batch)
            idx, cu = self._index([q.outfit for q in queries])
            if self.fitb_candidates == "index":
                if len({len(c) for c in cands}) != 1:
                    raise ValueError(f"FITB questions of one batch must have the same number of candidates, got {sorted({len(c) for c in cands})}")
                ci = np.array([[self._row(j) for j in c] for c in cands], np.int32).reshape(len(cands), -1)
                target = torch.from_numpy(np.fromiter((self._row(q.target_item.item_id) for q in queries), np.int32, count=len(queries)))
                return {"input_dict": {"task": OutfitComplementaryItemRetrievalTask, "item_index": idx, "cu_seqlens": cu,
                                       "target_item_index": target},
                        "candidate_item_index": torch.from_numpy(ci),
                        "answer_index": torch.tensor(answers, dtype=torch.long)}
            txt = torch.from_numpy(np.stack([np.asarray(q.target_item.text_embedding, np.float32) for q in queries]))
            return {"input_dict": {"task": OutfitComplementaryItemRetrievalTask, "item_index": idx, "cu_seqlens": cu,
                                   "target_item_text_embedding": txt},
                    "candidate_item_embedding": torch.stack([torch.as_tensor(c) for c in cands]),
                    "answer_index": torch.tensor(answers, dtype=torch.long)}
        if self.task is OutfitComplementaryItemRetrievalTask:
            queries, negs = zip(*batch)
            idx, cu = self._index([q.outfit for q in queries])
            target = torch.from_numpy(np.fromiter((self._row(q.target_item.item_id) for q in queries), np.int32, count=len(queries)))
            out = {"input_dict": {"task": OutfitComplementaryItemRetrievalTask, "item_index": idx, "cu_seqlens": cu,
                                  "target_item_index": target}}
            if self.run_mode != "train":
                out["pos_item_id"] = [q.target_item.item_id for q in queries]
            if self.run_mode != "test":
                out["pos_item_index"] = target.clone()
                out["neg_items_index"] = self._neg_index([list(n) for n in negs])
            return out
        raise ValueError(f"no indexed collate for task {self.task!r}")


class OutfitXProcessorFactory:
    """outfit_x_processor_factory.py:16-36"""

    @staticmethod
    def get_processor(task: Type, cfg: Optional[OutfitXConfig] = None,
                      run_mode: Optional[Literal["train", "valid", "test"]] = None, *args, **kwargs):
        if cfg is None:
            cfg = OutfitXConfig()
        if task is OutfitCompatibilityPredictionTask:
            return OutfitXCompatibilityPredictionTaskProcessor(cfg=cfg)
        if task is OutfitComplementaryItemRetrievalTask:
            if run_mode is None:
                raise ValueError("run_mode must be specified for OutfitComplementaryItemRetrievalTask")
            return OutfitXComplementaryItemRetrievalTaskProcessor(run_mode=run_mode, cfg=cfg)
        if task is OutfitFillInTheBlankTask:
            return OutfitXFillInTheBlankTaskProcessor(cfg=cfg)
        if task is OutfitPrecomputeEmbeddingTask:
            return OutfitXPrecomputeEmbeddingTaskProcessor(cfg=cfg)
        return None
