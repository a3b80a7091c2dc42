"""CIR training batches built on the device (ofx_cir_sample_batch, outfitx_amd/csrc/cir_sample.hip).

The reference draws a training sample in Python, per sample: `random.choice` of the positive, `random.shuffle` of the rest of the outfit,
`random.sample` of k negatives from the positive's category pool (polyvore_complementary_item_retrieval_dataset.py:50-67, 94-109), and
a collate turns the samples into tensors.  Everything such a batch names is a row of the HBM-resident embedding table, so here the
training split and the negative pools are uploaded once as int32 index arrays and one kernel call draws a whole batch into the index
form `CIRTrainer` takes: no host tensors, no H2D copy and no host synchronisation per step.  The same distributions as the reference's,
not Python's `random` stream; a draw is a pure function of (seed, draw, batch slot), so any batch can be rebuilt.

    pools = {"easy": CIRNegativePools(semantic_category_of_row), "hard": CIRNegativePools(category_id_of_row)}
    ds = CIRDeviceDataset(outfits, pools["easy"], positive_idx_lists, negatives=10)
    trainer.train_epoch(ds.epoch(3072, epoch))          # ... ds.set_pools(pools["hard"]) is the easy -> hard switch

`FITBDeviceSplit` does the same for the fill-in-the-blank test, which draws nothing: the split's questions, candidates and answers are
uploaded once and every batch is a set of device views (`trainer.FITBEvaluator(model).test_epoch(split.batches(1024))`).
"""
from __future__ import annotations

import math
from typing import Dict, Iterator, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .configs import OutfitXConfig
from .datatypes import OutfitComplementaryItemRetrievalTask

MAX_OUTFIT_ITEMS = 64        # what one wave of the draw kernel ranks
MAX_NEGATIVES = 64
MAX_TRAIN_LEN = 31           # the training step's limit on items per set


def _upload(a: np.ndarray, device: torch.device) -> torch.Tensor:
    """int32 host array -> device tensor of at least one element (an empty array still needs an address)."""
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return torch.from_numpy(a if a.size else np.zeros(1, np.int32)).to(device)


def _device(device) -> Optional[torch.device]:
    if device is None:
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


class CIRNegativePools:
    """The negative pools of one sampling key (the reference's `negative_pool`, :94-99): `row_key[r]` is table row r's key
    (`semantic_category` for the 'easy' mode, `category_id` for 'hard'); a negative key puts the row in no pool (it then has no negatives).
    Pools are numbered in ascending key order and hold their rows in table order.  The four CSR arrays are built here on the host
    (numpy, int32: `pool_cu` [G + 1], `pool_rows`, `row_pool` [n_table] (-1 = none), `row_slot` [n_table]) and uploaded to `device`
    (default: the current HIP device; without one the instance stays host-only and cannot feed a dataset)."""

    def __init__(self, row_key, device=None):
        key = np.asarray(row_key)
        if key.ndim != 1 or key.size < 1 or not np.issubdtype(key.dtype, np.integer):
            raise ValueError("row_key must be a non-empty 1-d integer array: one sampling key per table row")
        self.n_table = int(key.size)
        rows = np.flatnonzero(key >= 0)
        order = rows[np.argsort(key[rows], kind="stable")]                    # by key, table order inside a key
        uniq, start, count = np.unique(key[order], return_index=True, return_counts=True)
        self.keys = uniq                                                      # pool g holds the rows of key keys[g]
        self.pool_cu = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
        self.pool_rows = order.astype(np.int32)
        self.row_pool = np.full(self.n_table, -1, np.int32)
        self.row_slot = np.zeros(self.n_table, np.int32)
        pool_of = np.repeat(np.arange(len(uniq)), count)
        self.row_pool[order] = pool_of
        self.row_slot[order] = np.arange(len(order)) - start[pool_of]
        self.n_pools, self.n_pool_rows = int(len(uniq)), int(len(order))
        self.device = _device(device)
        self.dev: Optional[Dict[str, torch.Tensor]] = None
        if self.device is not None:
            self.dev = {k: _upload(getattr(self, k), self.device) for k in ("pool_cu", "pool_rows", "row_pool", "row_slot")}


class FITBDeviceSplit:
    """A fill-in-the-blank split (the questions of polyvore's fill_in_the_blank/test.json) on the device, uploaded once: `question_rows`
    int [total items] and `question_cu` int [N + 1] - question q's outfit is the table rows question_rows[question_cu[q] .. question_cu[q + 1])
    -, `candidate_rows` int [N, C] - its candidates' table rows - and `answers` int [N] - which candidate is right.  `batches(batch_size)`
    yields the index-form batches `trainer.FITBEvaluator` takes, every tensor a view of (or a device computation on) the uploaded arrays: no
    H2D copy and no synchronisation per batch.  The host keeps `question_cu` to cut `item_index`; `cu_seqlens` is rebased to 0 on the device.
    `target_item_index` is the answer candidate's row, what the reference's dataset puts into `query.target_item`
    (polyvore_fill_in_the_blank_dataset.py:37-40); computed once at upload.
    ValueError: arrays that do not fit together, offsets that do not start at 0, ascend and end at len(question_rows), an answer outside
    [0, C); with `n_table` given also a row outside [0, n_table) (afterwards the rows are device-side and trusted: the kernels clamp)."""

    def __init__(self, question_rows, question_cu, candidate_rows, answers, device=None, n_table: Optional[int] = None):
        rows = np.ascontiguousarray(np.asarray(question_rows).reshape(-1), dtype=np.int32)
        cu = np.asarray(question_cu, dtype=np.int64).reshape(-1)
        cand = np.ascontiguousarray(np.asarray(candidate_rows), dtype=np.int32)
        ans = np.asarray(answers, dtype=np.int64).reshape(-1)
        n = cu.size - 1
        if n < 1 or cand.ndim != 2 or cand.shape[0] != n or cand.shape[1] < 1 or ans.size != n:
            raise ValueError(f"question_cu [{cu.size}], candidate_rows {cand.shape}, answers [{ans.size}] are not [N + 1], [N, C], [N] with N, C >= 1")
        if int(cu[0]) != 0 or bool((np.diff(cu) < 0).any()) or int(cu[-1]) != rows.size:
            raise ValueError("question_cu must start at 0, be non-decreasing and end at len(question_rows)")
        if int(ans.min()) < 0 or int(ans.max()) >= cand.shape[1]:
            raise ValueError(f"answers span [{int(ans.min())}, {int(ans.max())}]: outside [0, {cand.shape[1]})")
        if n_table is not None:
            lo = min(int(rows.min()) if rows.size else 0, int(cand.min()))
            hi = max(int(rows.max()) if rows.size else 0, int(cand.max()))
            if lo < 0 or hi >= n_table:
                raise ValueError(f"rows span [{lo}, {hi}]: outside the table's [0, {n_table})")
        self.n_questions, self.n_candidates = int(n), int(cand.shape[1])
        self.question_cu = cu                                   # host copy: where a batch's item_index starts and ends
        self.max_items = int(np.diff(cu).max())
        self.device = _device(device)
        self.dev: Optional[Dict[str, torch.Tensor]] = None
        if self.device is not None:
            target = cand[np.arange(n), ans]
            self.dev = {"question_rows": _upload(rows, self.device), "question_cu": _upload(cu, self.device),
                        "candidate_rows": _upload(cand, self.device).view(n, -1), "target_rows": _upload(target, self.device),
                        "answers": torch.from_numpy(ans).to(self.device)}

    def __len__(self) -> int:
        return self.n_questions

    def steps(self, batch_size: int) -> int:
        return math.ceil(self.n_questions / batch_size)

    def batches(self, batch_size: int, rank: int = 0, world: int = 1) -> Iterator[dict]:
        """Index-form FITB batches of `batch_size` consecutive questions (the last one ragged): {'input_dict': {'task' (the CIR class),
        'item_index', 'cu_seqlens' [B + 1] starting at 0, 'target_item_index' [B]}, 'candidate_item_index' int32 [B, C], 'answer_index'
        long [B]}, all on the device.  rank r of `world` takes batches r, r + world, ... (a test split needs no padding: the ranks may hold
        different batch counts, FITBEvaluator sums the counts)."""
        if self.dev is None:
            raise L.OfxError("FITBDeviceSplit has no HIP device: its batches are device views, there is no CPU path")
        if batch_size < 1 or not 0 <= rank < world:
            raise ValueError(f"batch_size = {batch_size}, rank = {rank}, world = {world}")
        d = self.dev
        for step in range(rank, self.steps(batch_size), world):
            q0, q1 = step * batch_size, min((step + 1) * batch_size, self.n_questions)
            i0, i1 = int(self.question_cu[q0]), int(self.question_cu[q1])
            cu = d["question_cu"][q0:q1 + 1]
            yield {"input_dict": {"task": OutfitComplementaryItemRetrievalTask, "item_index": d["question_rows"][i0:i1], "cu_seqlens": cu - cu[:1],
                                  "target_item_index": d["target_rows"][q0:q1]},
                   "candidate_item_index": d["candidate_rows"][q0:q1], "answer_index": d["answers"][q0:q1]}


class CIRDeviceDataset:
    """The CIR training split on the device.  `outfits`: one list of table rows per training outfit (2 .. 64 items);
    `positive_idx_lists`: per outfit the positions that may become the positive (the reference's `positive_idx_list`, :76-79), None =
    every position (its train mode: the large-category threshold is 0); `pools`: a CIRNegativePools over the same table;
    `max_length`: items kept of the shuffled remainder (the processor's truncation; at most 31, the training step's limit);
    `negatives`: K, the reference's `negative_sample_k`; `seed`: of every draw and of the epoch permutations.
    ValueError: an outfit of fewer than 2 or more than 64 items, a row outside the table, an eligible position outside its outfit or an
    empty list of them, max_length outside [1, 31], negatives outside [0, 64]."""

    def __init__(self, outfits: Sequence[Sequence[int]], pools: CIRNegativePools, positive_idx_lists: Optional[Sequence[Sequence[int]]] = None,
                 max_length: Optional[int] = None, negatives: int = 10, seed: int = 0):
        max_length = OutfitXConfig().max_length if max_length is None else int(max_length)
        if not 1 <= max_length <= MAX_TRAIN_LEN:
            raise ValueError(f"max_length = {max_length}; the training step takes 1 .. {MAX_TRAIN_LEN} items per set")
        if not 0 <= int(negatives) <= MAX_NEGATIVES:
            raise ValueError(f"negatives = {negatives}; the sampler draws 0 .. {MAX_NEGATIVES} per query")
        sizes = np.asarray([len(o) for o in outfits], np.int64)
        if sizes.size < 1:
            raise ValueError("no outfits")
        if int(sizes.min()) < 2 or int(sizes.max()) > MAX_OUTFIT_ITEMS:
            raise ValueError(f"an outfit holds {int(sizes.min())} .. {int(sizes.max())} items; the sampler takes 2 .. {MAX_OUTFIT_ITEMS} "
                             "(one becomes the positive, at least one remains)")
        rows = np.fromiter((r for o in outfits for r in o), np.int64, count=int(sizes.sum()))
        if int(rows.min()) < 0 or int(rows.max()) >= pools.n_table:
            raise ValueError(f"outfit rows span [{int(rows.min())}, {int(rows.max())}]: outside the table's [0, {pools.n_table})")
        if positive_idx_lists is None:
            counts = sizes
            slots = np.concatenate([np.arange(n) for n in sizes])
        else:
            if len(positive_idx_lists) != len(outfits):
                raise ValueError("positive_idx_lists must hold one list per outfit")
            counts = np.asarray([len(p) for p in positive_idx_lists], np.int64)
            if int(counts.min()) < 1:
                raise ValueError("an outfit has no eligible position (the reference drops such outfits from the split)")
            slots = np.fromiter((s for p in positive_idx_lists for s in p), np.int64, count=int(counts.sum()))
            if bool((slots < 0).any()) or bool((slots >= np.repeat(sizes, counts)).any()):
                raise ValueError("an eligible position lies outside its outfit")
        cum = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int32)
        self.host = {"outfit_cu": cum(sizes), "outfit_rows": rows.astype(np.int32), "pos_cu": cum(counts), "pos_slots": slots.astype(np.int32)}
        self.n_outfits, self.max_length, self.negatives, self.seed = int(sizes.size), max_length, int(negatives), int(seed)
        self.n_table, self.device = pools.n_table, pools.device
        self.dev = None if self.device is None else {k: _upload(v, self.device) for k, v in self.host.items()}
        self.set_pools(pools)

    def __len__(self) -> int:
        return self.n_outfits

    def set_pools(self, pools: CIRNegativePools) -> None:
        """The easy -> hard switch (the reference rebuilds its dataset with another `negative_sample_mode`): from the next batch on the
        negatives come from `pools`.  Positives and remainders do not depend on the pools."""
        if pools.n_table != self.n_table:
            raise ValueError(f"the pools index a table of {pools.n_table} rows, the split one of {self.n_table}")
        if pools.device != self.device:
            raise ValueError(f"pools live on {pools.device}, the split on {self.device}")
        self.pools = pools

    def batch(self, outfit_ids: torch.Tensor, draw: int) -> dict:
        """One index-form CIR batch of the outfits `outfit_ids` (int32 [B] on the device; anything else is converted, which copies),
        drawn under (seed, draw): {'input_dict': {'task', 'item_index' [B * max_length] (compact: what lies past cu_seqlens[B] is
        unwritten memory, never read), 'cu_seqlens' [B + 1], 'target_item_index' [B]}, 'pos_item_index' (the same tensor),
        'neg_items_index' [B, K], -1 = empty}, all int32 on the device.  Two kernel launches; nothing here waits for the device."""
        if self.dev is None:
            raise L.OfxError("CIRDeviceDataset has no HIP device: batches are drawn by a kernel, there is no CPU path")
        from .engine import Engine
        item_index, cu, target, neg = Engine.cir_sample_batch(self.dev, self.pools.dev, outfit_ids, self.seed, draw, self.negatives, self.max_length,
                                                       n_pool_rows=self.pools.n_pool_rows)
        return {"input_dict": {"task": OutfitComplementaryItemRetrievalTask, "item_index": item_index, "cu_seqlens": cu, "target_item_index": target},
                "pos_item_index": target, "neg_items_index": neg}

    def steps_per_epoch(self, batch_size: int, drop_last: bool = False, world: int = 1) -> int:
        n = math.ceil(self.n_outfits / world)
        return n // batch_size if drop_last else math.ceil(n / batch_size)

    def order(self, epoch: int, shuffle: bool = True, rank: int = 0, world: int = 1) -> torch.Tensor:
        """The outfit ids (int32, on the device) that `epoch` walks on this rank, in order: a permutation made on the device from
        (seed, epoch) - the same on every rank -, of which rank r of `world` takes elements r, r + world, ...; the list is first padded
        from its own start to a multiple of `world`, as torch's DistributedSampler pads, so every rank gets the same count."""
        if self.dev is None:
            raise L.OfxError("CIRDeviceDataset has no HIP device: batches are drawn by a kernel, there is no CPU path")
        if not 0 <= rank < world or world > self.n_outfits:
            raise ValueError(f"rank = {rank}, world = {world}, {self.n_outfits} outfits")
        if shuffle:
            gen = torch.Generator(device=self.device)
            gen.manual_seed((self.seed * 1000003 + int(epoch)) & (2 ** 63 - 1))
            order = torch.randperm(self.n_outfits, generator=gen, device=self.device).to(torch.int32)
        else:
            order = torch.arange(self.n_outfits, device=self.device, dtype=torch.int32)
        if world > 1:
            pad = -self.n_outfits % world
            order = (torch.cat([order, order[:pad]]) if pad else order)[rank::world].contiguous()
        return order

    def epoch(self, batch_size: int, epoch: int, shuffle: bool = True, drop_last: bool = False, rank: int = 0, world: int = 1) -> Iterator[dict]:
        """Batches over one pass of the split in the order of `order(epoch, shuffle, rank, world)`; every rank runs `steps_per_epoch`
        steps.  Step i draws under `draw_of(epoch, i, rank, world)`: no two (step, rank) pairs of an epoch share a draw, so the ranks'
        batches are independent draws.  The last batch is ragged unless drop_last."""
        if batch_size < 1:
            raise ValueError(f"batch_size = {batch_size}")
        order = self.order(epoch, shuffle, rank, world)
        n = order.numel()
        for step in range(self.steps_per_epoch(batch_size, drop_last, world)):
            yield self.batch(order[step * batch_size: min((step + 1) * batch_size, n)], self.draw_of(epoch, step, rank, world))

    @staticmethod
    def draw_of(epoch: int, step: int, rank: int = 0, world: int = 1) -> int:
        """The `draw` argument of step `step` of `epoch` on rank `rank`: (epoch * 2654435761 + step * world + rank) mod 2^32 - the epochs'
        ranges lie a golden-ratio stride apart, far beyond any epoch's step count."""
        return (int(epoch) * 2654435761 + int(step) * int(world) + int(rank)) & 0xFFFFFFFF
