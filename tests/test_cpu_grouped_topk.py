"""CPU checks of the category-pool CIR retrieval's host side: the exact host reference (tests/grouped_topk_ref.py, what
tests/test_gpu_grouped_topk.py holds the kernels to) against the reference's own formulation
(complementary_item_retrieval_trainer.py:192-249), parallel.grouped_recall on one rank and over a world_size-2 gloo group, and
CIRTrainer.valid_epoch driven by the stand-in module of tests/test_cpu_cir_trainer.py with the host reference as its topk_fn."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from grouped_topk_ref import grouped_topk_ref, recall_counts, recall_ref
from oracle import np_oracle as O

TOP_K = (1, 5, 10, 15, 30, 50)


def test_grouped_reference_equals_the_padded_cdist_topk_recall_of_the_reference_trainer():
    """compute_recall_metrics written out: equal-size pools stacked [C, P, D], each category's queries zero-padded to [C, maxq, D],
    torch.cdist -> torch.topk(50, largest=False) -> masked any(idx[:, :, :K] == gt) hit ratio.  Lattice D = 64, values in [-16, 16], 150
    rows per pool: d2 spreads over thousands of integers, so few ground truths are tied (cap asserted: 5 % of the queries).  Each
    query's ground truth is the row at a drawn rank of the exact order, ranks 0 .. 79: every K of the list has hits and misses."""
    C, PN, D, K = 5, 150, 64, 50
    nq_of = [40, 7, 0, 25, 1]                                   # category 2 has no query: the reference never sees it
    P = O.lattice(11, C * PN, D, -16, 16)
    off = np.arange(C + 1) * PN
    grp = np.concatenate([np.full(n, c) for c, n in enumerate(nq_of)])
    nq = len(grp)
    Q = O.lattice(12, nq, D, -16, 16)
    g = np.random.default_rng(13)
    perm = g.permutation(nq)                                    # the caller's order: categories interleaved
    grp, Q = grp[perm], Q[perm]
    gt = np.empty(nq, np.int64)
    tied = np.zeros(nq, bool)
    for q in range(nq):
        lo = off[grp[q]]
        d2 = O.d2_exact(Q[q:q + 1], P[lo:lo + PN])[0]
        r = np.argsort(d2, kind="stable")[g.integers(0, 80)]
        gt[q] = lo + r
        tied[q] = (d2 == d2[r]).sum() > 1
    assert tied.sum() <= 0.05 * nq, tied.sum()
    idx, d2k, gt_pos = grouped_topk_ref(Q, grp, P, off, K, gt)
    assert idx.shape == d2k.shape == (nq, K) and (idx >= 0).all() and np.isfinite(d2k).all()
    assert ((idx >= off[grp][:, None]) & (idx < off[grp + 1][:, None])).all()          # nothing from another category's pool

    # the reference's formulation
    cats = [c for c in range(C) if nq_of[c]]
    maxq = max(nq_of)
    Qp = torch.zeros(len(cats), maxq, D)
    gtp = torch.full((len(cats), maxq), -1, dtype=torch.long)
    mask = torch.zeros(len(cats), maxq, dtype=torch.bool)
    where = {}
    for ci, c in enumerate(cats):
        sel = np.flatnonzero(grp == c)
        Qp[ci, :len(sel)] = torch.from_numpy(Q[sel])
        gtp[ci, :len(sel)] = torch.from_numpy(gt[sel] - off[c])
        mask[ci, :len(sel)] = True
        where.update({int(q): (ci, j) for j, q in enumerate(sel)})
    cand = torch.stack([torch.from_numpy(P[off[c]:off[c + 1]]) for c in cats])
    td, ti = torch.topk(torch.cdist(Qp, cand), k=max(TOP_K), largest=False)
    td2 = np.rint(td.numpy().astype(np.float64) ** 2)

    # index sets per distinct distance, as tests/test_cpu_scoring_ref.py compares them (torch's order inside a tie is unspecified)
    for q in range(nq):
        ci, j = where[q]
        c = cats[ci]
        full = O.d2_exact(Q[q:q + 1], P[off[c]:off[c + 1]])[0]
        assert np.array_equal(td2[ci, j], d2k[q])
        for v in np.unique(d2k[q]):
            ours, theirs = set(idx[q, d2k[q] == v] - off[c]), set(ti[ci, j].numpy()[td2[ci, j] == v])
            if v < d2k[q, -1]:
                assert ours == theirs
            else:
                assert len(ours) == len(theirs) and theirs <= set(np.flatnonzero(full == v))
                assert sorted(ours) == list(np.flatnonzero(full == v)[:len(ours)])

    # recall: exactly equal over the queries whose ground truth is not tied with another row of its pool
    keep = mask.clone()
    for q in np.flatnonzero(tied):
        keep[where[int(q)]] = False
    want = recall_ref(gt_pos[~tied], TOP_K)
    for k in TOP_K:
        hits = (keep.unsqueeze(-1) & (ti[:, :, :k] == gtp.unsqueeze(-1))).any(dim=-1).float()
        assert hits.sum().item() / keep.sum().item() == want[f"Recall@{k}"], k
    assert 0 < want["Recall@1"] < want["Recall@10"] < want["Recall@50"] < 1


def test_grouped_reference_tail_and_ground_truth_position():
    """A pool of fewer than k rows ends in -1 / +inf; gt_pos is the position, k for a row the list does not hold, -1 without ground truth."""
    P = O.lattice(1, 7 + 30, 32, -8, 8)
    Q = O.lattice(2, 3, 32, -8, 8)
    off = [0, 7, 37]
    idx, d2, _ = grouped_topk_ref(Q, [0, 1, 0], P, off, 10)
    assert (idx[[0, 2], 7:] == -1).all() and np.isinf(d2[[0, 2], 7:]).all() and sorted(idx[0, :7]) == list(range(7))
    assert (idx[1] >= 7).all() and (np.diff(d2[1]) >= 0).all()
    far = int(np.setdiff1d(np.arange(7, 37), idx[1])[0])
    _, _, pos = grouped_topk_ref(Q, [0, 1, 0], P, off, 10, gt=[idx[0, 3], far, -1])
    assert pos.tolist() == [3, 10, -1]
    assert recall_counts(pos, (1, 5, 10)) == ([0, 1, 1], 2)


def test_panel_table_is_runs_of_one_group_cut_at_128_queries_and_at_call_ends():
    """Engine.l2_topk_grouped's host step, 5 / 0 / 128 / 129 / 300 / 1 queries per group, as one call and as calls of 100 and 128 queries:
    per call the panels ascend, are disjoint and cover the call's queries; each holds at most 128 queries of ONE group and names that
    group's pool rows.  One call: exactly ceil(n / 128) panels per group."""
    from outfitx_amd.engine import _group_panels
    counts = [5, 0, 128, 129, 300, 1]
    off = torch.tensor([0, 10, 30, 60, 100, 150, 210])
    sg = torch.repeat_interleave(torch.arange(6), torch.tensor(counts))
    nq = len(sg)
    for chunk in (nq, 100, 128):
        table, calls = _group_panels(sg, off, chunk)
        assert table.dtype == torch.int32 and table.shape[1] == 4
        assert [(c0, c1) for c0, c1, _, _ in calls] == [(c0, min(c0 + chunk, nq)) for c0 in range(0, nq, chunk)]
        assert sum(n for _, _, _, n in calls) == len(table) and [f for _, _, f, _ in calls] == list(np.cumsum([0] + [n for _, _, _, n in calls])[:-1])
        for c0, c1, first, n in calls:
            at = 0
            for q_lo, q_hi, p_lo, p_hi in table[first:first + n].tolist():
                g = int(sg[c0 + q_lo])
                assert q_lo == at and 0 < q_hi - q_lo <= 128 and (sg[c0 + q_lo:c0 + q_hi] == g).all() and (p_lo, p_hi) == (int(off[g]), int(off[g + 1]))
                at = q_hi
            assert at == c1 - c0
    assert [p[:2] for p in _group_panels(sg, off, nq)[0].tolist()] == [[0, 5], [5, 133], [133, 261], [261, 262], [262, 390], [390, 518], [518, 562], [562, 563]]


def test_grouped_recall_one_rank():
    from outfitx_amd.parallel import grouped_recall
    pos = torch.tensor([0, 3, 50, -1, 9, 49, 50, 4, -1, 14], dtype=torch.int32)
    got = grouped_recall(pos, 50, TOP_K)
    assert got == recall_ref(pos.numpy(), TOP_K) and list(got) == [f"Recall@{k}" for k in TOP_K]
    assert got["Recall@1"] == 1 / 8 and got["Recall@5"] == 3 / 8 and got["Recall@50"] == 6 / 8
    assert grouped_recall(torch.tensor([-1, -1]), 50, (1, 50)) == {"Recall@1": 0.0, "Recall@50": 0.0}
    assert grouped_recall(torch.empty(0, dtype=torch.int32), 50, (1,)) == {"Recall@1": 0.0}
    with pytest.raises(ValueError):
        grouped_recall(pos, 10, (1, 15))                        # a position beyond k = 10 is unknown


_RECALL_WORKER = r'''
import os, sys
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["OFX_ROOT"])
sys.path.insert(0, os.path.join(os.environ["OFX_ROOT"], "tests"))
from outfitx_amd.parallel import grouped_recall
from grouped_topk_ref import recall_ref
dist.init_process_group("gloo")
rank = dist.get_rank()
TOP_K = (1, 5, 10, 15, 30, 50)
# uneven shards: 5 queries (4 hits at 50) on rank 0, 11 (1 hit, one query without ground truth) on rank 1
parts = [torch.tensor([0, 2, 7, 50, 20]), torch.tensor([50, 50, 50, -1, 50, 0, 50, 50, 50, 50, 50])]
calls = []
orig = dist.all_reduce
def counting(t, *a, **k):
    calls.append((t.dtype, t.numel()))
    return orig(t, *a, **k)
dist.all_reduce = counting
got = grouped_recall(parts[rank], 50, TOP_K)
dist.all_reduce = orig
assert calls == [(torch.int64, len(TOP_K) + 1)], calls                 # ONE collective, integer counts
want = recall_ref(torch.cat(parts).numpy(), TOP_K)
assert got == want, (got, want)
own = [recall_ref(p.numpy(), TOP_K) for p in parts]
assert abs((own[0]["Recall@50"] + own[1]["Recall@50"]) / 2 - want["Recall@50"]) > 0.1       # the mean of the ranks' ratios is another number
dist.destroy_process_group()
print("rank", rank, "ok")
'''


def _run_world2(tmp_path, text):
    script = tmp_path / "worker.py"
    script.write_text(text)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OFX_ROOT=ROOT, OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.count("ok") == 2


def test_grouped_recall_world2_gloo_sums_counts_over_uneven_shards(tmp_path):
    _run_world2(tmp_path, _RECALL_WORKER)


def _valid_setup():
    """The stand-in module and batches of tests/test_cpu_cir_trainer.py, the two validation keys added, and 3 pools of 12-dim rows."""
    from test_cpu_cir_trainer import _COMMON
    ns = {}
    exec(_COMMON, ns)
    g = np.random.default_rng(21)
    off = [0, 9, 9 + 70, 9 + 70 + 64]                           # the first pool is smaller than k = 50
    P = g.standard_normal((off[-1], 12)).astype(np.float32)
    batches = ns["batches"](0, 8, 3, 8)
    for b in batches:
        grp = g.integers(0, 3, 8)
        b["pos_item_group"] = torch.from_numpy(grp)
        b["pos_item_row"] = [int(g.integers(0, off[c + 1] - off[c])) for c in grp]          # a list: host metadata
    return ns, torch.from_numpy(P), off, batches


def _host_topk(calls):
    def fn(Q, group_of_query, P, pool_offsets, k, gt=None):
        calls.append(len(Q))
        idx, d2, pos = grouped_topk_ref(Q.numpy(), np.asarray(group_of_query), P.numpy(), pool_offsets, k, None if gt is None else np.asarray(gt))
        return torch.from_numpy(idx), torch.from_numpy(np.sqrt(d2).astype(np.float32)), torch.from_numpy(pos)
    return fn


def test_cir_valid_epoch_loss_recall_and_training_flag():
    from outfitx_amd.losses import SetWiseRankingLoss
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    ns, P, off, batches = _valid_setup()
    loss_fn = SetWiseRankingLoss(margin=2.0)
    m = ns["Stub"]()
    tr = CIRTrainer(m, steps_per_epoch=3, cfg=CIRTrainConfig(learning_rate=1e-2, accumulation_steps=2, n_epochs=1), loss_fn=loss_fn)
    before = [p.detach().clone() for p in m.parameters()]
    # the hand-written loop (cir_trainer:122-172): eval, no gradients, summed loss / number of batches, all y_hat kept
    m.eval()
    with torch.no_grad():
        ys = [m(**b["input_dict"]) for b in batches]
        want_loss = sum(float(loss_fn(batch_y=b["pos_item_embedding"], batch_y_hat=y, batch_negative_samples=b["neg_items_embedding"],
                                      batch_negative_mask=b["neg_items_mask"])) for b, y in zip(batches, ys)) / len(batches)
    grp = np.concatenate([b["pos_item_group"].numpy() for b in batches])
    gt = np.asarray(off)[grp] + np.concatenate([np.asarray(b["pos_item_row"]) for b in batches])
    want = recall_ref(grouped_topk_ref(torch.cat(ys).numpy(), grp, P.numpy(), off, 50, gt)[2], TOP_K)

    for training in (True, False):
        m.train(training)
        calls = []
        out = tr.valid_epoch(batches, (P, off), topk_fn=_host_topk(calls))
        assert m.training is training                           # the flag is restored, whichever it was
        assert calls == [24]                                    # ONE retrieval over all collected queries
        assert list(out) == ["loss"] + [f"Recall@{k}" for k in TOP_K]
        assert abs(out["loss"] - want_loss) <= 1e-6 * abs(want_loss)
        assert {k: out[k] for k in want} == want
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), before)) and float(tr.grads.flat.abs().sum()) == 0.0

    def never(*a, **k):
        raise AssertionError("with_recall=False must not retrieve")
    m.train()
    out = tr.valid_epoch(batches, (P, off), with_recall=False, topk_fn=never)
    assert list(out) == ["loss"] and abs(out["loss"] - want_loss) <= 1e-6 * abs(want_loss) and m.training
    out = tr.valid_epoch(batches, None, with_recall=False)     # neither pools nor an engine are needed for the loss alone
    assert list(out) == ["loss"]
    # another top_k_list: k = its maximum
    ks = []
    def spy(Q, group_of_query, P_, pool_offsets, k, gt=None):
        ks.append(k)
        return _host_topk([])(Q, group_of_query, P_, pool_offsets, k, gt)
    assert list(tr.valid_epoch(batches, (P, off), top_k_list=(1, 7), topk_fn=spy)) == ["loss", "Recall@1", "Recall@7"] and ks == [7]


def test_cir_valid_epoch_without_an_engine_or_topk_fn_raises():
    """No quiet CPU retrieval: the default topk_fn is the HIP model's engine; the stand-in module has none."""
    from outfitx_amd._lib import OfxError
    from outfitx_amd.losses import SetWiseRankingLoss
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    ns, P, off, batches = _valid_setup()
    m = ns["Stub"]()
    tr = CIRTrainer(m, steps_per_epoch=3, cfg=CIRTrainConfig(n_epochs=1), loss_fn=SetWiseRankingLoss(margin=2.0))
    with pytest.raises(OfxError):
        tr.valid_epoch(batches, (P, off))
    assert m.training
