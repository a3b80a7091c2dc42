"""Index-form FITB on a real MI355X: ofx_fitb_argmin_indexed (outfitx_amd/csrc/scoring.hip, the TableCand instance of fitb_kernel) through
the C ABI, then FITBEvaluator / FITBDeviceSplit and CPTrainer.valid_epoch on the HIP model.

The indexed entry is the dense kernel's body reading its candidate rows through indices, so it is held three ways on integer-lattice
inputs (oracle.np_oracle.lattice: every fp32 partial sum of a squared distance is exact in any order): idx == fitb_argmin_exact on the
gathered rows, dist bit for bit == float32(sqrt(float64 d2)), and idx / dist torch.equal to ofx_fitb_argmin on the gathered rows.  The count
of correct answers is an integer and compared as one.  Outputs of raw calls are poisoned (-1 / NaN) first; the table has row stride D + 64
with NaN in the pad columns, so nothing may read them.  Model and loops are held to bit identity between the dense batches, the index batches
made on the host and the batches of a FITBDeviceSplit."""
import warnings

import numpy as np
import pytest
import torch

from oracle import np_oracle as O
from outfitx_amd import synth

warnings.simplefilter("ignore")
pytestmark = pytest.mark.gpu
OFX_EINVAL, OFX_ESHAPE = -1, -2
PAD = 64                                       # the table's row stride is D + PAD floats


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def f32_sqrt(d2):
    return np.sqrt(np.asarray(d2, np.float64)).astype(np.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def strided_table(table, lead=0, tail=0):
    """Device copy with row stride D + PAD inside a NaN-filled allocation of lead + n + tail rows -> (the view of the n rows, the allocation)."""
    n, D = table.shape
    whole = torch.full((lead + n + tail, D + PAD), float("nan"), device="cuda")
    whole[lead:lead + n, :D] = cu(table)
    return whole[lead:lead + n], whole


def indexed_call(tab, n_table, ci, y, D, answer_t=None, counter=None, with_dist=True, over=None):
    """ofx_fitb_argmin_indexed on device tensors -> (rc, idx, dist); idx poisoned with -1, dist with NaN.  `over` replaces single
    arguments (pointers as ints or None, sizes) to provoke a rejection."""
    from outfitx_amd import _lib as L
    lib = L.load()
    B, C = ci.shape
    idx = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    dist = torch.full((B, C), float("nan"), dtype=torch.float32, device="cuda") if with_dist else None
    a = dict(table=tab.data_ptr(), ld=tab.stride(0), n_table=n_table, cand_index=ci.data_ptr(), y_hat=y.data_ptr(), B=B, C=C, D=D,
             answer=None if answer_t is None else answer_t.data_ptr(), idx=idx.data_ptr(), dist=None if dist is None else dist.data_ptr(),
             n_correct=None if counter is None else counter.data_ptr())
    a.update(over or {})
    rc = lib.ofx_fitb_argmin_indexed(a["table"], a["ld"], a["n_table"], a["cand_index"], a["y_hat"], a["B"], a["C"], a["D"], a["answer"], a["idx"],
                                     a["dist"], a["n_correct"], stream())
    torch.cuda.synchronize()
    return rc, idx, dist


def dense_call(y, cand, with_dist=True):
    from outfitx_amd import _lib as L
    B, C, D = cand.shape
    idx = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    dist = torch.full((B, C), float("nan"), dtype=torch.float32, device="cuda") if with_dist else None
    rc = L.load().ofx_fitb_argmin(y.data_ptr(), cand.data_ptr(), B, C, D, idx.data_ptr(), None if dist is None else dist.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, idx, dist


def make_case(seed, B, C, D, n_rows, lo, hi):
    """table [n_rows, D], y [B, D] on the lattice, cand_index [B, C] int32.  Rows repeat within and across questions (n_rows is small
    against B * C); every third question's last candidate is its first again; every fifth question's y_hat IS its middle candidate, the
    last question's y_hat is its first two."""
    g = np.random.default_rng(seed)
    table, y = O.lattice(seed, n_rows, D, lo, hi), O.lattice(seed + 1000, B, D, lo, hi)
    ci = g.integers(0, n_rows, (B, C)).astype(np.int32)
    if C >= 2:
        ci[::3, C - 1] = ci[::3, 0]
        y[1::5] = table[ci[1::5, C // 2]]
        ci[B - 1, 1] = ci[B - 1, 0]
        y[B - 1] = table[ci[B - 1, 0]]
    return table, y, ci


# B, C, D, table rows, lo, hi
CASES = [(1, 1, 4, 1, -8, 8), (3, 2, 8, 5, -8, 8), (4, 4, 252, 6, -8, 8), (5, 4, 260, 11, -8, 8), (5, 7, 256, 9, -8, 8), (1030, 4, 1024, 300, -8, 8),
         (16385, 4, 8, 50, -8, 8), (2, 3, 4100, 7, -2, 2)]


@pytest.mark.parametrize("B,C,D,n_rows,lo,hi", CASES)
def test_indexed_fitb_is_exact_on_the_lattice_and_returns_the_bits_of_the_dense_call(B, C, D, n_rows, lo, hi):
    table, y, ci = make_case(B + C + D, B, C, D, n_rows, lo, hi)
    rows = table[ci]                                                          # what the dense entry is fed
    ei, ed2 = O.fitb_argmin_exact(y, rows)
    answer = np.where(np.arange(B) % 2 == 0, ei, (ei + 1) % max(C, 2))        # even questions right, odd ones wrong (C = 1: answer 1 never is)
    want_hits = int((ei == answer).sum())
    assert want_hits == (B + 1) // 2
    tab, _ = strided_table(table)
    yd, cid, ad = cu(y), cu(ci), cu(answer.astype(np.int64))
    rc_d, idx_d, dist_d = dense_call(yd, cu(rows))
    assert rc_d == 0
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    calls = 0
    for with_dist in (True, False):
        for with_answer in (False, True):
            rc, idx, dist = indexed_call(tab, n_rows, cid, yd, D, ad if with_answer else None, counter if with_answer else None, with_dist)
            calls += with_answer
            assert rc == 0
            assert np.array_equal(idx.cpu().numpy(), ei) and torch.equal(idx, idx_d)
            if with_dist:
                assert np.array_equal(dist.cpu().numpy().view(np.uint32), f32_sqrt(ed2).view(np.uint32))
                assert torch.equal(bits(dist), bits(dist_d))
            assert int(counter) == calls * want_hits, (with_dist, with_answer, int(counter), want_hits)      # it accumulates
    if C >= 2:
        d = dist_d.cpu().numpy()
        assert ei[B - 1] == 0 and d[B - 1, 0].view(np.uint32) == 0 and d[B - 1, 1].view(np.uint32) == 0      # exact hits: +0.0, the first wins
        dup = np.setdiff1d(np.arange(0, B - 1, 3), np.arange(1, B, 5))
        assert (ei[dup] != C - 1).all() and (ed2[dup, 0] == ed2[dup, C - 1]).all()                         # the later copy never wins
    # two calls with different answers into one counter: the sum of the two expected counts
    other = (answer + 1) % max(C, 2)
    counter.zero_()
    for a in (answer, other):
        assert indexed_call(tab, n_rows, cid, yd, D, cu(a.astype(np.int64)), counter, False)[0] == 0
    assert int(counter) == want_hits + int((ei == other).sum())


def test_engine_wrapper_returns_the_raw_call_and_checks_host_indices():
    from outfitx_amd.engine import fitb_argmin, fitb_argmin_indexed
    B, C, D, n_rows = 37, 4, 1024, 20
    table, y, ci = make_case(5, B, C, D, n_rows, -8, 8)
    tab, _ = strided_table(table)
    ei, _ = O.fitb_argmin_exact(y, table[ci])
    want = fitb_argmin(cu(y), cu(table[ci]), return_dist=True)
    hits = torch.zeros(1, dtype=torch.int32, device="cuda")
    for index in (torch.from_numpy(ci), cu(ci), cu(ci).long()):                # host int32, device int32, device int64
        idx, dist = fitb_argmin_indexed(tab[:, :D], index, cu(y), answer=torch.from_numpy(ei), n_correct=hits, return_dist=True)
        assert torch.equal(idx, want[0]) and torch.equal(bits(dist), bits(want[1]))
    assert int(hits) == 3 * B
    assert torch.equal(fitb_argmin_indexed(tab[:, :D], cu(ci), cu(y)), want[0])
    bad = torch.from_numpy(ci).clone()
    bad[3, 1] = n_rows
    with pytest.raises(IndexError):
        fitb_argmin_indexed(tab[:, :D], bad, cu(y))
    with pytest.raises(ValueError):
        fitb_argmin_indexed(tab[:, :D], cu(ci), cu(y), answer=torch.from_numpy(ei))        # answer without n_correct
    # a table the kernel cannot read in place is refused, not copied: a column slice off the 16-byte grid, another dtype, a host table
    for bad_table in (tab[:, 2:D + 2], tab[:, :D].double(), tab[:, :D].cpu()):
        with pytest.raises(ValueError, match="fitb_argmin_indexed: the table must be"):
            fitb_argmin_indexed(bad_table, cu(ci), cu(y))


def test_indices_outside_the_table_are_clamped_into_it():
    """The table is a view that starts 8 rows inside a NaN-filled allocation and is followed by 8 more NaN rows; n_table = 16.  Indices -5
    and n_table + 3 then address poison INSIDE the allocation: a missing clamp gives NaN distances and fails the comparison, it cannot
    fault.  Expected: the result of the clamped rows 0 and n_table - 1."""
    B, C, D, n = 6, 4, 256, 16
    table, y, ci = make_case(9, B, C, D, n, -8, 8)
    tab, whole = strided_table(table, lead=8, tail=8)
    assert whole.shape[0] == 32 and tab.data_ptr() == whole.data_ptr() + 8 * whole.stride(0) * 4
    ci[0, 1] = -5; ci[2, 0] = n + 3; ci[3, 3] = -5; ci[5, 2] = n + 3; ci[4] = (-5, n + 3, -1, n)
    clamped = np.clip(ci, 0, n - 1)
    ei, ed2 = O.fitb_argmin_exact(y, table[clamped])
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc, idx, dist = indexed_call(tab, n, cu(ci), cu(y), D, cu(ei), counter)
    assert rc == 0
    assert np.array_equal(idx.cpu().numpy(), ei) and int(counter) == B
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), f32_sqrt(ed2).view(np.uint32))
    rc_d, idx_d, dist_d = dense_call(cu(y), cu(table[clamped]))
    assert rc_d == 0 and torch.equal(idx, idx_d) and torch.equal(bits(dist), bits(dist_d))


def test_a_gathered_row_with_a_nan_follows_the_dense_kernels_rule():
    """torch.cdist(...).argmin(-1) returns the index of the first NaN; +inf is an ordinary (largest) number."""
    B, C, D, n = 9, 5, 260, 30
    table, y, _ = make_case(13, B, C, D, n, -8, 8)
    ci = np.stack([np.random.default_rng(b).permutation(20)[:C] for b in range(B)]).astype(np.int32)      # clean rows 0..19, distinct per question
    table[20, 7] = np.nan; table[21, 259] = np.nan; table[22, 0] = np.inf
    ei, _ = O.fitb_argmin_exact(y, table[ci])
    want = ei.copy()
    ci[0, 3] = 20; want[0] = 3                                    # one NaN row
    ci[1, 4] = 20; ci[1, 2] = 21; want[1] = 2                     # two: the first
    ci[2, 0] = 21; want[2] = 0
    ci[3, :] = 20; want[3] = 0                                    # every distance NaN: the first
    ci[4, (ei[4] + 1) % C] = 22                                   # a +inf distance beside the minimum changes nothing
    ci[5, :] = 22; want[5] = 0                                    # every distance +inf: the first
    y[6, 9] = np.nan; want[6] = 0                                 # NaN in y_hat
    tab, _ = strided_table(table)
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    for with_dist in (False, True):
        rc, idx, dist = indexed_call(tab, n, cu(ci), cu(y), D, cu(want), counter, with_dist)
        assert rc == 0 and np.array_equal(idx.cpu().numpy(), want)
    assert int(counter) == 2 * B
    rc_d, idx_d, dist_d = dense_call(cu(y), cu(table[ci]))
    assert rc_d == 0 and torch.equal(idx, idx_d) and torch.equal(bits(dist), bits(dist_d))
    d = dist.cpu().numpy()
    assert np.isnan(d[0, 3]) and np.isnan(d[1, [2, 4]]).all() and np.isnan(d[3]).all() and np.isinf(d[5]).all() and np.isnan(d[6]).all()
    assert np.isfinite(np.delete(d[0], 3)).all() and np.isfinite(d[[7, 8]]).all()


def test_indexed_fitb_rejects_what_it_cannot_run_and_launches_nothing():
    from outfitx_amd import _lib as L
    lib = L.load()
    B, C, D, n = 4, 3, 64, 10
    table, y, ci = make_case(17, B, C, D, n, -8, 8)
    tab, _ = strided_table(table)
    yd, cid = cu(y), cu(ci)
    y4 = cu(np.concatenate([np.zeros(1, np.float32), y.ravel()]))
    assert y4.data_ptr() % 16 == 0
    ans = torch.zeros(B, dtype=torch.int64, device="cuda")
    cases = [(dict(table=None), OFX_EINVAL), (dict(cand_index=None), OFX_EINVAL), (dict(y_hat=None), OFX_EINVAL), (dict(idx=None), OFX_EINVAL),
             (dict(n_correct=None), OFX_EINVAL), (dict(answer=None), OFX_EINVAL),
             (dict(table=tab.data_ptr() + 4), OFX_EINVAL), (dict(y_hat=y4.data_ptr() + 4), OFX_EINVAL),
             (dict(B=0), OFX_ESHAPE), (dict(C=0), OFX_ESHAPE), (dict(D=6), OFX_ESHAPE), (dict(D=62), OFX_ESHAPE), (dict(ld=D - 4), OFX_ESHAPE),
             (dict(ld=D + 2), OFX_ESHAPE), (dict(n_table=0), OFX_ESHAPE), (dict(n_table=-3), OFX_ESHAPE), (dict(n_table=2 ** 31), OFX_ESHAPE)]
    for kw, code in cases:
        counter = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc, idx, dist = indexed_call(tab, n, cid, yd, D, ans, counter, True, over=kw)
        assert rc == code and b"fitb_argmin_indexed" in lib.ofx_last_error(), (kw, rc, lib.ofx_last_error())
        assert bool((idx == -1).all()) and bool(torch.isnan(dist).all()) and int(counter) == -1, kw      # the poisoned outputs are untouched
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc, idx, dist = indexed_call(tab, n, cid, yd, D, ans, counter)                                       # and the same call, unspoiled, runs
    ei, _ = O.fitb_argmin_exact(y, table[ci])
    assert rc == 0 and np.array_equal(idx.cpu().numpy(), ei) and int(counter) == int((ei == 0).sum())


# ------------------------------------------------------------------------------------------------ model and loops
@pytest.fixture(scope="module")
def model():
    """One one-layer model for both loop tests (building it is most of their time); neither changes what the other reads."""
    return make_model()


def make_model(n_layers=1):
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    from conftest import W_SEED
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    cfg.transformer.dropout = 0.0
    cfg.transformer.n_layers = n_layers
    m = OutfitX(cfg, train_precision="f16")
    sd = {k: torch.from_numpy(v) for k, v in synth.full_state_dict(W_SEED).items()}
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()}, strict=True)     # a shallower model takes the first layers
    return m.cuda()


def trainable(m):
    return {k: v for k, v in m.named_parameters() if not k.startswith("item_encoder.")}


def padded(table, rows, cu_items, L=16):
    B = len(cu_items) - 1
    emb = np.zeros((B, L, table.shape[1]), np.float32); mask = np.ones((B, L), bool)
    for b in range(B):
        n = cu_items[b + 1] - cu_items[b]
        emb[b, :n] = table[rows[cu_items[b]:cu_items[b + 1]]]
        mask[b, :n] = False
    return torch.from_numpy(emb), torch.from_numpy(mask)


class Recorder:
    """Collects what the model returned and what the scoring entries returned while a loop runs."""

    def __init__(self, model, monkeypatch=None):
        self.y, self.idx = [], []
        self.handle = model.register_forward_hook(lambda mod, args, out: self.y.append(out.detach().clone()))
        if monkeypatch is not None:
            from outfitx_amd import engine
            for name in ("fitb_argmin", "fitb_argmin_indexed"):
                fn = getattr(engine, name)
                monkeypatch.setattr(engine, name, lambda *a, _fn=fn, **k: self._keep(_fn(*a, **k)))

    def _keep(self, idx):
        self.idx.append(idx.clone())
        return idx

    def close(self):
        self.handle.remove()
        return torch.cat(self.y), (torch.cat(self.idx) if self.idx else None)


def test_fitb_evaluator_index_dense_and_device_split_batches_agree_bit_for_bit(model, monkeypatch):
    """6 questions of 2 to 8 items over a 40-row table, 4 candidates each, two batches of 3."""
    from outfitx_amd.engine import fitb_argmin
    from outfitx_amd.sampler import FITBDeviceSplit
    from outfitx_amd.trainer import FITBEvaluator
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    N, C, n_rows = 6, 4, 40
    g = np.random.default_rng(21)
    table = synth.item_embeddings(21, "table", n_rows)
    n_items = np.array([2, 8, 5, 3, 7, 4])
    cu_items = np.concatenate([[0], np.cumsum(n_items)]).astype(np.int32)
    rows = g.integers(0, n_rows, int(cu_items[-1])).astype(np.int32)
    cand = np.stack([g.permutation(n_rows)[:C] for _ in range(N)]).astype(np.int32)
    m = model.eval()
    m.set_embedding_table(torch.from_numpy(table))
    emb, mask = padded(table, rows, cu_items)
    # the answer's text embedding enters the model: try all four, take one the model then picks for even questions, one it misses for odd ones
    pick = np.empty((N, C), np.int64)
    with torch.no_grad():
        for a in range(C):
            y = m(task=CIR, outfit_embedding=emb.cuda(), outfit_mask=mask.cuda(), target_item_text_embedding=cu(table[cand[:, a], 512:]))
            pick[:, a] = fitb_argmin(y, cu(table[cand])).cpu().numpy()
    ans = np.empty(N, np.int64)
    for b in range(N):
        good, bad = [a for a in range(C) if pick[b, a] == a], [a for a in range(C) if pick[b, a] != a]
        ans[b] = ((good or bad) if b % 2 == 0 else (bad or good))[0]
    target = cand[np.arange(N), ans].astype(np.int32)
    want_idx = pick[np.arange(N), ans]
    want_acc = float((want_idx == ans).sum()) / N
    assert 0.0 < want_acc < 1.0, (pick, ans)
    t = torch.from_numpy
    index_b, dense_b = [], []
    for q0, q1 in ((0, 3), (3, 6)):
        i0, i1 = cu_items[q0], cu_items[q1]
        index_b.append({"input_dict": {"task": CIR, "item_index": t(rows[i0:i1].copy()), "cu_seqlens": t(cu_items[q0:q1 + 1] - i0),
                                       "target_item_index": t(target[q0:q1].copy())},
                        "candidate_item_index": t(cand[q0:q1].copy()), "answer_index": t(ans[q0:q1].copy())})
        dense_b.append({"input_dict": {"task": CIR, "outfit_embedding": emb[q0:q1], "outfit_mask": mask[q0:q1],
                                       "target_item_text_embedding": t(np.ascontiguousarray(table[target[q0:q1], 512:]))},
                        "candidate_item_embedding": t(table[cand[q0:q1]]), "answer_index": t(ans[q0:q1].copy())})
    split = FITBDeviceSplit(rows, cu_items, cand, ans, n_table=n_rows)
    assert len(split) == N and split.steps(3) == 2
    first = next(iter(split.batches(3)))
    assert all(v.is_cuda for k, v in first["input_dict"].items() if k != "task") and first["candidate_item_index"].is_cuda
    assert first["input_dict"]["cu_seqlens"].tolist() == cu_items[:4].tolist() and first["input_dict"]["target_item_index"].tolist() == target[:3].tolist()
    runs = {}
    for name, batches in (("index", index_b), ("dense", dense_b), ("split", split.batches(3))):
        m.train()                                          # the evaluator switches to eval mode and back
        rec = Recorder(m, monkeypatch)
        out = FITBEvaluator(m).test_epoch(batches)
        monkeypatch.undo()
        y, idx = rec.close()
        assert m.training and list(out) == ["Accuracy"]
        runs[name] = (y, idx, out["Accuracy"])
    yi, ii, ai = runs["index"]
    assert yi.shape == (N, 1024) and torch.isfinite(yi).all()
    assert np.array_equal(ii.cpu().numpy(), want_idx) and ai == want_acc
    for name in ("dense", "split"):
        y, idx, acc = runs[name]
        assert torch.equal(y, yi) and torch.equal(idx, ii) and acc == ai, name
    # ragged last batch and a rank's share of the batches
    assert [b["answer_index"].numel() for b in split.batches(4)] == [4, 2]
    assert [b["answer_index"].tolist() for b in split.batches(2, rank=1, world=2)] == [ans[2:4].tolist()]
    assert FITBEvaluator(m).test_epoch(split.batches(4)) == {"Accuracy": want_acc}
    with pytest.raises(ValueError):
        FITBDeviceSplit(rows, cu_items, cand, ans, n_table=int(max(rows.max(), cand.max())))             # the largest row is outside such a table


def test_cp_valid_epoch_on_the_hip_model_dense_and_indexed(model):
    """2 batches of 4 outfits.  The loop's logits are those of direct eval-mode calls, bit for bit; its metrics are gather_epoch of them;
    parameters, optimizer state and the gradient arena stay as a training step left them; the training flag is restored."""
    from outfitx_amd.losses import FocalLoss
    from outfitx_amd.trainer import CPTrainConfig, CPTrainer, gather_epoch
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    n_rows = 40
    g = np.random.default_rng(33)
    table = synth.item_embeddings(33, "table", n_rows)
    t = torch.from_numpy
    forms = {"indexed": [], "dense": []}
    for s in range(2):
        n_items = g.integers(1, 9, 4)
        cu_items = np.concatenate([[0], np.cumsum(n_items)]).astype(np.int32)
        rows = g.integers(0, n_rows, int(cu_items[-1])).astype(np.int32)
        lab = t(np.array([1, 0, 0, 1] if s == 0 else [0, 1, 1, 0], np.float32))
        emb, mask = padded(table, rows, cu_items)
        forms["indexed"].append({"input_dict": {"task": CP, "item_index": t(rows), "cu_seqlens": t(cu_items)}, "label": lab})
        forms["dense"].append({"input_dict": {"task": CP, "outfit_embedding": emb, "outfit_mask": mask}, "label": lab})
    m = model
    m.set_embedding_table(t(table))
    tr = CPTrainer(m, steps_per_epoch=2, cfg=CPTrainConfig(learning_rate=2e-5, accumulation_steps=1, n_epochs=1), params=list(trainable(m).values()))
    m.train()
    tr.grads.zero_()
    tr.micro_step(forms["dense"][0], 0)                                         # one optimizer step: there is state to guard
    tr.grads.flat.copy_(torch.arange(tr.grads.flat.numel(), dtype=torch.float32, device="cuda") % 7)      # an arena in the middle of a window
    snap = lambda: ([p.detach().clone() for p in trainable(m).values()], tr.grads.flat.clone(),
                    [v.clone() for s in tr.optimizer.state.values() for v in s.values() if isinstance(v, torch.Tensor)], tr.scheduler.get_last_lr())
    before = snap()
    assert before[2]
    loss_fn = FocalLoss(alpha=0.75, gamma=2.0, reduction="mean")
    results = {}
    for name, batches in forms.items():
        m.eval()
        with torch.no_grad():
            direct = [m(**{k: (v if k == "task" else v.cuda()) for k, v in b["input_dict"].items()}).squeeze(-1) for b in batches]
            total = sum(loss_fn(y_hat=y, y_true=b["label"].cuda()) for y, b in zip(direct, batches))
        labels = torch.cat([b["label"] for b in batches]).cuda()
        want = gather_epoch(torch.cat(direct), labels, total, 2)
        for training in (True, False):
            m.train(training)
            rec = Recorder(m)
            valid = tr.valid_epoch(batches)
            y, _ = rec.close()
            test = tr.test_epoch(iter(batches))
            assert m.training is training
            assert torch.equal(y.squeeze(-1), torch.cat(direct)), name
            assert list(valid) == ["loss", "Accuracy", "Precision", "Recall", "F1", "AUC"] and valid == want, (name, valid, want)
            assert test == {k: v for k, v in want.items() if k != "loss"}
        results[name] = (torch.cat(direct), valid)
    assert torch.equal(results["indexed"][0], results["dense"][0]) and results["indexed"][1] == results["dense"][1]
    assert np.isfinite(list(results["dense"][1].values())).all()
    after = snap()
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0])) and torch.equal(before[1], after[1])
    assert len(before[2]) == len(after[2]) and all(torch.equal(a, b) for a, b in zip(before[2], after[2])) and before[3] == after[3]
