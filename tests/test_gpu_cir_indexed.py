"""Index-form CIR batches on a real MI355X: ofx_set_rank_loss_indexed (outfitx_amd/csrc/rank_loss.hip, the TableRows instances of the
rank-loss kernels), OutfitX's `target_item_index`, and CIRTrainer fed by index batches.

The indexed loss is the dense kernel's body reading its rows through indices, so it is held to BIT identity with ofx_set_rank_loss on the
gathered rows (torch.equal on loss, dy_hat, d_pos and d_neg, nothing left out), and additionally to the float64 restatement of
tests/test_gpu_rank_loss.py under that file's own bounds.  Model and trainer are held to bit identity with the dense batches gathered from
the same rows.  Outputs of raw calls are poisoned with NaN first."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from conftest import W_SEED
from outfitx_amd import synth
from test_gpu_rank_loss import abi_call, compare, ref_rank_loss

warnings.simplefilter("ignore")
pytestmark = pytest.mark.gpu
OFX_EINVAL, OFX_ESHAPE, OFX_EWORKSPACE = -1, -2, -4
PAD = 64                                       # the table's row stride is D + PAD floats


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wide_rows(seed, tag, n, D):
    """[n, D] item-encoder-shaped rows * 3 (the scale tests/test_gpu_rank_loss.py feeds), D up to 4096."""
    parts = [synth.item_embeddings(seed, f"{tag}{j}", n) for j in range((D + 1023) // 1024)]
    return np.ascontiguousarray(np.concatenate(parts, 1)[:, :D] * 3.0)


def make_case(seed, B, K, D, n_rows, distinct=False):
    """table [n_rows, D], y_hat [B, D], pos [B], neg [B, K] int32.  Rows repeat within and across queries, one negative equals its query's
    positive, about 20 % of the slots are padded (-1); distinct=True draws a query's negatives without repetition and never its positive
    (exact ties and hinges at exactly the margin are where the float64 comparison leaves rows out)."""
    g = np.random.default_rng(seed)
    table, y_hat = wide_rows(seed, "table", n_rows, D), wide_rows(seed, "y_hat", B, D)
    pos = g.integers(0, n_rows, B).astype(np.int32)
    if distinct:
        neg = np.stack([(lambda p: p[p != pos[b]][:K])(g.permutation(n_rows)) for b in range(B)]).astype(np.int32).reshape(B, K)
    else:
        neg = g.integers(0, n_rows, (B, K)).astype(np.int32)
        if K >= 3:
            neg[:, 2] = neg[:, 0]                                              # the same row twice within a query
    if K >= 2:
        if not distinct:
            neg[0, 1] = pos[0]                                                 # a negative that is the positive
        neg[g.random((B, K)) < 0.2] = -1
    return table, y_hat, pos, neg


def gathered(table, pos, neg):
    """What the dense entry is fed: y, neg rows (row 0 stands in for a padded slot: never loaded), mask."""
    return table[pos], table[np.maximum(neg, 0)], neg < 0


def strided_table(table, rows=None):
    """Device copy with row stride D + PAD; the pad columns hold NaN: nothing may read them."""
    n, D = table.shape
    t = torch.full((rows or n, D + PAD), float("nan"), device="cuda")
    t[:n, :D] = cu(table)
    return t


def indexed_call(tab, n_table, pos, neg, y_hat, K, margin, upstream=1.0, want_grad=True, want_d=True, ws_bytes=None, ld=None, table_ptr=None,
                 null_pos=False):
    """ofx_set_rank_loss_indexed on a device table -> (rc, loss, dy, d_pos, d_neg), outputs poisoned with NaN first."""
    from outfitx_amd import _lib as L
    lib = L.load()
    B, D = y_hat.shape
    th, tp = cu(y_hat), cu(np.asarray(pos, np.int32))
    tn = cu(np.asarray(neg, np.int32)) if K else None
    loss = torch.full((), float("nan"), device="cuda")
    dy = torch.full_like(th, float("nan")) if want_grad else None
    dp = torch.full((B,), float("nan"), device="cuda") if want_d else None
    dn = torch.full((B, max(K, 1)), float("nan"), device="cuda") if want_d else None
    n = lib.ofx_set_rank_loss_ws_bytes(B, K, D) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.ofx_set_rank_loss_indexed(tab.data_ptr() if table_ptr is None else table_ptr, tab.stride(0) if ld is None else ld, n_table,
                                       None if null_pos else p(tp), p(tn), p(th), B, K, D, C.c_float(margin), C.c_float(upstream), p(loss), p(dy),
                                       p(dp), p(dn), p(ws), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, loss, dy, dp, (dn[:, :K] if dn is not None else None)


def same_bits(a, b):
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


# (B, K, D, table rows): the path each reaches is in the id
SHAPES = [pytest.param(3, 10, 1024, 12, id="resident-nv1"), pytest.param(5, 11, 1024, 20, id="not_resident-reread_through_indices"),
          pytest.param(4, 40, 256, 30, id="resident-two_chunks"), pytest.param(2, 3, 2048, 5, id="nv2"), pytest.param(2, 2, 4096, 4, id="nv4"),
          pytest.param(300, 2, 64, 50, id="last_block_reduction_over_300_rows"), pytest.param(3, 0, 1024, 6, id="k0-null_neg_index")]


@pytest.mark.parametrize("B,K,D,n_rows", SHAPES)
def test_indexed_entry_returns_the_bits_of_the_dense_entry_on_the_gathered_rows(B, K, D, n_rows):
    table, y_hat, pos, neg = make_case(60 + K, B, K, D, n_rows)
    if (B, K) == (3, 10):
        neg[1] = -1                                                            # one row fully padded
        neg[2] = np.abs(neg[2]); neg[2, 4] = -1                                # one entry padded
    tab = strided_table(table)
    y, nrows, mask = gathered(table, pos, neg)
    for margin in (2.0, 0.0):
        want = abi_call(y, y_hat, nrows if K else None, mask if K else None, margin, shape=(B, K, D))
        got = indexed_call(tab, n_rows, pos, neg, y_hat, K, margin)
        assert want[0] == 0 and got[0] == 0
        for name, u, v in zip(("loss", "dy_hat", "d_pos", "d_neg"), got[1:], want[1:]):
            assert torch.equal(u, v), (margin, name, (u - v).abs().max())
        assert torch.isfinite(got[1]) and torch.isfinite(got[2]).all()
        if K:
            assert torch.equal(torch.isinf(got[4]).cpu(), torch.from_numpy(mask))
    # upstream != 1, no gradient wanted, no distances wanted: each the dense call's bits again; two calls: the same bits
    for kw in (dict(upstream=0.37), dict(want_grad=False), dict(want_d=False), dict(upstream=0.25, want_grad=False, want_d=False)):
        want = abi_call(y, y_hat, nrows if K else None, mask if K else None, 2.0, shape=(B, K, D), **kw)
        got = indexed_call(tab, n_rows, pos, neg, y_hat, K, 2.0, **kw)
        again = indexed_call(tab, n_rows, pos, neg, y_hat, K, 2.0, **kw)
        assert got[0] == 0 and same_bits(got[1:], want[1:]) and same_bits(got[1:], again[1:]), kw


@pytest.mark.parametrize("B,K,D,n_rows", SHAPES[:3])
def test_indexed_entry_against_the_float64_restatement(B, K, D, n_rows):
    """tests/test_gpu_rank_loss.py's float64 restatement, TOL and cap on rows left out near a hinge or a tie.  A query's negatives are
    distinct rows here: the same row twice is an exact tie of two distances, which that file's rule leaves out when it is the hardest."""
    table, y_hat, pos, neg = make_case(80 + K, B, K, D, max(n_rows, K + 1), distinct=True)
    tab = strided_table(table)
    y, nrows, mask = gathered(table, pos, neg)
    for margin in (2.0, 0.0):
        r = ref_rank_loss(y, y_hat, nrows, mask, margin)
        rc, loss, dy, dp, dn = indexed_call(tab, len(table), pos, neg, y_hat, K, margin)
        assert rc == 0
        compare(f"indexed B{B} K{K} D{D} margin {margin}", r, loss, dy, dp, dn)


def test_indices_outside_the_table_are_clamped_into_it():
    """64 rows allocated, n_table = 32: indices 32..63 and a pos_index of -1 give the bits of the call with the indices clamped to [0, 31].
    Every address an unclamped kernel would touch is inside the allocation (row -1 is kept inside by a leading row), so a missing clamp
    fails the comparison instead of faulting."""
    B, K, D = 4, 6, 1024
    table, y_hat, _, _ = make_case(7, B, K, D, 65)
    whole = strided_table(table)
    tab = whole[1:]                                                            # row -1 of `tab` is row 0 of the allocation
    pos = np.array([-1, 40, 63, 5], np.int32)
    neg = np.random.default_rng(7).integers(32, 64, (B, K)).astype(np.int32)
    neg[0, :2] = (3, 31)
    neg[1, 3] = -1                                                             # stays padded: a negative neg_index is never clamped to a row
    neg[2, 5] = -5
    got = indexed_call(tab, 32, pos, neg, y_hat, K, 2.0)
    want = indexed_call(tab, 32, np.clip(pos, 0, 31), np.where(neg < 0, neg, np.minimum(neg, 31)), y_hat, K, 2.0)
    assert got[0] == 0 and want[0] == 0 and same_bits(got[1:], want[1:])
    assert torch.equal(torch.isinf(got[4]).cpu(), torch.from_numpy(neg < 0))
    dense = abi_call(*(lambda t: (t[np.clip(pos, 0, 31)], y_hat, t[np.clip(neg, 0, 31)], neg < 0))(table[1:]), 2.0)
    assert same_bits(got[1:], dense[1:])
    unclamped = indexed_call(tab, 64, pos.clip(0), neg, y_hat, K, 2.0)         # the rows 32..63 differ from row 31: the clamp changed the result
    assert not torch.equal(unclamped[4], got[4])


def test_indexed_entry_rejects_what_it_cannot_run_and_launches_nothing():
    from outfitx_amd import _lib as L
    lib = L.load()
    B, K, D = 4, 6, 1024
    table, y_hat, pos, neg = make_case(8, B, K, D, 16)
    tab = strided_table(table)
    ws = lib.ofx_set_rank_loss_ws_bytes(B, K, D)
    cases = [(dict(table_ptr=tab.data_ptr() + 4), OFX_EINVAL), (dict(null_pos=True), OFX_EINVAL), (dict(ld=D - 4), OFX_ESHAPE),
             (dict(ld=D + 2), OFX_ESHAPE), (dict(n_table=0), OFX_ESHAPE), (dict(n_table=2 ** 31), OFX_ESHAPE), (dict(ws_bytes=ws - 16), OFX_EWORKSPACE)]
    for kw, code in cases:
        kw = dict(kw)
        rc, loss, dy, dp, dn = indexed_call(tab, kw.pop("n_table", 16), pos, neg, y_hat, K, 2.0, **kw)
        assert rc == code and b"set_rank_loss_indexed" in lib.ofx_last_error(), (kw, rc, lib.ofx_last_error())
        assert all(torch.isnan(t).all() for t in (loss, dy, dp, dn)), kw       # the poisoned outputs are untouched
    # the engine wrapper has no CPU form
    from outfitx_amd.engine import set_rank_loss_indexed
    with pytest.raises(L.OfxError):
        set_rank_loss_indexed(torch.from_numpy(table), torch.from_numpy(pos), torch.from_numpy(neg), torch.from_numpy(y_hat), 2.0)   # CPU tensors
    # and the accepted call on the same buffers; the engine wrapper and the loss class return its bits
    rc, loss, dy, _, _ = indexed_call(tab, 16, pos, neg, y_hat, K, 2.0)
    assert rc == 0
    l_e, dy_e = set_rank_loss_indexed(tab[:, :D], cu(pos), cu(neg), cu(y_hat), 2.0)
    assert torch.equal(l_e, loss) and torch.equal(dy_e, dy)
    assert set_rank_loss_indexed(tab[:, :D], cu(pos), cu(neg), cu(y_hat), 2.0, need_grad=False)[1] is None
    from outfitx_amd.losses import SetWiseRankingLoss
    th = cu(y_hat).requires_grad_(True)
    l_c = SetWiseRankingLoss(margin=2.0).forward_indexed(th, tab[:, :D], cu(pos), cu(neg))
    assert "SetRankIndexed" in type(l_c.grad_fn).__name__, type(l_c.grad_fn).__name__       # the kernel, not the gather
    (l_c * 0.5).backward()
    assert torch.equal(l_c.detach(), loss) and torch.equal(th.grad, dy * 0.5)
    # other dtypes take the gather + forward() path: int64 indices here, the dense kernel underneath - the same bits again
    l_g = SetWiseRankingLoss(margin=2.0).forward_indexed(cu(y_hat), tab[:, :D], cu(pos).long(), cu(neg).long())
    assert torch.equal(l_g, loss)


# ------------------------------------------------------------------------------------------------ model and trainer
def make_model(n_layers=1):
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    cfg.transformer.dropout = 0.0
    cfg.transformer.n_layers = n_layers
    m = OutfitX(cfg, train_precision="f16")
    sd = {k: torch.from_numpy(v) for k, v in synth.full_state_dict(W_SEED).items()}
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()}, strict=True)     # a shallower model takes the first layers
    return m.cuda().train()


def trainable(m):
    return {k: v for k, v in m.named_parameters() if not k.startswith("item_encoder.")}


def index_batch(g, table, B, K, CIR):
    """One micro-batch in both forms: the index batch, and the dense batch gathered from the same rows."""
    n_rows = len(table)
    n_items = g.integers(0, 13, B)
    n_items[0] = 16
    idx = g.integers(0, n_rows, int(n_items.sum())).astype(np.int32)
    cu_items = np.concatenate([[0], np.cumsum(n_items)]).astype(np.int32)
    pos = g.integers(0, n_rows, B).astype(np.int32)
    neg = g.integers(0, n_rows, (B, K)).astype(np.int32)
    neg[g.random((B, K)) < 0.2] = -1
    neg[1] = -1
    emb = np.zeros((B, 16, 1024), np.float32); mask = np.ones((B, 16), bool)
    for b in range(B):
        emb[b, :n_items[b]] = table[idx[cu_items[b]:cu_items[b + 1]]]
        mask[b, :n_items[b]] = False
    t = torch.from_numpy
    indexed = {"input_dict": {"task": CIR, "item_index": t(idx), "cu_seqlens": t(cu_items), "target_item_index": t(pos)},
               "pos_item_index": t(pos), "neg_items_index": t(neg)}
    dense = {"input_dict": {"task": CIR, "outfit_embedding": t(emb), "outfit_mask": t(mask),
                            "target_item_text_embedding": t(np.ascontiguousarray(table[pos, 512:]))},
             "pos_item_embedding": t(table[pos]), "neg_items_embedding": t(table[np.maximum(neg, 0)]), "neg_items_mask": t(neg < 0)}
    return indexed, dense


def test_model_takes_the_target_by_table_row():
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    table = synth.item_embeddings(8, "table", 300)
    ib, db = index_batch(np.random.default_rng(8), table, 6, 3, CIR)
    ind, dd = {k: (v if k == "task" else v.cuda()) for k, v in ib["input_dict"].items()}, {k: (v if k == "task" else v.cuda()) for k, v in db["input_dict"].items()}
    txt, tix = dd["target_item_text_embedding"], ind["target_item_index"]
    m = make_model()
    # no table yet: an index cannot be resolved, with the dense set either
    with pytest.raises(ValueError):
        m(task=CIR, outfit_embedding=dd["outfit_embedding"], outfit_mask=dd["outfit_mask"], target_item_index=tix)
    m.set_embedding_table(torch.from_numpy(table))
    with pytest.raises(ValueError):
        m(task=CIR, item_index=ind["item_index"], cu_seqlens=ind["cu_seqlens"], target_item_text_embedding=txt, target_item_index=tix)
    sets = {"indexed": dict(item_index=ind["item_index"], cu_seqlens=ind["cu_seqlens"]),
            "dense": dict(outfit_embedding=dd["outfit_embedding"], outfit_mask=dd["outfit_mask"])}
    up = torch.linspace(-1.0, 2.0, 6).cuda()[:, None]
    for name, s in sets.items():
        m.eval()
        with torch.no_grad():
            assert torch.equal(m(task=CIR, target_item_index=tix, **s), m(task=CIR, target_item_text_embedding=txt, **s)), name
        m.train()
        grads = []
        for kw in (dict(target_item_text_embedding=txt), dict(target_item_index=tix)):
            m.zero_grad(set_to_none=True)
            y = m(task=CIR, **kw, **s)
            (y * up).sum().backward()
            grads.append((y.detach().clone(), {k: v.grad.clone() for k, v in trainable(m).items() if v.grad is not None}))
        (y0, g0), (y1, g1) = grads
        assert torch.equal(y0, y1) and g0 and set(g0) == set(g1), name
        assert all(torch.equal(g0[k], g1[k]) for k in g0), name
    # the table handed to the call instead of the resident one (a CPU index is moved like the other index arguments)
    del m.embedding_table
    m.eval()
    with torch.no_grad():
        y = m(task=CIR, target_item_index=tix.cpu(), embedding_table=cu(table), **sets["indexed"])
        assert torch.equal(y, m(task=CIR, target_item_text_embedding=txt, embedding_table=cu(table), **sets["indexed"]))


@pytest.mark.parametrize("hip_optimizer", [False, True], ids=["torch_adamw", "hip_adamw"])
def test_cir_trainer_on_index_batches_equals_the_dense_batches_bit_for_bit(hip_optimizer):
    """B = 8, K = 5, accumulation 2, four micro-batches -> two optimizer steps, one-layer model: losses and parameters of the run on index
    batches == the run on the dense batches gathered from the same rows; then valid_epoch on both forms: the same loss and Recall@K."""
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    B, K = 8, 5
    table = synth.item_embeddings(31, "table", 200) * 3.0
    g = np.random.default_rng(31)
    forms = [index_batch(g, table, B, K, CIR) for _ in range(4)]
    off = [0, 64, 128, 200]                                        # validation: the table is the three category pools, concatenated
    for ib, db in forms:
        grp = g.integers(0, 3, B)
        for b in (ib, db):
            b["pos_item_group"] = torch.from_numpy(grp)
            b["pos_item_row"] = torch.tensor([int(g.integers(0, off[c + 1] - off[c])) for c in grp]) if b is ib else ib["pos_item_row"]
    m = make_model()
    start = {k: v.detach().clone() for k, v in trainable(m).items()}
    runs = {}
    for name in ("indexed", "dense"):
        with torch.no_grad():
            for k, v in trainable(m).items():
                v.copy_(start[k])
        m.mark_weights_changed()
        if name == "indexed":
            m.set_embedding_table(torch.from_numpy(table))
        elif hasattr(m, "embedding_table"):
            del m.embedding_table                                  # the dense run has no table to fall back on
        batches = [f[0 if name == "indexed" else 1] for f in forms]
        on_path = [p for p in CIRTrainer._default_params(m) if any(p is q for q in trainable(m).values())]
        tr = CIRTrainer(m, steps_per_epoch=4, cfg=CIRTrainConfig(learning_rate=2e-5, accumulation_steps=2, n_epochs=1, hip_optimizer=hip_optimizer),
                        params=on_path)
        m.train()
        tr.grads.zero_()
        losses = torch.stack([tr.micro_step(b, i)[0] for i, b in enumerate(batches)])
        params = {k: v.detach().clone() for k, v in trainable(m).items()}
        valid = tr.valid_epoch(batches, (cu(table), off), top_k_list=(1, 5, 10))
        assert m.training
        runs[name] = (losses, params, valid)
    (li, pi, vi), (ld, pd, vd) = runs["indexed"], runs["dense"]
    print("losses", li.tolist(), "valid", vi)
    assert torch.isfinite(li).all() and torch.equal(li, ld), (li, ld)
    moved = [k for k in pi if not torch.equal(pi[k], start[k])]
    assert len(moved) >= len(pi) - 3, moved                        # everything on the CIR path was stepped
    assert all(torch.equal(pi[k], pd[k]) for k in pi), [k for k in pi if not torch.equal(pi[k], pd[k])]
    assert list(vi) == ["loss", "Recall@1", "Recall@5", "Recall@10"] and vi == vd, (vi, vd)
