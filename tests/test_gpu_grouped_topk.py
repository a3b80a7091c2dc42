"""Category-pool CIR retrieval on a real MI355X: ofx_l2_topk_grouped / Engine.l2_topk_grouped (outfitx_amd/csrc/scoring.hip) and
CIRTrainer.valid_epoch on the real model.

Method as in tests/test_gpu_scoring.py: finite inputs are integer lattices (oracle.np_oracle.lattice), on which the kernels' fp32 d2 is
exact, so indices and ground-truth positions are compared with array_equal on every position against tests/grouped_topk_ref.py (pinned
to the reference's formulation by tests/test_cpu_grouped_topk.py) and distances bit for bit with float32(sqrt(float64 d2)).  On
real-valued embeddings the grouped call is held to Engine.l2_topk on each group's own pool, bit for bit.  Outputs of raw calls are
poisoned first and the workspace is followed by guard bytes."""
import numpy as np
import pytest
import torch

from grouped_topk_ref import f32_sqrt, grouped_topk_ref, recall_ref
from oracle import np_oracle as O
from outfitx_amd import synth

pytestmark = pytest.mark.gpu

L = None
ENG = None
OFX_EINVAL, OFX_ESHAPE, OFX_EWORKSPACE = -1, -2, -4
GUARD = 4096
TOP_K = (1, 5, 10, 15, 30, 50)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global L, ENG
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from outfitx_amd import _lib as lib
    from outfitx_amd.engine import Engine
    lib.load()
    L = lib
    ENG = Engine(torch.device("cuda", 0))
    yield
    ENG = None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def guard_pattern():
    return torch.arange(GUARD, dtype=torch.int32, device="cuda").mul_(37).add_(11).to(torch.uint8)


class CountingLib:
    """The loaded library with the grouped call counted (Engine.lib stand-in: how many C calls did a Python call make?)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ofx_l2_topk_grouped(self, *a):
        self.calls += 1
        return self._lib.ofx_l2_topk_grouped(*a)


def grouped(Q, grp, P, off, k, gt=None, **kw):
    """Engine.l2_topk_grouped on host arrays -> numpy (idx, dist, gt_pos | None, number of C calls)."""
    lib = CountingLib(ENG.lib)
    ENG.lib = lib
    try:
        idx, dist, pos = ENG.l2_topk_grouped(dev(Q), grp, dev(P), off, k, gt=gt, **kw)
    finally:
        ENG.lib = lib._lib
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy(), None if pos is None else pos.cpu().numpy(), lib.calls


def assert_ref(idx, dist, pos, Q, grp, P, off, k, gt=None):
    ei, ed2, ep = grouped_topk_ref(Q, grp, P, off, k, gt)
    assert np.array_equal(idx, ei)
    assert same_bits(dist, f32_sqrt(ed2))
    if gt is not None:
        assert np.array_equal(pos, ep)
    return ei, ed2, ep


# pool sizes: one row, one below / exactly / one above the 128-row tile, several tiles, and one smaller than k = 50;
# queries per group: a handful against the 1-row pool, none, an exactly full panel, a group that needs two panels, one, a last partial panel
POOL_ROWS = [1, 127, 128, 129, 300, 40]
QUERIES = [5, 0, 128, 129, 1, 5]


def layout(seed, D, lo=-8, hi=8):
    off = np.concatenate([[0], np.cumsum(POOL_ROWS)])
    grp = np.concatenate([np.full(n, g) for g, n in enumerate(QUERIES)])
    P, Q = O.lattice(seed, off[-1], D, lo, hi), O.lattice(seed + 1, len(grp), D, lo, hi)
    g = np.random.default_rng(seed + 2)
    gt = off[grp] + g.integers(0, np.asarray(POOL_ROWS)[grp])
    gt[::17] = -1                                                 # some queries without ground truth
    # by construction: the 300-row pool's query looks for its FARTHEST row (never among k <= 128), the 129-row pool's first for its nearest
    far, near = int(np.flatnonzero(grp == 4)[0]), int(np.flatnonzero(grp == 3)[0])
    gt[far] = off[4] + O.d2_exact(Q[far:far + 1], P[off[4]:off[5]])[0].argmax()
    gt[near] = off[3] + O.d2_exact(Q[near:near + 1], P[off[3]:off[4]])[0].argmin()
    return Q, grp, P, off, gt


@pytest.mark.parametrize("D", [32, 96, 128])                      # 1 k-step; 3: the first odd count that reaches the two-stage steady state; 4: even
@pytest.mark.parametrize("k", [1, 50, 128])
def test_grouped_exact_on_the_lattice(D, k):
    Q, grp, P, off, gt = layout(100 + D + k, D)
    idx, dist, pos, calls = grouped(Q, grp, P, off, k, gt)
    assert calls == 1
    ei, _, ep = assert_ref(idx, dist, pos, Q, grp, P, off, k, gt)
    # what the layout is there for: the -1 / +inf tail behind a pool smaller than k, a ground truth beyond the list, one inside it, none
    small = np.asarray(POOL_ROWS)[grp] < k
    assert small.any() == (k > 1) and all((idx[q, POOL_ROWS[grp[q]]:] == -1).all() and np.isinf(dist[q, POOL_ROWS[grp[q]]:]).all()
                                          for q in np.flatnonzero(small))
    assert (ep == -1).any() and (ep == k).any() and (ep == 0).any()
    if k == 50:
        last = grp == 5                                           # the 40-row pool: every row listed, so a ground truth is always found
        assert (idx[last, 39] >= 0).all() and (idx[last, 40:] == -1).all() and ((pos[last] < 40) | (gt[last] < 0)).all()


def test_ground_truth_beyond_k_and_absent_through_the_c_abi():
    """The C call itself: gt_pos = k for a row that is in the pool but not among the k nearest, and k as well for gt < 0 (the Python layer
    turns the latter into -1); idx / dist do not depend on gt being asked for."""
    Q, grp, P, off, _ = layout(7, 64)
    k = 10
    ei, ed2, _ = grouped_topk_ref(Q, grp, P, off, k)
    gt = np.where(np.arange(len(Q)) % 3 == 0, -1, ei[:, 0])
    far = np.flatnonzero(grp == 4)[0]                             # 300-row pool: some row outside the 10 nearest
    gt[far] = int(np.setdiff1d(np.arange(off[4], off[5]), ei[far])[0])
    gt[np.flatnonzero(grp == 3)[5]] = ei[np.flatnonzero(grp == 3)[5], 7]
    panels = panel_table(grp, off)
    rc, idx, dist, pos = raw_grouped(dev(Q), dev(P), len(Q), len(P), 64, k, panels, max(POOL_ROWS), gt=gt)
    assert rc == 0
    assert np.array_equal(idx.cpu().numpy(), ei) and same_bits(dist.cpu().numpy(), f32_sqrt(ed2))
    want = np.where(gt < 0, k, np.where((ei == gt[:, None]).any(1), (ei == gt[:, None]).argmax(1), k))
    assert np.array_equal(pos.cpu().numpy(), want) and want[far] == k and (want == 7).any() and (want == 0).any()
    rc, idx2, dist2, _ = raw_grouped(dev(Q), dev(P), len(Q), len(P), 64, k, panels, max(POOL_ROWS))
    assert rc == 0 and torch.equal(idx, idx2) and torch.equal(dist.view(torch.int32), dist2.view(torch.int32))


def panel_table(grp, off):
    """The panel table Engine.l2_topk_grouped builds, for queries already sorted by group: runs of one group cut at 128 queries."""
    out, s, n = [], 0, len(grp)
    while s < n:
        e = s + 1
        while e < n and e - s < 128 and grp[e] == grp[s]:
            e += 1
        out.append((s, e, int(off[grp[s]]), int(off[grp[s] + 1])))
        s = e
    return torch.tensor(out, dtype=torch.int32).cuda()


def raw_grouped(Qd, Pd, nq, npool, D, k, panels, max_rows, gt=None, ws_short=0, n_panels=None, null=(), q_ptr=None, pos_without_gt=False):
    """One ofx_l2_topk_grouped call -> (rc, idx, dist, gt_pos): outputs poisoned (-7 / NaN / -7), workspace of exactly the _ws figure
    (minus ws_short) followed by guard bytes that must survive."""
    lib = L.load()
    idx = torch.full((nq, max(k, 1)), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((nq, max(k, 1)), float("nan"), dtype=torch.float32, device="cuda")
    pos = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    gtd = None if gt is None else torch.from_numpy(np.asarray(gt, np.int64)).cuda()
    need = int(lib.ofx_l2_topk_grouped_ws(nq, npool, max(max_rows, 1)))
    assert need > 0
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device="cuda")
    ws[need:] = guard_pattern()
    arg = {"Q": Qd.data_ptr() if q_ptr is None else q_ptr, "P": Pd.data_ptr(), "panels": panels.data_ptr(), "idx": idx.data_ptr(),
           "dist": dist.data_ptr(), "ws": ws.data_ptr()}
    arg.update({n: None for n in null})
    rc = lib.ofx_l2_topk_grouped(ENG.h, arg["Q"], arg["P"], nq, npool, D, k, arg["panels"], len(panels) if n_panels is None else n_panels, max_rows,
                                 None if gtd is None else gtd.data_ptr(), arg["idx"], arg["dist"],
                                 pos.data_ptr() if (gtd is not None or pos_without_gt) else None, arg["ws"], need - ws_short, stream())
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], guard_pattern()), "ofx_l2_topk_grouped wrote behind its workspace"
    return rc, idx, dist, pos


def test_rows_next_to_a_pool_do_not_leak_into_it():
    """Rows p_lo - 1 and p_hi (the neighbouring pools' last / first rows) are exact copies of one query of the middle group: a leak would
    put them first at distance 0.  The query's result must not hold them, and its distances are those of the call without the copies."""
    off = np.array([0, 100, 230, 330])
    grp = np.repeat([0, 1, 2], [3, 4, 3])
    P, Q = O.lattice(31, 330, 64, -8, 8), O.lattice(32, 10, 64, -8, 8)
    k = 50
    clean = grouped(Q, grp, P, off, k)
    planted = P.copy()
    planted[99] = Q[4]; planted[230] = Q[4]
    got = grouped(Q, grp, planted, off, k)
    mid = grp == 1
    assert not np.isin(got[0][mid], [99, 230]).any() and got[1][4, 0] > 0
    assert np.array_equal(got[0][mid], clean[0][mid]) and same_bits(got[1][mid], clean[1][mid])
    assert_ref(got[0], got[1], None, Q, grp, planted, off, k)
    # the neighbours do see their own planted row, at distance 0 only for a query that equals it
    Q2 = Q.copy(); Q2[0] = Q[4]; Q2[9] = Q[4]
    i2, d2, _, _ = grouped(Q2, grp, planted, off, k)
    assert i2[0, 0] == 99 and d2[0, 0] == 0 and i2[9, 0] == 230 and d2[9, 0] == 0 and i2[4, 0] != 99


def test_grouped_equals_the_flat_call_bit_for_bit_on_real_embeddings():
    """Random normalised item embeddings (not a lattice), D = 1024, groups of 200 / 3000 / 65 rows: idx and dist bits equal, group by
    group, Engine.l2_topk(Q_g, P_g, k) plus the group's base - the tile arithmetic of a (q, p) pair does not depend on the launch."""
    rows, nq_of, k = [200, 3000, 65], [10, 140, 7], 50
    off = np.concatenate([[0], np.cumsum(rows)])
    P = synth.item_embeddings(51, "pool", int(off[-1]))
    Q = (synth.item_embeddings(51, "queries", sum(nq_of)) * 3.0).astype(np.float32)
    grp = np.repeat(np.arange(3), nq_of)
    idx, dist, _, calls = grouped(Q, grp, P, off, k)
    assert calls == 1
    Pd, Qd = dev(P), dev(Q)
    for g in range(3):
        sel = np.flatnonzero(grp == g)
        fi, fd = ENG.l2_topk(Qd[sel[0]:sel[-1] + 1], Pd[off[g]:off[g + 1]], k, index_base=int(off[g]))
        assert np.array_equal(idx[sel], fi.cpu().numpy()), g
        assert same_bits(dist[sel], fd.cpu().numpy()), g
    assert (np.diff(dist, axis=1) >= 0).all()


def test_callers_order_and_chunking_give_the_same_rows():
    """A shuffled group_of_query gives the sorted call's rows, un-permuted; max_ws_bytes that forces three C calls gives the same again."""
    Q, grp, P, off, gt = layout(77, 96)
    k = 50
    want = grouped(Q, grp, P, off, k, gt)
    assert want[3] == 1
    perm = np.random.default_rng(3).permutation(len(Q))
    got = grouped(Q[perm], grp[perm], P, off, k, gt[perm])
    assert got[3] == 1
    assert np.array_equal(got[0], want[0][perm]) and same_bits(got[1], want[1][perm]) and np.array_equal(got[2], want[2][perm])
    assert_ref(*got[:3], Q[perm], grp[perm], P, off, k, gt[perm])
    # three chunks: the workspace of a third of the queries fits, that of half of them does not
    lib = L.load()
    n3 = -(-len(Q) // 3)
    budget = int(lib.ofx_l2_topk_grouped_ws(n3, len(P), max(POOL_ROWS)))
    assert budget < int(lib.ofx_l2_topk_grouped_ws(len(Q) // 2, len(P), max(POOL_ROWS)))
    for q, g_, t in ((Q, grp, gt), (Q[perm], grp[perm], gt[perm])):
        ch = grouped(q, g_, P, off, k, t, max_ws_bytes=budget)
        assert ch[3] == 3
        assert_ref(*ch[:3], q, g_, P, off, k, t)
    with pytest.raises(ValueError):
        grouped(Q, grp, P, off, k, gt, max_ws_bytes=1024)         # not even one query fits


def test_non_finite_rows_sort_last_within_their_pool_and_stay_out_of_the_others():
    """A NaN row and a +inf row inside pool 0 - the +inf one its LAST row, next to pool 1: with k = the pool's size they take the last
    two places of every pool-0 query behind the finite rows in exact order; pool 1's queries are those of the clean call."""
    off = np.array([0, 60, 120])
    grp = np.repeat([0, 1], [6, 5])
    P, Q = O.lattice(41, 120, 64, -8, 8), O.lattice(42, 11, 64, -8, 8)
    bad = P.copy()
    bad[17, 5] = np.nan
    bad[59, 0] = np.inf
    k = 60
    idx, dist, _, _ = grouped(Q, grp, bad, off, k)
    finite = np.setdiff1d(np.arange(60), [17, 59])
    ei, ed2 = O.l2_topk_exact(Q[:6], P[finite], 58)
    assert np.array_equal(idx[:6, :58], finite[ei]) and same_bits(dist[:6, :58], f32_sqrt(ed2))
    assert all(set(r) == {17, 59} for r in idx[:6, 58:]) and not np.isfinite(dist[:6, 58:]).any()
    ci, cd, _, _ = grouped(Q, grp, P, off, k)
    assert np.array_equal(idx[6:], ci[6:]) and same_bits(dist[6:], cd[6:]) and np.isfinite(dist[6:]).all()
    assert_ref(ci, cd, None, Q, grp, P, off, k)


def last_error():
    return L.load().ofx_last_error().decode()


def test_python_layer_rejects_bad_metadata_before_any_launch():
    Q, grp, P, off, gt = layout(5, 32)
    lib = CountingLib(ENG.lib)
    ENG.lib = lib
    try:
        Qd, Pd = dev(Q), dev(P)
        bad_grp = grp.copy(); bad_grp[3] = 6
        neg_grp = grp.copy(); neg_grp[3] = -1
        empty_q = np.array([0, 1, 128, 128, 385, 685, 725])                  # group 2, which has queries, without rows (group 1, empty of queries, may be)
        back = off.copy(); back[3] = back[2] - 1
        short = off.copy(); short[-1] -= 1
        gt_out = gt.copy(); gt_out[1] = off[grp[1] + 1]                      # first row of the NEXT pool
        for args in ((bad_grp, off, None), (neg_grp, off, None), (grp, empty_q, None), (grp, back, None), (grp, short, None), (grp, off[1:], None),
                     (grp, off, gt_out), (grp[:-1], off, None), (grp, off, gt[:-1])):
            with pytest.raises(ValueError):
                ENG.l2_topk_grouped(Qd, args[0], Pd, args[1], 10, gt=args[2])
        assert lib.calls == 0
        # what the C call refuses surfaces as OfxError, nothing quiet
        with pytest.raises(L.OfxError, match="k=129"):
            ENG.l2_topk_grouped(Qd, grp, Pd, off, 129)
    finally:
        ENG.lib = lib._lib


def test_c_call_rejects_what_it_cannot_run_and_launches_nothing():
    """Return code and a fragment of ofx_last_error(); the poisoned outputs of a rejected call are untouched."""
    Q, grp, P, off, gt = layout(6, 64)
    Qd, Pd, nq, npool, mr = dev(Q), dev(P), len(Q), len(P), max(POOL_ROWS)
    panels = panel_table(grp, off)
    cases = [
        (dict(null=("Q",)), OFX_EINVAL), (dict(null=("P",)), OFX_EINVAL), (dict(null=("panels",)), OFX_EINVAL), (dict(null=("idx",)), OFX_EINVAL),
        (dict(null=("dist",)), OFX_EINVAL), (dict(null=("ws",)), OFX_EINVAL), (dict(q_ptr=Qd.data_ptr() + 4), OFX_EINVAL),
        (dict(gt=None, pos_without_gt=True), OFX_EINVAL), (dict(D=48), OFX_ESHAPE), (dict(D=0), OFX_ESHAPE), (dict(k=0), OFX_ESHAPE), (dict(k=129), OFX_ESHAPE),
        (dict(n_panels=0), OFX_ESHAPE), (dict(max_rows=0), OFX_ESHAPE), (dict(ws_short=1), OFX_EWORKSPACE),
    ]
    for kw, code in cases:
        a = dict(D=64, k=10, max_rows=mr, gt=gt)
        a.update(kw)
        rc, idx, dist, pos = raw_grouped(Qd, Pd, nq, npool, a.pop("D"), a.pop("k"), panels, a.pop("max_rows"), **a)
        assert rc == code and "l2_topk_grouped" in last_error(), (kw, rc, last_error())
        assert (idx == -7).all() and torch.isnan(dist).all() and (pos == -7).all(), kw
    assert int(L.load().ofx_l2_topk_grouped_ws(-1, 10, 10)) == 0
    # and the accepted call on the same buffers
    rc, idx, dist, pos = raw_grouped(Qd, Pd, nq, npool, 64, 10, panels, mr, gt=gt)
    assert rc == 0
    assert_ref(idx.cpu().numpy(), dist.cpu().numpy(), np.where(gt < 0, -1, pos.cpu().numpy()), Q, grp, P, off, 10, gt)


def test_valid_epoch_on_the_real_model():
    """CIRTrainer.valid_epoch, synth weights, two batches of 16, 3 pools of 64 rows, D = 1024: recall equals the host reference applied to the
    y_hat the model returned, loss equals SetWiseRankingLoss evaluated without gradients on the same tensors; one retrieval call.
    The y_hat of synthetic weights lie far from the pools (|y_hat| ~ 44, |row| ~ 4): a pool's 64 distances crowd into 0.3, closer together
    in places than fp32 can tell apart.  The position of a ground truth is defined for the kernel and the float64 reference alike only
    where its d2 is further from every other row's than both sides' rounding can move it, so each query's positive is drawn among the
    rows that are: a gap above twice the worst-case fp32 bound (D + 3) 2^-24 (|q| + |p|)^2 of |q|^2 + |p|^2 - 2 q.p."""
    from conftest import W_SEED
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    cfg.transformer.dropout = 0.0
    m = OutfitX(cfg, train_precision="f16")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.full_state_dict(W_SEED).items()}, strict=True)
    m = m.cuda().train()
    B, K, seed = 16, 4, 900
    off = [0, 64, 128, 192]
    P = torch.from_numpy(synth.item_embeddings(seed, "pool", 192) * 3.0).cuda()
    g = np.random.default_rng(seed)
    batches = []
    for i in range(2):
        emb, mask = synth.outfit_batch(seed + i, B, 16, synth.ragged_lengths(seed + i, B, 1, 12))
        batches.append({"input_dict": {"task": CIR, "outfit_embedding": torch.from_numpy(emb), "outfit_mask": torch.from_numpy(mask),
                                       "target_item_text_embedding": torch.from_numpy(synth.unit_rows(seed + i, "target_text", B, 512))},
                        "pos_item_embedding": torch.from_numpy(synth.item_embeddings(seed + i, "pos", B) * 3.0),
                        "neg_items_embedding": torch.from_numpy(synth.item_embeddings(seed + i, "neg", B * K).reshape(B, K, 1024) * 3.0),
                        "neg_items_mask": torch.from_numpy(g.random((B, K)) < 0.3), "pos_item_group": torch.from_numpy(g.integers(0, 3, B))})
    # the model's y_hat (eval mode, as valid_epoch runs it) -> positives whose position is well defined
    m.eval()
    with torch.no_grad():
        y0 = torch.cat([m(**{n: (v if n == "task" else v.cuda()) for n, v in b["input_dict"].items()}) for b in batches])
    m.train()
    Ph, y0h = P.cpu().numpy().astype(np.float64), y0.cpu().numpy().astype(np.float64)
    for i, b in enumerate(batches):
        rows = []
        for j, c in enumerate(b["pos_item_group"].tolist()):
            q, pool = y0h[i * B + j], Ph[off[c]:off[c + 1]]
            d2 = ((q - pool) ** 2).sum(-1)
            bound = (1024 + 3) * 2.0 ** -24 * (np.linalg.norm(q) + np.linalg.norm(pool, axis=1).max()) ** 2
            gap = np.abs(d2[:, None] - d2[None, :]) + np.where(np.eye(64, dtype=bool), np.inf, 0.0)
            ok = np.flatnonzero(gap.min(1) > 2 * bound)
            assert len(ok) >= 4, (len(ok), bound)
            rows.append(int(g.choice(ok)))
        b["pos_item_row"] = torch.tensor(rows)
    on_path = [p for p in CIRTrainer._default_params(m) if not any(p is q for q in m.item_encoder.parameters())]
    tr = CIRTrainer(m, steps_per_epoch=2, cfg=CIRTrainConfig(n_epochs=1), params=on_path)
    seen = []
    eng_fn = m._engine().l2_topk_grouped

    def spy(Q, *a, **kw):
        seen.append(Q.detach().clone())
        return eng_fn(Q, *a, **kw)
    out = tr.valid_epoch(batches, (P, off), topk_fn=spy)
    default = tr.valid_epoch(batches, (P, off))                   # the default topk_fn is that engine call
    assert out == default and m.training and len(seen) == 1 and seen[0].shape == (2 * B, 1024)
    y_hat = seen[0]
    grp = np.concatenate([b["pos_item_group"].numpy() for b in batches])
    gt = np.asarray(off)[grp] + np.concatenate([b["pos_item_row"].numpy() for b in batches])
    assert torch.equal(y_hat, y0)
    yh = y_hat.cpu().numpy()
    want = recall_ref(grouped_topk_ref(yh, grp, Ph, off, 50, gt)[2], TOP_K)
    assert {n: out[n] for n in want} == want and 0 < want["Recall@50"]
    with torch.no_grad():
        tot = torch.zeros((), device="cuda")
        for i, b in enumerate(batches):
            tot += tr.loss_fn(batch_y=b["pos_item_embedding"].cuda(), batch_y_hat=y_hat[i * B:(i + 1) * B], batch_negative_samples=b["neg_items_embedding"].cuda(),
                              batch_negative_mask=b["neg_items_mask"].cuda())
    assert out["loss"] == float(tot / 2) and np.isfinite(out["loss"])
    assert list(tr.valid_epoch(batches, None, with_recall=False)) == ["loss"]
