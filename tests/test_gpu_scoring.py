"""Index-exact edge tests of the scoring kernels (outfitx_amd/csrc/scoring.hip: ofx_fitb_argmin, both paths of ofx_l2_topk,
ofx_topk_merge) on a real MI355X, through the C ABI.

Method: every finite input is an integer lattice (oracle.np_oracle.lattice), on which each fp32 product, norm and partial sum of
|q|^2 + |p|^2 - 2 q.p is exact in any summation order.  The kernels' d2 then equals the float64 d2 of l2_topk_exact / fitb_argmin_exact,
so indices are compared with np.array_equal on EVERY position of every query (ties -> smaller pool index; no near-tie clause, no
tolerance) and distances bit for bit with float32(sqrt(float64 d2)).  tests/test_cpu_scoring_ref.py pins those host functions against
torch.cdist + topk / argmin, and pins where the reference puts non-finite rows (last in smallest-k; argmin returns the first NaN).
Outputs are poisoned (-1 / NaN) before each call, and ofx_l2_topk's workspace is followed by 4 KiB of guard bytes.

HIP's sqrtf under the library's flags (-O3, no fast-math) gave the correctly rounded root on every distance of every case here: the
distance comparison is exact equality, no ulp allowance was needed.

Wall time of this file on the MI355X box: 81 tests in 11.5 s of pytest time run alone (14 s with interpreter and torch start-up), 7.6 s
inside the whole GPU suite, where tests/test_gpu_ops.py takes 22.5 s; the host references are most of it.
"""
import numpy as np
import pytest
import torch

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

L = None
ENG = None
OFX_EINVAL, OFX_ESHAPE, OFX_EWORKSPACE = -1, -2, -4
GUARD = 4096


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


def f32_sqrt(d2):
    return np.sqrt(np.asarray(d2, np.float64)).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def guard_pattern():
    return torch.arange(GUARD, dtype=torch.int32, device="cuda").mul_(37).add_(11).to(torch.uint8)


def raw_topk(Qd, Pd, nq, npool, D, k, index_base=0, ws_short=0, idx_null=False):
    """One ofx_l2_topk call on device tensors -> (rc, idx, dist): outputs poisoned, workspace of exactly ofx_workspace_bytes
    (minus ws_short) followed by guard bytes that must survive."""
    lib = L.load()
    idx = torch.full((nq, max(k, 1)), -1, dtype=torch.int64, device="cuda")
    dist = torch.full((nq, max(k, 1)), float("nan"), dtype=torch.float32, device="cuda")
    need = int(lib.ofx_workspace_bytes(ENG.h, L.OP_TOPK, nq, npool))
    assert need > 0
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device="cuda")
    ws[need:] = guard_pattern()
    qp = Qd if isinstance(Qd, int) else Qd.data_ptr()
    rc = lib.ofx_l2_topk(ENG.h, qp, Pd.data_ptr(), nq, npool, D, k, index_base, None if idx_null else idx.data_ptr(), dist.data_ptr(),
                         ws.data_ptr(), need - ws_short, stream())
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], guard_pattern()), "ofx_l2_topk wrote behind its workspace"
    return rc, idx, dist


def topk(Q, P, k, index_base=0, filtered=None):
    """ofx_l2_topk on host arrays -> numpy (idx, dist); filtered: None = the library's default path choice, 1 / 0 = ofx_tune(17, .)."""
    lib = L.load()
    nq, D = Q.shape
    if filtered is not None:
        lib.ofx_tune(17, filtered)
    try:
        rc, idx, dist = raw_topk(dev(Q), dev(P), nq, P.shape[0], D, k, index_base)
    finally:
        if filtered is not None:
            lib.ofx_tune(17, 1)
    L.check(rc, "ofx_l2_topk")
    return idx.cpu().numpy(), dist.cpu().numpy()


def assert_exact(idx, dist, Q, P, k, index_base=0):
    ei, ed2 = O.l2_topk_exact(Q, P, k, index_base)
    assert np.array_equal(idx, ei)
    assert same_bits(dist, f32_sqrt(ed2))
    return ei, ed2


BIG = 2 ** 33
MATRIX_CASES = [
    # D, nq, np, k, index_base, lo, hi
    (32, 1, 1, 1, 0, -8, 8), (32, 5, 50, 50, 7, -1, 1), (32, 129, 4099, 128, 0, -1, 1), (32, 300, 1001, 127, BIG, -1, 1),
    (32, 127, 128, 1, 0, -8, 8), (64, 1, 127, 127, 0, -8, 8), (64, 127, 128, 128, 7, -8, 8), (64, 128, 129, 2, 0, -8, 8),
    (64, 129, 4099, 50, BIG, -8, 8), (64, 300, 32767, 128, 0, -8, 8), (64, 5, 32767, 1, 7, -8, 8), (64, 300, 50, 50, 0, -8, 8),
    (96, 129, 1001, 50, 0, -8, 8), (96, 1, 4099, 127, 0, -8, 8), (96, 128, 127, 1, 7, -8, 8), (96, 5, 129, 128, 0, -8, 8),
    (1024, 127, 4099, 50, 0, -8, 8), (1024, 300, 1001, 128, 7, -8, 8), (1024, 1, 50, 2, 0, -8, 8), (1024, 129, 32767, 50, BIG, -8, 8),
    (1024, 5, 1, 1, 0, -8, 8), (1024, 128, 129, 127, 0, -8, 8), (2048, 129, 1001, 127, 0, -4, 4), (2048, 5, 128, 128, 7, -4, 4),
    (2048, 128, 4099, 2, 0, -4, 4),
]


@pytest.mark.parametrize("D,nq,npool,k,base,lo,hi", MATRIX_CASES)
def test_topk_matrix_path_exact_on_the_lattice(D, nq, npool, k, base, lo, hi):
    """Distance matrix + radix select (np < 32768): 1, 2, 3, 32 and 64 k-steps; one query, ragged and full query panels side by side;
    pools below one tile, np % 4 != 0, k = 1 ... 128 and k = np; index_base up to 2^33.  [-8, 8] has few ties, {-1, 0, 1} at D = 32 ties
    every distance hundreds of times."""
    Q, P = O.lattice(1000 + D + nq, nq, D, lo, hi), O.lattice(2000 + D + npool, npool, D, lo, hi)
    idx, dist = topk(Q, P, k, base)
    assert_exact(idx, dist, Q, P, k, base)


def test_topk_identical_rows_and_queries_that_are_pool_rows():
    """A pool of 5,000 identical rows (and one of 33,000, on both paths of the large pools): the answer is rows 0 .. k-1, whatever the
    distance.  Queries that ARE pool rows: their first distance has the bits of +0.0 - never -0.0 (which would sort last as a bit
    pattern) or NaN."""
    row = O.lattice(1, 1, 64, -8, 8)
    Q = np.concatenate([row, O.lattice(2, 130, 64, -8, 8)])
    for n, filtered in ((5000, None), (33000, 1), (33000, 0)):
        P = np.repeat(row, n, 0)
        for k in (1, 50, 128):
            idx, dist = topk(Q, P, k, 7, filtered)
            assert np.array_equal(idx, np.broadcast_to(np.arange(k) + 7, (131, k)))
            assert_exact(idx, dist, Q, P, k, 7)
            assert (dist[0].view(np.uint32) == 0).all()
    P = O.lattice(3, 4099, 96, -8, 8)
    P[4000] = P[17]
    sel = np.array([0, 17, 127, 128, 4000, 4098])
    Q = np.concatenate([P[sel], O.lattice(4, 125, 96, -8, 8)])
    idx, dist = topk(Q, P, 50)
    assert_exact(idx, dist, Q, P, 50)
    assert (dist[:6, 0].view(np.uint32) == 0).all() and (dist[:6, 2] > 0).all()
    assert idx[:6, 0].tolist() == [0, 17, 127, 128, 17, 4098] and idx[1, 1] == 4000 and idx[4, 1] == 4000


# ------------------------------------------------------------------------------------------------ sample + filter path
FCAP = 2048          # candidate list per query (scoring.hip): a longer list sends the query to the exact fallback


def sample_rows(npool):
    return (max(4096, npool // 16) + 127) // 128 * 128


def filter_counts(Q, P, k):
    """Per query: how many rows behind the sample are no farther than the sample's k-th nearest - the length its candidate list needs.
    Computed from the exact d2: a condition on the INPUTS (which path a query takes), not a measurement of the kernel."""
    S = sample_rows(len(P))
    out = np.empty(len(Q), np.int64)
    for s in range(0, len(Q), 32):
        d2 = O.d2_exact(Q[s:s + 32], P)
        tau = np.partition(d2[:, :S], k - 1, axis=1)[:, k - 1]
        out[s:s + 32] = (d2[:, S:] <= tau[:, None]).sum(1)
    return out


def both_paths_exact(Q, P, k, base=0):
    fi, fd = topk(Q, P, k, base, filtered=1)
    mi, md = topk(Q, P, k, base, filtered=0)
    ei, ed2 = assert_exact(fi, fd, Q, P, k, base)
    assert np.array_equal(mi, ei) and same_bits(md, f32_sqrt(ed2))
    return ei, ed2


@pytest.mark.parametrize("npool,k,nq,D", [(32768, 128, 129, 64), (40000, 128, 200, 64), (40000, 50, 200, 1024), (70001, 50, 129, 64),
                                          (70001, 1, 1, 1024), (32768, 1, 200, 1024)])
def test_topk_filtered_path_no_query_overflows(npool, k, nq, D):
    Q, P = O.lattice(3000 + nq + D, nq, D, -8, 8), O.lattice(4000 + npool + D, npool, D, -8, 8)
    cnt = filter_counts(Q, P, k)
    print(f"candidate-list lengths np={npool} k={k} D={D}: max {cnt.max()} of {FCAP}")
    assert cnt.max() <= FCAP, "test construction: a query would overflow its candidate list"
    both_paths_exact(Q, P, k, 7)


@pytest.mark.parametrize("npool,k,nq,D", [(40000, 50, 129, 64), (32768, 128, 200, 64), (70001, 1, 5, 1024)])
def test_topk_filtered_path_every_query_overflows(npool, k, nq, D):
    """A pool of 8 distinct rows repeated in random order: the nearest row has thousands of copies behind the sample, every query's list
    overflows and the fallback recomputes it; the answer is the k lowest-index copies (all inside the sample)."""
    g = np.random.default_rng(npool + k)
    rows = O.lattice(5000 + D, 8, D, -8, 8)
    which = g.integers(0, 8, npool)
    P = rows[which]
    Q = O.lattice(6000 + D, nq, D, -8, 8)
    cnt = filter_counts(Q, P, k)
    print(f"candidate-list lengths, 8-row pool np={npool} k={k}: min {cnt.min()} max {cnt.max()}")
    assert cnt.min() > FCAP, "test construction: a query would NOT overflow its candidate list"
    ei, ed2 = both_paths_exact(Q, P, k, BIG)
    near = O.d2_exact(Q, rows).argmin(1)
    for q in range(nq):
        assert np.array_equal(ei[q] - BIG, np.flatnonzero(which == near[q])[:k])


def test_topk_filtered_path_overflowing_and_fitting_queries_in_one_launch():
    """Lattice pool with two planted clusters behind the sample (copies of query 3 / query 77 moved by one unit step): exactly those two
    queries overflow, the other 198 stay on the filtered path, in the same launch."""
    nq, npool, k, D = 200, 40000, 50, 64
    g = np.random.default_rng(45)
    Q, P = O.lattice(43, nq, D, -8, 8), O.lattice(44, npool, D, -8, 8)
    Q[[3, 77]] = 8 * g.choice(np.array([-1, 1], np.float32), (2, D))        # two corners of the lattice: far from every other query, so that a cluster is near ITS query only
    for q, lo_, n in ((3, 20000, 3000), (77, 30000, 2500)):
        P[lo_:lo_ + n] = Q[q]
        P[np.arange(lo_, lo_ + n), g.integers(0, D, n)] += g.choice(np.array([-1, 1], np.float32), n)      # d2 = 1, 128 variants: ties
    cnt = filter_counts(Q, P, k)
    print(f"candidate-list lengths: queries 3 / 77 {cnt[3]} / {cnt[77]}, largest other {np.delete(cnt, [3, 77]).max()}")
    assert np.flatnonzero(cnt > FCAP).tolist() == [3, 77], "test construction"
    ei, _ = both_paths_exact(Q, P, k, 7)
    assert np.array_equal(ei[3] - 7, np.arange(20000, 20000 + k)) and np.array_equal(ei[77] - 7, np.arange(30000, 30000 + k))


def test_topk_filtered_path_answers_inside_behind_and_tied_across_the_sample_boundary():
    nq, npool, k, D = 129, 32768, 50, 64
    S = sample_rows(npool)
    assert S == 4096
    Q, P = O.lattice(53, nq, D, -8, 8), O.lattice(54, npool, D, -8, 8)

    def near(q, n, seed):                       # n rows at d2 = 1 or 2 from query q
        r = np.repeat(Q[q:q + 1], n, 0)
        gg = np.random.default_rng(seed)
        r[np.arange(n), gg.integers(0, D // 2, n)] += 1
        r[np.arange(n), D // 2 + gg.integers(0, D // 2, n)] -= gg.integers(0, 2, n).astype(np.float32)
        return r
    P[100:100 + k] = near(0, k, 1)                              # query 0: wholly inside the sample
    P[S + 1000:S + 1000 + k] = near(1, k, 2)                    # query 1: wholly behind it
    P[S - 30:S + 30] = near(2, 60, 3)                           # query 2: tied (d2 = 1 / 2, many times) across row S
    P[S - 1] = P[S] = P[S + 1] = Q[5]                           # query 5: three zero distances around row S
    P[20000] = P[50]                                            # and a duplicate pair sample / rest for whoever is near it
    Q[6] = P[50]
    cnt = filter_counts(Q, P, k)
    assert cnt.max() <= FCAP, "test construction"
    ei, ed2 = both_paths_exact(Q, P, k)
    assert set(ei[0]) == set(range(100, 100 + k)) and set(ei[1]) == set(range(S + 1000, S + 1000 + k))
    assert set(ei[2]) <= set(range(S - 30, S + 30)) and ei[2].min() < S <= ei[2].max()
    assert ei[5, :3].tolist() == [S - 1, S, S + 1] and ei[6, :2].tolist() == [50, 20000] and (ed2[6, :2] == 0).all()


# ------------------------------------------------------------------------------------------------ sharding + merge
def merge(idx_parts, dist_parts):
    lib = L.load()
    parts, nq, k = idx_parts.shape
    ii, dd = dev(idx_parts), dev(dist_parts)
    idx = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
    dist = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
    L.check(lib.ofx_topk_merge(ii.data_ptr(), dd.data_ptr(), parts, nq, k, idx.data_ptr(), dist.data_ptr(), stream()), "ofx_topk_merge")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dist.cpu().numpy()


def shard_cases():
    out = []
    for parts in (1, 2, 3, 8):
        out.append((f"equal{parts}", 20001, 64, 50, -8, 8, parts))
    out.append(("uneven", 20001, 64, 50, -8, 8, "uneven"))
    out.append(("uneven-ties", 9000, 32, 127, -1, 1, "uneven"))
    out.append(("limit-8x128", 32800, 64, 128, -8, 8, 8))              # parts * k = 1024; the unsharded call takes the filtered path
    out.append(("limit-8x128-ties", 8 * 600, 32, 128, -1, 1, 8))
    return out


@pytest.mark.parametrize("name,npool,D,k,lo,hi,how", shard_cases(), ids=[c[0] for c in shard_cases()])
def test_topk_sharded_merge_equals_unsharded_equals_reference(name, npool, D, k, lo, hi, how):
    nq = 129
    Q, P = O.lattice(70 + D, nq, D, lo, hi), O.lattice(71 + npool, npool, D, lo, hi)
    if how == "uneven":
        cuts = [0, k, k + 129, k + 129 + 4096, npool]
    else:
        cuts = [npool * i // how for i in range(how + 1)]
    starts = cuts[:-1]
    for s in starts:                                             # identical rows in different shards: ties across shard boundaries
        P[s + 5] = P[3]
        P[s + 9] = Q[1]
    Q[0] = P[3]
    ui, ud = topk(Q, P, k)
    ei, ed2 = assert_exact(ui, ud, Q, P, k)
    pi, pd = zip(*[topk(Q, P[a:b], k, index_base=a) for a, b in zip(cuts[:-1], cuts[1:])])
    mi, md = merge(np.stack(pi), np.stack(pd))
    assert np.array_equal(mi, ui) and same_bits(md, ud)
    z = np.sort(np.r_[3, np.array(starts) + 5])[:k]             # query 0's zero distances: one or two rows in every shard
    assert np.array_equal(ei[0, :len(z)], z) and (ed2[0, :len(z)] == 0).all()


def test_topk_merge_with_a_64_bit_index_base():
    Q, P = O.lattice(80, 5, 32, -1, 1), O.lattice(81, 600, 32, -1, 1)
    k = 50
    pi, pd = zip(*[topk(Q, P[a:a + 200], k, index_base=BIG + a) for a in (0, 200, 400)])
    mi, md = merge(np.stack(pi), np.stack(pd))
    assert_exact(mi, md, Q, P, k, BIG)


# ------------------------------------------------------------------------------------------------ FITB
FITB_CASES = [
    # B, C, D, lo, hi
    (1, 1, 4, -8, 8), (3, 2, 8, -8, 8), (4, 4, 252, -8, 8), (5, 7, 256, -8, 8), (1024, 4, 260, -8, 8), (1024, 33, 1024, -8, 8),
    (16385, 4, 8, -8, 8), (20000, 7, 4, -8, 8), (5, 33, 4100, -2, 2), (3, 1, 1024, -8, 8), (4, 2, 4100, -2, 2), (1, 7, 252, -8, 8),
    (1024, 1, 256, -8, 8), (5, 4, 1024, -8, 8), (16385, 2, 4, -1, 1), (20000, 1, 8, -8, 8), (3, 33, 260, -8, 8), (4, 7, 8, -1, 1),
    (1, 4, 4100, -2, 2), (1024, 2, 252, -8, 8),
]


def fitb(y, cand, with_dist):
    lib = L.load()
    B, Cn, D = cand.shape
    yd, cd = dev(y), dev(cand)
    idx = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    dist = torch.full((B, Cn), float("nan"), dtype=torch.float32, device="cuda") if with_dist else None
    rc = lib.ofx_fitb_argmin(yd.data_ptr(), cd.data_ptr(), B, Cn, D, idx.data_ptr(), dist.data_ptr() if with_dist else None, stream())
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), dist.cpu().numpy() if with_dist else None


@pytest.mark.parametrize("B,Cn,D,lo,hi", FITB_CASES)
def test_fitb_argmin_exact_on_the_lattice(B, Cn, D, lo, hi):
    """D / 4 below, at and not a multiple of the wavefront; C other than 4; B not a multiple of the 4 rows of a block, and B > 16384 (the
    grid-stride loop); duplicate candidates (first minimum wins); y equal to a candidate (distance +0.0); with and without `dist`."""
    y, cand = O.lattice(B + D, B, D, lo, hi), O.lattice(B + D + Cn, B * Cn, D, lo, hi).reshape(B, Cn, D)
    if Cn >= 2:
        cand[::3, Cn - 1] = cand[::3, 0]                          # duplicates: the later copy never wins
        cand[1::5, Cn // 2] = y[1::5]                             # exact hits
        cand[B - 1, 1] = cand[B - 1, 0] = y[B - 1]                # two exact hits: the first
    ei, ed2 = O.fitb_argmin_exact(y, cand)
    for with_dist in (False, True):
        rc, idx, dist = fitb(y, cand, with_dist)
        assert rc == 0
        assert np.array_equal(idx, ei)
    assert same_bits(dist, f32_sqrt(ed2))
    if Cn >= 2:
        assert ei[B - 1] == 0 and dist[B - 1, 0].view(np.uint32) == 0 and dist[B - 1, 1].view(np.uint32) == 0
        dup = np.setdiff1d(np.arange(0, B - 1, 3), np.arange(1, B, 5))           # rows whose last candidate still copies their first
        assert (ei[dup] != Cn - 1).all() and (ed2[dup, 0] == ed2[dup, Cn - 1]).all()


# ------------------------------------------------------------------------------------------------ rejections
def last_error():
    return L.load().ofx_last_error().decode()


def test_l2_topk_and_merge_reject_what_they_cannot_run():
    """Return code and a fragment of ofx_last_error(); a rejected call launches nothing: the poisoned outputs are untouched."""
    Q, P = O.lattice(90, 8, 64, -8, 8), O.lattice(91, 50, 64, -8, 8)
    Qd, Pd = dev(Q), dev(P)

    def untouched(idx, dist):
        return bool((idx == -1).all()) and bool(torch.isnan(dist).all())
    for D, k, code, frag in ((48, 5, OFX_ESHAPE, "multiple of 32"), (64, 0, OFX_ESHAPE, "k=0"), (64, 129, OFX_ESHAPE, "k=129"),
                             (64, 51, OFX_ESHAPE, "k=51")):
        rc, idx, dist = raw_topk(Qd, Pd, 8, 50, D, k)
        assert rc == code and frag in last_error(), (D, k, rc, last_error())
        assert untouched(idx, dist)
    Q4 = dev(np.concatenate([np.zeros(1, np.float32), Q.ravel()]))
    assert Q4.data_ptr() % 16 == 0
    rc, idx, dist = raw_topk(Q4.data_ptr() + 4, Pd, 8, 50, 64, 5)
    assert rc == OFX_EINVAL and "16-byte aligned" in last_error() and untouched(idx, dist)
    rc, idx, dist = raw_topk(Qd, Pd, 8, 50, 64, 5, ws_short=1)
    assert rc == OFX_EWORKSPACE and "workspace" in last_error() and untouched(idx, dist)
    rc, idx, dist = raw_topk(Qd, Pd, 8, 50, 64, 5, idx_null=True)
    assert rc == OFX_EINVAL and "NULL" in last_error() and untouched(idx, dist)
    rc, idx, dist = raw_topk(Qd, Pd, 8, 50, 64, 5)              # and the same call, unspoiled, runs
    assert rc == 0
    assert_exact(idx.cpu().numpy(), dist.cpu().numpy(), Q, P, 5)
    lib = L.load()
    for parts, k in ((9, 128), (1025, 1), (8, 129)):
        ii = torch.zeros(parts, 1, k, dtype=torch.int64, device="cuda"); dd = torch.zeros(parts, 1, k, device="cuda")
        oi = torch.full((1, k), -1, dtype=torch.int64, device="cuda"); od = torch.full((1, k), float("nan"), device="cuda")
        rc = lib.ofx_topk_merge(ii.data_ptr(), dd.data_ptr(), parts, 1, k, oi.data_ptr(), od.data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == OFX_ESHAPE and f"parts*k={parts * k}" in last_error() and untouched(oi, od)


def test_fitb_rejects_a_row_length_that_is_not_a_multiple_of_4():
    y, cand = O.lattice(92, 4, 6, -8, 8), O.lattice(93, 8, 6, -8, 8).reshape(4, 2, 6)
    rc, idx, _ = fitb(y, cand, True)
    assert rc == OFX_EINVAL and "fitb_argmin" in last_error() and (idx == -1).all()


# ------------------------------------------------------------------------------------------------ non-finite rows
def spoil(P, rows, seed, vals=(np.nan, np.inf, -np.inf)):
    """Overwrite one coordinate of each of `rows` with NaN, +inf, -inf in turn."""
    g = np.random.default_rng(seed)
    vals = np.array(vals, np.float32)
    P[rows, g.integers(0, P.shape[1], len(rows))] = vals[np.arange(len(rows)) % len(vals)]


def assert_non_finite_rows_last(idx, dist, Q, P, k, bad, base=0):
    """The reference's rule as properties (NaN versus inf is not pinned): the first min(k, #finite rows) entries are the exact answer on
    the finite rows alone; what follows has a non-finite distance and the index of a non-finite row; no index repeats."""
    finite = np.setdiff1d(np.arange(len(P)), bad)
    m = min(k, len(finite))
    if m:
        ei, ed2 = O.l2_topk_exact(Q, P[finite], m)
        assert np.array_equal(idx[:, :m], finite[ei] + base)
        assert same_bits(dist[:, :m], f32_sqrt(ed2))
    assert not np.isfinite(dist[:, m:]).any()
    assert np.isin(idx[:, m:] - base, bad).all()
    assert all(len(set(r)) == k for r in idx.tolist())


@pytest.mark.parametrize("npool,k,n_bad", [(1001, 50, 9), (130, 128, 10), (4099, 128, 4000), (129, 129 - 1, 129)])
def test_topk_matrix_path_sorts_non_finite_pool_rows_last(npool, k, n_bad):
    """One corrupt embedding must not become every query's best match (parent commit: its distance came out as 0)."""
    Q, P = O.lattice(100, 129, 64, -8, 8), O.lattice(101 + npool, npool, 64, -8, 8)
    bad = np.sort(np.random.default_rng(npool).choice(npool, n_bad, replace=False))
    spoil(P, bad, 7)
    idx, dist = topk(Q, P, k, 7)
    assert_non_finite_rows_last(idx, dist, Q, P, k, bad, 7)


@pytest.mark.parametrize("filtered", [1, 0])
def test_topk_large_pool_sorts_non_finite_pool_rows_last(filtered):
    nq, npool, k = 129, 40000, 50
    Q, P = O.lattice(110, nq, 64, -8, 8), O.lattice(111, npool, 64, -8, 8)
    bad = np.sort(np.random.default_rng(5).choice(npool, 300, replace=False))
    assert (bad < sample_rows(npool)).sum() >= 9 and (bad >= sample_rows(npool)).sum() >= 9
    spoil(P, bad, 8)
    idx, dist = topk(Q, P, k, 0, filtered)
    assert_non_finite_rows_last(idx, dist, Q, P, k, bad)


@pytest.mark.parametrize("vals", [(np.nan,), (np.nan, np.inf, -np.inf)], ids=["nan", "mixed"])
@pytest.mark.parametrize("filtered", [1, 0])
def test_topk_finite_rows_behind_a_mostly_non_finite_sample_are_found(filtered, vals):
    """The first S rows hold k - 1 finite rows only, so the sample's k-th distance - the filter threshold - is not a number (NaN rows
    only) or not a finite one: the finite rows behind the sample must still be found."""
    nq, npool, k = 129, 32768, 50
    S = sample_rows(npool)
    Q, P = O.lattice(120, nq, 64, -8, 8), O.lattice(121, npool, 64, -8, 8)
    keep = np.sort(np.random.default_rng(6).choice(S, k - 1, replace=False))
    bad = np.setdiff1d(np.arange(S), keep)
    spoil(P, bad, 9, vals)
    idx, dist = topk(Q, P, k, 0, filtered)
    assert_non_finite_rows_last(idx, dist, Q, P, k, bad)
    assert np.isfinite(dist).all() and (idx >= S).any(1).all()


@pytest.mark.parametrize("npool", [1001, 40000])
def test_topk_query_with_a_nan(npool):
    """Nothing is defined for such a query but that the call answers: indices in range and distinct, distances not numbers; its
    neighbours in the panel are exact."""
    k = 50
    Q, P = O.lattice(130, 129, 64, -8, 8), O.lattice(131, npool, 64, -8, 8)
    Qn = Q.copy()
    Qn[[0, 77, 128], [3, 0, 63]] = np.nan
    for filtered in (1, 0):
        idx, dist = topk(Qn, P, k, 0, filtered)
        ok = np.setdiff1d(np.arange(129), [0, 77, 128])
        assert_exact(idx[ok], dist[ok], Q[ok], P, k)
        for q in (0, 77, 128):
            assert ((idx[q] >= 0) & (idx[q] < npool)).all() and len(set(idx[q].tolist())) == k
            assert not np.isfinite(dist[q]).any()


def test_fitb_first_nan_distance_wins():
    """torch.cdist(...).argmin(-1) returns the index of the first NaN; +inf is an ordinary (largest) number."""
    B, Cn, D = 1030, 7, 260
    y, cand = O.lattice(140, B, D, -8, 8), O.lattice(141, B * Cn, D, -8, 8).reshape(B, Cn, D)
    ei, ed2 = O.fitb_argmin_exact(y, cand)
    want = ei.copy()
    cand[0, 3, 5] = np.nan; want[0] = 3
    cand[1, 6, 259] = np.nan; cand[1, 2, 0] = np.nan; want[1] = 2
    cand[2, 0, 1] = np.nan; want[2] = 0
    cand[1029, 5, 7] = np.nan; cand[1029, 6, 7] = np.nan; want[1029] = 5
    y[5, 9] = np.nan; want[5] = 0                                  # every distance NaN: the first
    cand[6, :, 4] = np.inf; want[6] = 0                            # every distance +inf: the first
    inf_c = (ei[7] + 1) % Cn
    cand[7, inf_c, 2] = -np.inf                                    # one +inf distance beside the minimum: changes nothing
    for with_dist in (False, True):
        rc, idx, dist = fitb(y, cand, with_dist)
        assert rc == 0
        assert np.array_equal(idx, want)
    clean = np.setdiff1d(np.arange(B), [0, 1, 2, 5, 6, 7, 1029])
    assert same_bits(dist[clean], f32_sqrt(ed2[clean]))
    assert np.isnan(dist[0, 3]) and np.isnan(dist[1, [2, 6]]).all() and np.isnan(dist[5]).all() and np.isinf(dist[6]).all()
    assert np.isinf(dist[7, inf_c]) and np.isfinite(np.delete(dist[7], inf_c)).all()
