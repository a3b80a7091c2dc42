"""The exact host reference of the scoring kernels (oracle/np_oracle.py: lattice, l2_topk_exact,
fitb_argmin_exact) against the reference's own calls, torch.cdist + torch.topk(largest=False) /
argmin, on the CPU.  tests/test_gpu_scoring.py takes its expectations from these functions, so what
is pinned here is what the kernels are held to - including where non-finite rows go."""
import numpy as np
import pytest
import torch

from oracle import np_oracle as O


def f32_sqrt(d2):
    """float32(sqrt(float64 d2)): the correctly rounded fp32 square root of an exact d2 (53 >= 2 * 24 + 2 bits: no double rounding)."""
    return np.sqrt(np.asarray(d2, np.float64)).astype(np.float32)


def assert_same_distances(td, d2):
    """torch's fp32 distances against the exact d2.  The d2 inside torch.cdist is exact on the lattice and is recovered exactly from the
    distance (d < 2^9, so one ulp of d moves d^2 by < 0.04): that comparison is bit for bit.  The distance itself is compared with the
    correctly rounded root to <= 1 ulp, because torch's vectorised fp32 sqrt on the CPU is not correctly rounded (measured with the
    installed torch: 191 of 40,040 lattice distances are one ulp off float32(sqrt(float64 d2)); torch.sqrt of the exact d2 gives the same
    191, numpy's fp32 sqrt and cdist's direct-form path give none)."""
    td = np.asarray(td, np.float32)
    assert np.array_equal(np.rint(td.astype(np.float64) ** 2), np.asarray(d2, np.float64))
    assert np.abs(td.view(np.int32).astype(np.int64) - f32_sqrt(d2).view(np.int32)).max(initial=0) <= 1


def test_lattice_is_integer_valued_seeded_and_asserts_its_bounds():
    x = O.lattice(3, 100, 64, -8, 8)
    assert x.dtype == np.float32 and x.shape == (100, 64)
    assert (x == np.rint(x)).all() and x.min() == -8 and x.max() == 8
    assert np.array_equal(x, O.lattice(3, 100, 64, -8, 8)) and not np.array_equal(x, O.lattice(4, 100, 64, -8, 8))
    with pytest.raises(AssertionError):
        O.lattice(0, 4, 1024, -128, 128)          # 2 D max^2 = 2^25
    with pytest.raises(AssertionError):
        O.lattice(0, 64, 4096, -8, 8)             # 4 |row|^2 ~ 3.9e5: a d2 may pass 2^18
    O.lattice(0, 8, 1024, -8, 8); O.lattice(0, 8, 2048, -4, 4); O.lattice(0, 8, 4100, -2, 2)


@pytest.mark.parametrize("nq,npool,D,k,lo,hi", [(5, 50, 32, 50, -1, 1), (40, 1001, 64, 50, -8, 8), (3, 129, 96, 128, -8, 8),
                                                  (30, 5000, 1024, 50, -8, 8), (7, 300, 2048, 1, -4, 4), (1, 1, 32, 1, -8, 8)])
def test_l2_topk_exact_equals_torch_cdist_topk_on_the_lattice(nq, npool, D, k, lo, hi):
    Q, P = O.lattice(nq + D, nq, D, lo, hi), O.lattice(npool + D, npool, D, lo, hi)
    if npool >= 40:
        Q[0] = P[npool // 2]                                                   # a zero distance
        P[npool - 3] = P[4]                                                    # an exact duplicate
    idx, d2 = O.l2_topk_exact(Q, P, k)
    assert idx.dtype == np.int64 and d2.dtype == np.float64 and idx.shape == d2.shape == (nq, k)
    # the direct form in plain float64, and a stable sort, whichever form the helper took
    full = ((Q[:, None, :].astype(np.float64) - P[None].astype(np.float64)) ** 2).sum(-1)
    order = np.argsort(full, axis=1, kind="stable")[:, :k]
    assert np.array_equal(idx, order) and np.array_equal(d2, np.take_along_axis(full, order, 1))
    # the reference's call: distances bit for bit, index sets per distinct distance (torch's order inside a tie is unspecified)
    td, ti = torch.topk(torch.cdist(torch.from_numpy(Q), torch.from_numpy(P)), k, dim=-1, largest=False)
    td, ti = td.numpy(), ti.numpy()
    assert_same_distances(td, d2)
    td2 = np.rint(td.astype(np.float64) ** 2)
    for q in range(nq):
        last = d2[q, -1]
        for v in np.unique(d2[q]):
            ours, theirs = set(idx[q, d2[q] == v]), set(ti[q, td2[q] == v])
            if v < last:
                assert ours == theirs
            else:                                                              # the tie that k cuts: ours holds its smallest rows
                assert len(ours) == len(theirs) and theirs <= set(np.flatnonzero(full[q] == v))
                assert sorted(ours) == list(np.flatnonzero(full[q] == v)[:len(ours)])
    # the fp32 oracle agrees on indices exactly (its sums are exact here) ...
    oi, od = O.l2_topk(Q, P, k)
    assert np.array_equal(oi, idx) and np.array_equal(od.view(np.uint32), f32_sqrt(d2).view(np.uint32))
    # ... and index_base is an offset
    assert np.array_equal(O.l2_topk_exact(Q, P, k, index_base=2 ** 33)[0], idx + 2 ** 33)


def test_l2_topk_exact_direct_form_on_real_valued_inputs():
    g = np.random.default_rng(5)
    Q, P = g.standard_normal((4, 48)).astype(np.float32), g.standard_normal((300, 48)).astype(np.float32)
    idx, d2 = O.l2_topk_exact(Q, P, 10)
    full = ((Q[:, None, :].astype(np.float64) - P[None].astype(np.float64)) ** 2).sum(-1)
    order = np.argsort(full, axis=1, kind="stable")[:, :10]
    assert np.array_equal(idx, order) and np.allclose(d2, np.take_along_axis(full, order, 1), rtol=1e-15, atol=0)
    with pytest.raises(AssertionError):
        P[3, 3] = np.nan
        O.l2_topk_exact(Q, P, 10)


@pytest.mark.parametrize("B,C,D,lo,hi", [(1, 1, 4, -8, 8), (5, 7, 260, -8, 8), (64, 4, 1024, -8, 8), (9, 33, 4100, -2, 2), (300, 2, 8, -1, 1)])
def test_fitb_argmin_exact_equals_torch_cdist_argmin(B, C, D, lo, hi):
    y, cand = O.lattice(B + D, B, D, lo, hi), O.lattice(B + D + 1, B * C, D, lo, hi).reshape(B, C, D)
    if C >= 4:
        cand[0, 3] = cand[0, 1]                                                # duplicate candidates
        cand[B - 1, 2] = y[B - 1]                                              # y equal to a candidate
    idx, d2 = O.fitb_argmin_exact(y, cand)
    d = torch.cdist(torch.from_numpy(y)[:, None, :], torch.from_numpy(cand)).squeeze(1)
    assert_same_distances(d.numpy(), d2)
    assert np.array_equal(idx, d.argmin(-1).numpy())
    assert np.array_equal(idx, O.fitb_argmin(y, cand)[0])
    if C >= 4:
        assert d2[B - 1, 2] == 0 and idx[B - 1] == 2 and idx[0] != 3


def test_reference_sorts_non_finite_rows_last_and_argmin_returns_the_first_nan():
    """What the reference does with a corrupt embedding, pinned with the installed torch: torch.cdist gives NaN / inf for a pool row that holds
    one, torch.topk(largest=False) sorts such rows BEHIND every finite distance, and argmin returns the index of the FIRST NaN."""
    Q, P = O.lattice(1, 6, 64, -8, 8), O.lattice(2, 200, 64, -8, 8)
    bad = {7: np.nan, 50: np.inf, 51: -np.inf, 199: np.nan}
    for r, v in bad.items():
        P[r, 5] = v
    finite = np.array([r for r in range(200) if r not in bad])
    d = torch.cdist(torch.from_numpy(Q), torch.from_numpy(P))
    assert not torch.isfinite(d[:, list(bad)]).any() and torch.isfinite(d[:, finite]).all()
    k = 198
    td, ti = torch.topk(d, k, dim=-1, largest=False)
    ei, ed2 = O.l2_topk_exact(Q, P[finite], len(finite))
    assert_same_distances(td[:, :196].numpy(), ed2)
    assert not torch.isfinite(td[:, 196:]).any()
    for q in range(6):
        assert set(ti[q, 196:].tolist()) <= set(bad) and len(set(ti[q].tolist())) == k
        assert sorted(ti[q, :196].tolist()) == sorted(finite[ei[q]].tolist())
    # one NaN among few finite rows is still last, not first
    td, ti = torch.topk(d[:, 5:9], 4, dim=-1, largest=False)
    assert (ti[:, 3] == 2).all() and torch.isnan(td[:, 3]).all()
    # argmin: the first NaN wins over every finite distance and over a later NaN; +inf does not
    y, cand = O.lattice(3, 4, 32, -8, 8), O.lattice(4, 4 * 5, 32, -8, 8).reshape(4, 5, 32)
    cand[0, 3, 0] = np.nan
    cand[1, 1, 2] = np.nan; cand[1, 4, 2] = np.nan
    cand[2, 0, 0] = np.inf
    fd = torch.cdist(torch.from_numpy(y)[:, None, :], torch.from_numpy(cand)).squeeze(1)
    am = fd.argmin(-1).numpy()
    ei, _ = O.fitb_argmin_exact(y[3:], cand[3:])
    assert am[0] == 3 and am[1] == 1 and am[3] == ei[0]
    assert torch.isinf(fd[2, 0]) and am[2] == 1 + int(fd[2, 1:].argmin())
