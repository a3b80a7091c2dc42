"""What tests/gemm_tn_cases.py claims of every case, checked without a GPU: the exactness condition (so that bit equality with the
float64 product is the right criterion on the device), that the operands survive the operand type, that the guards are where the
module says, that the launcher's own preconditions hold, and that the split count (tests/gemm_plan_ref.py's tn_splits, which
tests/test_gemm_plan.py pins to csrc/gemm_plan.h) and the kernel's documented k-partition of the live rows give each case the
per-split k-tile counts, the empty splits and the partial k-tile it is in the table for."""
import numpy as np
import pytest
import torch

import gemm_plan_ref as R
import gemm_tn_cases as T

TD = {"bf16": torch.bfloat16, "f16": torch.float16}


def _roundtrip(a, td):
    return torch.from_numpy(np.array(a)).to(td).float().numpy()


@pytest.mark.parametrize("group", list(T.GROUPS))
def test_every_case_is_exact_representable_and_has_its_partition(group):
    for c in T.GROUPS[group]:
        d = T.build(c)
        live, Kp = T.live_rows(c), T.round_up(c.K, 64)
        mv, nv = c.m_valid or c.M, c.n_valid or c.N
        # ---- the exactness condition
        assert d["bound"] < 2.0 ** 24, (c.name, d["bound"])
        assert d["want"].shape == (mv, nv) and np.array_equal(d["want"], np.round(d["want"])), c.name
        # ---- operands are what the operand type holds (the infinities too; NaN has no single image)
        td = TD[c.dt]
        for buf in (d["a"], d["b"], np.where(np.isnan(d["A"]), np.float32(0), d["A"]), np.where(np.isnan(d["B"]), np.float32(0), d["B"])):
            assert np.array_equal(_roundtrip(buf, td), buf), c.name
        if c.family == "ints":
            assert max(np.abs(d["a"]).max(initial=0), np.abs(d["b"]).max(initial=0)) <= 7
        if d["prefill"] is not None:
            assert d["prefill"].shape == (mv, c.ldc) and np.abs(d["prefill"]).max() <= 64 and np.array_equal(d["prefill"], np.round(d["prefill"]))
        assert (d["prefill"] is not None) == bool(c.accumulate)
        # ---- guards
        assert d["A"].shape == (Kp, c.lda) and d["B"].shape == (Kp, c.ldb) and 0 <= live <= c.K and d["live"] == live
        for buf, cols, blk in ((d["A"], c.M, d["a"]), (d["B"], c.N, d["b"])):
            assert np.array_equal(buf[:live, :cols], blk) and np.isnan(buf[:, cols:]).all(), c.name
            r = np.arange(live, Kp)
            assert np.isnan(buf[r[r % 2 == 0], :cols]).all() and (buf[r[r % 4 == 1], :cols] == np.inf).all() and (buf[r[r % 4 == 3], :cols] == -np.inf).all(), c.name
        # ---- the launcher's preconditions (ofx_launch_gemm_tn)
        assert c.M > 0 and c.N > 0 and c.K > 0 and c.M % 256 == 0 and c.N % 256 == 0, c.name
        assert c.lda >= c.M and c.ldb >= c.N and c.lda % 8 == 0 and c.ldb % 8 == 0, c.name
        assert c.ldc % 4 == 0 and nv % 4 == 0 and c.ldc >= nv and mv <= c.M and nv <= c.N, c.name
        assert c.entry == "into" or not (c.m_valid or c.n_valid or c.accumulate), c.name
        # ---- the plan
        if c.slab:
            assert R.tn_splits(c.M, c.N, c.K) == c.splits > 1, (c.name, R.tn_splits(c.M, c.N, c.K))
        else:
            assert c.splits == 1, c.name
        assert c.blocks == (c.M // 256) * (c.N // 256) * c.splits
        # ---- the k-partition of the live rows
        parts, tail = T.tn_partition(live, c.splits)
        assert (parts, tail) == (c.parts, c.tail), (c.name, parts, tail)
        assert len(parts) == c.splits and sum(parts) == (live + 63) // 64
        if tail:
            s, rows = tail
            assert 0 < rows < 64 and parts[s] > 0 and not any(parts[s + 1:]) and 64 * (sum(parts) - 1) + rows == live
        # ---- the census digits of the expected result
        if c.family == "census":
            assert c.K == T.CENSUS_K and not c.accumulate and live == c.K
            assert {T.census_digits(v, c) for v in np.unique(d["want"])} == {"1" * (c.K // 32)}, c.name


def _where(**kw):
    return [c for c in T.CASES if all(getattr(c, k) == v for k, v in kw.items())]


def test_tn_partition_restates_the_kernel_rule():
    assert T.tn_partition(0, 3) == ((0, 0, 0), None)
    assert T.tn_partition(65, 3) == ((1, 1, 0), (1, 1))
    assert T.tn_partition(300, 3) == ((2, 2, 1), (2, 44))
    assert T.tn_partition(1088, 9) == ((2,) * 8 + (1,), None)
    assert T.tn_partition(1100, 3) == ((6, 6, 6), (2, 12))
    assert T.tn_partition(200, 1) == ((4,), (0, 8))
    for live in range(0, 1200, 7):
        for s in (1, 2, 3, 4, 9, 16):
            parts, tail = T.tn_partition(live, s)
            per = max(parts)
            assert sum(parts) == (live + 63) // 64 and all(p == per for p in parts[:sum(parts) // per if per else 0])


def test_the_table_covers_what_it_is_for():
    """Every path the kernel and its launcher have, in both operand types."""
    for dt in T.DTYPES:
        direct = _where(dt=dt, slab=False, kdev=None, family="ints", M=256, N=256, entry="tn")
        assert {c.K for c in direct} >= {1, 63, 64, 65, 128, 192, 200, 256, 320, 512}
        assert {c.parts[0] for c in direct} >= {1, 2, 3, 4, 5, 8} and {c.tail[1] for c in direct if c.tail} == {1, 8, 63}
        # the group_m = 4 walk: a second group, a short group, more than one tile column; one of them on padded strides, A's rows
        # 16-byte but not 32-byte aligned
        walk = _where(dt=dt, slab=False, K=192, kdev=None, m_valid=0)
        assert {(c.M // 256, c.N // 256) for c in walk} >= {(5, 1), (2, 3), (6, 2)}
        assert any(c.lda == c.M + 8 and c.ldb == c.N + 16 and (2 * c.lda) % 32 == 16 and c.M // 256 > 4 for c in walk)
        # split-K as planned: one k-tile per split, several with a short last split, several with a partial last tile, block counts off the XCD count
        planned = {(c.M, c.N, c.K): c for c in _where(dt=dt, slab=True, kdev=None, m_valid=0, family="ints", entry="tn")}
        assert planned[(256, 256, 200)].parts == (1, 1, 1, 1) and planned[(256, 256, 1088)].parts == (2,) * 8 + (1,)
        assert planned[(1280, 768, 576)].parts == (3, 3, 3) and planned[(1280, 768, 576)].blocks == 45
        assert planned[(1280, 768, 1024)].parts == (4, 4, 4, 4)
        assert planned[(1280, 768, 1100)].parts == (6, 6, 6) and planned[(1280, 768, 1100)].tail == (2, 12)
        assert planned[(1536, 1536, 1024)].parts == (8, 8) and planned[(1536, 1536, 1024)].blocks == 72
        for c in planned.values():                                              # each next to the unsplit launch of the same arrays
            assert len(_where(dt=dt, slab=False, kdev=None, m_valid=0, M=c.M, N=c.N, K=c.K, lda=c.lda, family="ints")) >= 1
        # the device-side live row count
        M, N, K = T.LIVE_SHAPE
        live = {c.kdev: c for c in _where(dt=dt, slab=True, M=M, N=N, K=K, m_valid=0)}
        assert set(live) == {0, 1, 63, 64, 65, 129, 300, 576, 1087, 1088, 5000} and all(c.splits == 3 for c in live.values())
        assert live[65].parts == (1, 1, 0) and live[65].tail == (1, 1) and live[300].parts == (2, 2, 1) and live[300].tail == (2, 44)
        assert live[0].parts == (0, 0, 0) and live[5000].parts == live[1088].parts and T.live_rows(live[5000]) == K
        assert {c.kdev for c in _where(dt=dt, slab=False, M=M, N=N, K=K, m_valid=0)} == {0, 65, 300}
        # a split that starts at an odd k-tile, owns an even number of them and ends in the partial one: where a stage parity taken from
        # the absolute k-tile index goes wrong
        assert any(c.tail and sum(c.parts[:c.tail[0]]) % 2 == 1 and c.parts[c.tail[0]] % 2 == 0 for c in _where(dt=dt, slab=True))
        # valid extent and accumulate
        into = _where(dt=dt, entry="into", m_valid=1100, n_valid=700, M=1280, N=768)
        assert {(c.ldc, c.slab, c.K, c.accumulate) for c in into if c.kdev is None} == {(l, s, k, a) for l in (700, 772) for s, k in ((False, 192), (True, 576)) for a in (0, 1)}
        assert any(c.accumulate and c.kdev == 300 for c in into) and any(c.accumulate and c.kdev == 0 and c.slab for c in into)
        assert 1100 // 256 == 4 and 1100 % 256 and 700 % 256                     # both cuts fall inside a tile
        # the entry points, on one set of arrays
        e = _where(dt=dt, m_valid=0, n_valid=0, accumulate=0, M=1280, N=768, K=576, kdev=None, family="ints", lda=1280)
        assert {(c.entry, c.slab) for c in e} >= {("tn", False), ("into", False), ("tn", True), ("into", True)}
        # census
        cen = _where(dt=dt, family="census")
        assert {(c.M, c.N, c.slab, c.parts) for c in cen} == {(256, 256, False, (8,)), (256, 256, True, (1,) * 8), (1280, 768, False, (8,))}


def test_reassociated_float32_sums_equal_the_integer_result():
    """The condition at work: float32 sums of one case's products and prefill in random chunk orders (what split-K planes are) are
    bit-equal to the float64 `@`."""
    c = next(c for c in T.CASES if c.accumulate and c.kdev is None and c.slab)
    d = T.build(c)
    g = np.random.default_rng(0)
    terms = (d["a"][:, :64, None] * d["b"][:, None, :64]).astype(np.float32)       # [k, m, n]
    for _ in range(4):
        acc = np.zeros((64, 64), np.float32)
        for chunk in np.array_split(g.permutation(terms.shape[0]), 7):
            part = np.zeros((64, 64), np.float32)
            for k in chunk:
                part += terms[k]
            acc += part
        assert np.array_equal((acc + d["prefill"][:64, :64]).astype(np.float64), d["want"][:64, :64])
