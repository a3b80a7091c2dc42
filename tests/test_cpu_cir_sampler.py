"""The draw of ofx_cir_sample_batch, checked on its numpy restatement (tests/cir_sampler_ref.py) - the kernel is held to that restatement
bit for bit in tests/test_gpu_cir_sampler.py, so what holds here holds for the kernel: structure (negatives from the target's pool, never
the target, distinct; short pools; the remainder a truncated permutation; repeatability), uniformity at B = 40,000 under one fixed seed
within 4.5 sigma of the binomial, and the host side of outfitx_amd/sampler.py (the pools' CSR arrays, every ValueError).  No GPU."""
import itertools

import numpy as np
import pytest

import cir_sampler_ref as R

SEED, B_STAT, SIGMA = 1234, 40000, 4.5


def make_world(seed, n_table=400, n_keys=7, n_outfits=50, lone_key=True):
    """A table with pools of mixed sizes (one of a single row when lone_key), rows without a pool, and outfits of 2 .. 20 items."""
    g = np.random.default_rng(seed)
    key = g.integers(0, n_keys, n_table) * 3 + 1                        # keys need not be 0 .. G - 1
    key[g.random(n_table) < 0.05] = -1
    if lone_key:
        key[7] = 1000
    outfits = [g.choice(n_table, int(g.integers(2, 21)), replace=False).tolist() for _ in range(n_outfits)]
    pos = [sorted(g.choice(len(o), int(g.integers(1, len(o) + 1)), replace=False).tolist()) for o in outfits]
    return key, outfits, pos


def test_negatives_come_from_the_targets_pool_without_the_target_and_without_repeats():
    key, outfits, pos = make_world(1)
    outfits[0][0] = 7; pos[0] = [0]                                     # a target alone in its pool
    split, pools = R.build_split(outfits, pos), R.build_pools(key)
    ids = np.random.default_rng(2).integers(0, len(outfits), 600); ids[0] = 0
    for K in (1, 10, 64):
        item, cu, tgt, neg = R.sample_batch(split, pools, ids, SEED, 3, K, 16)
        for b in range(len(ids)):
            o = outfits[ids[b]]
            assert tgt[b] in [o[p] for p in pos[ids[b]]]
            others = [r for r in np.flatnonzero(key == key[tgt[b]]).tolist() if r != tgt[b]] if key[tgt[b]] >= 0 else []
            got = neg[b].tolist()
            if len(others) >= K:
                assert -1 not in got and len(set(got)) == K and set(got) <= set(others), (b, K)
            else:
                assert got == others + [-1] * (K - len(others)), (b, K)     # all the others in pool order, then -1
        assert neg[0].tolist() == [-1] * K


def test_the_remainder_is_a_truncated_permutation_of_the_outfit_without_the_positive():
    key, outfits, pos = make_world(3)
    split, pools = R.build_split(outfits, None), R.build_pools(key)
    ids = np.arange(len(outfits)).repeat(4)
    moved = 0
    for max_len in (1, 5, 31):
        item, cu, tgt, _ = R.sample_batch(split, pools, ids, SEED, 9, 0, max_len)
        assert cu[0] == 0 and cu[-1] == len(item)
        for b, oid in enumerate(ids):
            o, got = outfits[oid], item[cu[b]:cu[b + 1]].tolist()
            rest = list(o); rest.remove(tgt[b])
            assert len(got) == min(len(o) - 1, max_len) and len(set(got)) == len(got) and set(got) <= set(rest), (b, max_len)
            moved += got != rest[:len(got)]
    assert moved > len(ids)                                              # it is a shuffle, not the file order


def test_the_same_seed_and_draw_repeat_and_any_other_argument_changes_the_batch():
    key, outfits, pos = make_world(4)
    split, pools = R.build_split(outfits, pos), R.build_pools(key)
    ids = np.zeros(64, np.int64) + 5                                    # one outfit in every slot: the slots draw on their own
    a = R.sample_batch(split, pools, ids, SEED, 11, 10, 16)
    again = R.sample_batch(split, pools, ids, SEED, 11, 10, 16)
    assert all(np.array_equal(x, y) for x, y in zip(a, again))
    for other in (R.sample_batch(split, pools, ids, SEED, 12, 10, 16), R.sample_batch(split, pools, ids, SEED + 1, 11, 10, 16)):
        assert not np.array_equal(a[3], other[3]) and not np.array_equal(a[0], other[0])
    assert len({tuple(r) for r in a[3].tolist()}) > 32                   # the slots of one outfit differ


def _one_outfit_world(m, n_items=5, n_pos=None):
    """Table rows 0 .. m - 1 form one pool, the outfit is rows 0 .. n_items - 1."""
    split = R.build_split([list(range(n_items))], None if n_pos is None else [list(range(n_pos))])
    return split, R.build_pools(np.zeros(max(m, n_items), np.int64))


@pytest.mark.parametrize("others,K", [(11, 10), (12, 10), (13, 3), (100, 10)])
def test_every_pool_element_is_a_negative_equally_often(others, K):
    """m - 1 = `others` candidates, K drawn: each is included with probability K / others.  The target is fixed (one eligible position) so
    that the candidates are the same rows for every query."""
    split, pools = _one_outfit_world(others + 1, n_pos=1)
    neg = R.sample_batch(split, pools, np.zeros(B_STAT, np.int64), SEED, 0, K, 16)[3]
    assert (np.sort(neg, axis=1)[:, 1:] != np.sort(neg, axis=1)[:, :-1]).all()
    count = np.bincount(neg.ravel(), minlength=others + 1)
    assert count[0] == 0                                                 # row 0 is the target
    p = K / others
    dev = np.abs(count[1:] - B_STAT * p).max() / np.sqrt(B_STAT * p * (1 - p))
    print(f"inclusion ({others}, {K}): {dev:.2f} sigma")
    assert dev < SIGMA, dev


def test_the_orders_of_a_four_item_remainder_are_equally_likely():
    split, pools = _one_outfit_world(8, n_items=5, n_pos=1)             # the positive is position 0, rows 1 .. 4 remain
    item, cu, _, _ = R.sample_batch(split, pools, np.zeros(B_STAT, np.int64), SEED, 0, 0, 16)
    orders = item.reshape(B_STAT, 4)
    code = (orders * np.array([125, 25, 5, 1])).sum(1)
    want = sorted(sum(v * w for v, w in zip(p, (125, 25, 5, 1))) for p in itertools.permutations((1, 2, 3, 4)))
    values, count = np.unique(code, return_counts=True)
    assert values.tolist() == want
    dev = np.abs(count - B_STAT / 24).max() / np.sqrt(B_STAT * (1 / 24) * (23 / 24))
    print(f"24 orders: {dev:.2f} sigma")
    assert dev < SIGMA, dev


def test_the_positive_is_uniform_over_the_eligible_positions():
    split, pools = R.build_split([[10, 11, 12, 13, 14]], [[0, 2, 3]]), R.build_pools(np.zeros(20, np.int64))
    tgt = R.sample_batch(split, pools, np.zeros(B_STAT, np.int64), SEED, 0, 0, 16)[2]
    values, count = np.unique(tgt, return_counts=True)
    assert values.tolist() == [10, 12, 13]
    dev = np.abs(count - B_STAT / 3).max() / np.sqrt(B_STAT * (1 / 3) * (2 / 3))
    print(f"positive among 3: {dev:.2f} sigma")
    assert dev < SIGMA, dev


# ------------------------------------------------------------------------------------------------ outfitx_amd/sampler.py, host side
def test_pool_tables_equal_a_dict_built_the_references_way():
    from outfitx_amd.sampler import CIRNegativePools
    key, _, _ = make_world(6, n_table=1000, n_keys=13)
    pools = CIRNegativePools(key, device="cpu")
    want = R.build_pools(key)
    for k in ("pool_cu", "pool_rows", "row_pool", "row_slot"):
        got = getattr(pools, k)
        assert got.dtype == np.int32 and np.array_equal(got, want[k]), k
        assert pools.dev[k].dtype.is_floating_point is False and np.array_equal(pools.dev[k].numpy()[:len(got)], got)
    negative_pool = {}
    for r, k in enumerate(key.tolist()):                                # polyvore_complementary_item_retrieval_dataset.py:94-99
        negative_pool.setdefault(k, []).append(r)
    for r in range(len(key)):
        if key[r] < 0:
            assert pools.row_pool[r] == -1
            continue
        g = pools.row_pool[r]
        members = pools.pool_rows[pools.pool_cu[g]:pools.pool_cu[g + 1]].tolist()
        assert members == negative_pool[key[r]] and members[pools.row_slot[r]] == r and pools.keys[g] == key[r]
    assert (pools.n_table, pools.n_pools, pools.n_pool_rows) == (1000, len(set(key[key >= 0].tolist())), int((key >= 0).sum()))
    empty = CIRNegativePools(np.full(5, -1), device="cpu")              # no pool at all: every array still has an address
    assert empty.n_pools == 0 and empty.pool_cu.tolist() == [0] and empty.dev["pool_rows"].numel() == 1
    for bad in ([], [[1, 2]], [0.5, 1.0]):
        with pytest.raises(ValueError):
            CIRNegativePools(np.asarray(bad), device="cpu")


def test_dataset_tables_and_every_refusal():
    from outfitx_amd import _lib as L
    from outfitx_amd.sampler import CIRDeviceDataset, CIRNegativePools
    key, outfits, pos = make_world(7)
    pools = CIRNegativePools(key, device="cpu")
    for p in (pos, None):
        ds = CIRDeviceDataset(outfits, pools, p)
        want = R.build_split(outfits, p)
        assert all(ds.host[k].dtype == np.int32 and np.array_equal(ds.host[k], want[k]) for k in want), p is None
        assert len(ds) == len(outfits) and (ds.max_length, ds.negatives, ds.seed) == (16, 10, 0)
    assert (ds.steps_per_epoch(16), ds.steps_per_epoch(16, drop_last=True), ds.steps_per_epoch(16, world=2)) == (4, 3, 2)
    ok = [[0, 1, 2], [3, 4]]
    refused = [dict(outfits=[[0, 1, 2], [3]]), dict(outfits=[list(range(65)), [3, 4]]), dict(outfits=[[0, 1, len(key)], [3, 4]]),
               dict(outfits=[[0, -1, 2], [3, 4]]), dict(outfits=ok, positive_idx_lists=[[0, 3], [0]]), dict(outfits=ok, positive_idx_lists=[[-1], [0]]),
               dict(outfits=ok, positive_idx_lists=[[0], []]), dict(outfits=ok, positive_idx_lists=[[0]]), dict(outfits=[]),
               dict(outfits=ok, max_length=32), dict(outfits=ok, max_length=0), dict(outfits=ok, negatives=65), dict(outfits=ok, negatives=-1)]
    for kw in refused:
        with pytest.raises(ValueError):
            CIRDeviceDataset(pools=pools, **kw)
    ds = CIRDeviceDataset([list(range(64)), [3, 4]], pools, [[63], [1]], max_length=31, negatives=64)      # the limits themselves are taken
    with pytest.raises(ValueError):
        ds.set_pools(CIRNegativePools(key[:-1], device="cpu"))                                              # another table
    hard = CIRNegativePools(np.where(key >= 0, key // 2, key), device="cpu")
    ds.set_pools(hard)
    assert ds.pools is hard
    # the draw is a kernel: a dataset on the host refuses to make batches instead of sampling some other way
    import torch
    with pytest.raises(L.OfxError):
        ds.batch(torch.zeros(2, dtype=torch.int32), 0)
