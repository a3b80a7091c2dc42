"""numpy restatement of ofx_cir_sample_batch (include/ofx.h, outfitx_amd/csrc/cir_sample.hip): the specification the kernel is held to,
bit for bit, by tests/test_gpu_cir_sampler.py, and the object whose statistics tests/test_cpu_cir_sampler.py checks.

It is written the other way round from the kernel - whole-batch array expressions, an argsort where the kernel ranks, a loop over the
Floyd steps where the kernel ballots - and shares nothing with it but the definition of the draw: ofx_draw_u32 / ofx_draw_below of
outfitx_amd/csrc/ofx_common.h, restated here as `u32` and `below`."""
import numpy as np

U32 = np.uint32
MASK = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x).astype(np.uint64) & MASK


def fmix32(h):
    """murmur3's 32-bit finaliser on uint64 arrays holding 32-bit values."""
    h = _u(h)
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85EBCA6B)) & MASK
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & MASK
    h ^= h >> np.uint64(16)
    return h


def u32(seed, draw, stream, b, i):
    """Word i of stream `stream` (0 positive, 1 shuffle keys, 2 negatives) of batch slot b; b and i broadcast.  -> uint64 array < 2^32."""
    h = fmix32((_u(seed) + np.uint64(0x6A09E667)) & MASK)
    h = fmix32(h ^ _u(draw))
    h = fmix32((h + _u(stream) * np.uint64(0x9E3779B9) + np.uint64(0x7F4A7C15)) & MASK)
    h = fmix32(h ^ ((_u(b) * np.uint64(0x632BE5AB)) & MASK))
    return fmix32((h + _u(i) * np.uint64(0x9E3779B1)) & MASK)


def below(u, n):
    """A word -> an integer of [0, n): (u * n) >> 32."""
    return ((_u(u) * _u(n)) >> np.uint64(32)).astype(np.int64)


def build_pools(row_key):
    """One integer key per table row (negative = in no pool) -> pool_cu [G + 1], pool_rows, row_pool [n], row_slot [n] (int32): the pools
    in ascending key order, each holding its rows in table order - written as plain loops over a dict, the reference's way
    (polyvore_complementary_item_retrieval_dataset.py:94-99)."""
    pools = {}
    for r, k in enumerate(np.asarray(row_key).tolist()):
        if k >= 0:
            pools.setdefault(k, []).append(r)
    n = len(row_key)
    pool_cu, pool_rows = [0], []
    row_pool, row_slot = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for g, k in enumerate(sorted(pools)):
        for s, r in enumerate(pools[k]):
            row_pool[r], row_slot[r] = g, s
        pool_rows += pools[k]
        pool_cu.append(len(pool_rows))
    return {"pool_cu": np.asarray(pool_cu, np.int32), "pool_rows": np.asarray(pool_rows, np.int32).reshape(-1), "row_pool": row_pool, "row_slot": row_slot}


def build_split(outfits, positive_idx_lists=None):
    """Lists of table rows (and of eligible positions; None = every position) -> outfit_cu, outfit_rows, pos_cu, pos_slots (int32)."""
    if positive_idx_lists is None:
        positive_idx_lists = [list(range(len(o))) for o in outfits]
    cat = lambda ls: np.asarray([x for l in ls for x in l], np.int32).reshape(-1)
    cum = lambda ls: np.concatenate([[0], np.cumsum([len(l) for l in ls])]).astype(np.int32)
    return {"outfit_cu": cum(outfits), "outfit_rows": cat(outfits), "pos_cu": cum(positive_idx_lists), "pos_slots": cat(positive_idx_lists)}


def sample_batch(split, pools, outfit_ids, seed, draw, K, max_len):
    """-> (item_index [cu_seqlens[B]] - the compact part the kernel writes -, cu_seqlens [B + 1], target_item_index [B],
    neg_items_index [B, K]), int32.  Valid tables only (what CIRDeviceDataset and CIRNegativePools build)."""
    ocu, orows = split["outfit_cu"].astype(np.int64), split["outfit_rows"].astype(np.int64)
    pcu, pslots = split["pos_cu"].astype(np.int64), split["pos_slots"].astype(np.int64)
    gcu, grows = pools["pool_cu"].astype(np.int64), pools["pool_rows"].astype(np.int64)
    o = np.asarray(outfit_ids, np.int64).reshape(-1)
    B = len(o)
    b = np.arange(B)
    lo, n = ocu[o], ocu[o + 1] - ocu[o]
    # the positive
    P = pcu[o + 1] - pcu[o]
    p = pslots[pcu[o] + below(u32(seed, draw, 0, b, 0), P)]
    t = orows[lo + p]
    # the remainder: the other n - 1 items in file order, keyed, ordered by (key, j), truncated
    J = max(int(n.max()) - 1, 1)
    j = np.arange(J)[None, :]
    live = j < (n - 1)[:, None]
    src = np.minimum(lo[:, None] + j + (j >= p[:, None]), len(orows) - 1)
    keys = (u32(seed, draw, 1, b[:, None], j) << np.uint64(8)) | j.astype(np.uint64)           # (key, j) in one word: j < 64
    keys = np.where(live, keys, np.uint64(2 ** 63))
    order = np.argsort(keys, axis=1, kind="stable")
    shuffled = np.take_along_axis(orows[src], order, axis=1)
    length = np.minimum(n - 1, max_len)
    item_index = shuffled[np.arange(J)[None, :] < length[:, None]]                               # row-major: query after query
    cu_seqlens = np.concatenate([[0], np.cumsum(length)])
    # the negatives
    neg = np.full((B, K), -1, np.int64)
    if K:
        g = pools["row_pool"].astype(np.int64)[t]
        inpool = g >= 0
        gs = np.maximum(g, 0)
        m = np.where(inpool, gcu[gs + 1] - gcu[gs], 0)
        s_t = pools["row_slot"].astype(np.int64)[t]
        m1 = m - 1
        floyd = m1 >= K
        chosen = np.full((B, K), -1, np.int64)
        for s in range(K):
            jj = m1 - K + s
            v = below(u32(seed, draw, 2, b, s), np.maximum(jj + 1, 1))
            taken = (chosen[:, :s] == v[:, None]).any(axis=1)
            chosen[:, s] = np.where(taken, jj, v)
        k = np.arange(K)[None, :]
        short = np.where(k < m1[:, None], k, -1)                                                 # all the others in pool order, then -1
        c = np.where(floyd[:, None], chosen, short)
        slot = c + (c >= s_t[:, None])
        rows = grows[np.clip(gcu[gs][:, None] + slot, 0, max(len(grows) - 1, 0))] if len(grows) else np.zeros_like(slot)
        neg = np.where(c >= 0, rows, -1)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    return i32(item_index), i32(cu_seqlens), i32(t), i32(neg)
