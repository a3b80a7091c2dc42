"""Exact host reference of the category-pool retrieval (Engine.l2_topk_grouped / ofx_l2_topk_grouped): per group
oracle.np_oracle.l2_topk_exact of the group's queries against the group's pool, meant for oracle.np_oracle.lattice inputs (every d2 an
exact integer, so selection and order are defined on every position), plus what the grouped call adds: the -1 / +inf tail of a pool
smaller than k, the position of the ground-truth row, and the recall counts.  tests/test_cpu_grouped_topk.py pins it to the
reference's own formulation (complementary_item_retrieval_trainer.py:192-249: padded cdist -> topk -> masked hit ratio)."""
import numpy as np

from oracle import np_oracle as O


def f32_sqrt(d2):
    """float32(sqrt(float64 d2)): the correctly rounded fp32 root of an exact d2 (+inf stays +inf)."""
    return np.sqrt(np.asarray(d2, np.float64)).astype(np.float32)


def grouped_topk_ref(Q, group_of_query, P, pool_offsets, k, gt=None):
    """Q [nq, D] in any order, group_of_query [nq], P [np, D] = all pools concatenated, pool_offsets [G + 1], gt [nq] rows of P (< 0: none).
    -> (idx int64 [nq, k] rows of P, ascending by exact d2, ties -> smaller row, -1 behind a pool of fewer than k rows;
        d2 float64 [nq, k], +inf there;
        gt_pos int64 [nq]: the j with idx[q, j] == gt[q], k when there is none, -1 when gt[q] < 0; None without gt)."""
    Q, P = np.asarray(Q), np.asarray(P)
    grp, off = np.asarray(group_of_query, np.int64), np.asarray(pool_offsets, np.int64)
    nq = len(Q)
    idx = np.full((nq, k), -1, np.int64)
    d2 = np.full((nq, k), np.inf, np.float64)
    for g in np.unique(grp):
        sel = np.flatnonzero(grp == g)
        lo, hi = int(off[g]), int(off[g + 1])
        kk = min(k, hi - lo)
        idx[sel, :kk], d2[sel, :kk] = O.l2_topk_exact(Q[sel], P[lo:hi], kk, index_base=lo)
    if gt is None:
        return idx, d2, None
    gt = np.asarray(gt, np.int64)
    hit = idx == gt[:, None]
    gt_pos = np.where(hit.any(1), hit.argmax(1), k)
    return idx, d2, np.where(gt < 0, -1, gt_pos).astype(np.int64)


def recall_counts(gt_pos, top_k_list):
    """-> ([hits at K for K in top_k_list], number of queries with a ground truth): integers, the form that sums over ranks."""
    gt_pos = np.asarray(gt_pos)
    valid = gt_pos >= 0
    return [int((valid & (gt_pos < K)).sum()) for K in top_k_list], int(valid.sum())


def recall_ref(gt_pos, top_k_list):
    hits, n = recall_counts(gt_pos, top_k_list)
    return {f"Recall@{K}": (h / n if n else 0.0) for K, h in zip(top_k_list, hits)}
