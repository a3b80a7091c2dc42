#!/usr/bin/env python
"""Category-pool CIR retrieval, timed two ways on one MI355X ("Category-pool retrieval"):

  (a) Engine.l2_topk_grouped: every query against the pool of its own category, all categories in one call;
  (b) what the flat call offers: the queries grouped on the host, one Engine.l2_topk per non-empty category, results stitched.

Workload (seeded): 32 categories x 3000 rows, D = 1024, 4096 queries, k = 50; the categories of the queries follow a Zipf-like law
(weight 1 / rank, permuted), so a few categories get hundreds of queries and many get a handful.  Both forms give the same indices
(asserted).  The two forms alternate; medians of --reps device-event timings each after a warm-up, one process.  Host work that a
caller has to do per call (sorting by category, slicing, stitching, the panel table and its copy) is inside both timings.
Writes profiles/grouped_topk_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from outfitx_amd import synth  # noqa: E402
from outfitx_amd.engine import Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_topk_bench.json"))
    a = ap.parse_args()
    G, R, NQ, k, D = a.groups, a.rows, a.queries, a.k, 1024
    dev = torch.device("cuda", 0)
    eng = Engine(dev)
    g = np.random.default_rng(a.seed)
    w = 1.0 / np.arange(1, G + 1)
    grp = g.choice(G, size=NQ, p=g.permutation(w / w.sum()))
    counts = np.bincount(grp, minlength=G)
    off = np.arange(G + 1) * R
    P = torch.from_numpy(synth.item_embeddings(a.seed, "pool", G * R)).to(dev)
    Q = torch.from_numpy((synth.item_embeddings(a.seed, "queries", NQ) * 3.0).astype(np.float32)).to(dev)
    grp_t = torch.from_numpy(grp)

    def grouped():
        return eng.l2_topk_grouped(Q, grp_t, P, off, k)[:2]

    def per_group():
        order = torch.argsort(grp_t, stable=True)
        order_d = order.to(dev)
        Qs = Q.index_select(0, order_d)
        idx = torch.empty(NQ, k, dtype=torch.int64, device=dev)
        dist = torch.empty(NQ, k, dtype=torch.float32, device=dev)
        s = 0
        for c in range(G):
            n = int(counts[c])
            if n:
                i, d = eng.l2_topk(Qs[s:s + n], P[off[c]:off[c + 1]], k, index_base=int(off[c]))
                idx[order_d[s:s + n]] = i
                dist[order_d[s:s + n]] = d
                s += n
        return idx, dist

    ia, da = grouped()
    ib, db = per_group()
    torch.cuda.synchronize()
    assert torch.equal(ia, ib), "the two forms disagree on the indices"
    assert torch.equal(da.view(torch.int32), db.view(torch.int32)), "the two forms disagree on the distance bits"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        grouped(); per_group()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(a.reps):
        ta.append(timed(grouped))
        tb.append(timed(per_group))
    flops = 2.0 * D * float((counts * R).sum())
    ma, mb = statistics.median(ta), statistics.median(tb)
    out = {"workload": f"{G} categories x {R} rows, D={D}, {NQ} queries (Zipf-like over the categories), k={k}", "seed": a.seed, "reps": a.reps,
           "queries_per_category_min_median_max": [int(counts.min()), float(np.median(counts)), int(counts.max())],
           "non_empty_categories": int((counts > 0).sum()), "useful_flops": flops,
           "ms_grouped_median": ma, "ms_per_group_median": mb, "ms_grouped_min_max": [min(ta), max(ta)], "ms_per_group_min_max": [min(tb), max(tb)],
           "per_group_over_grouped": mb / ma, "tflops_grouped": flops / ma / 1e9, "tflops_per_group": flops / mb / 1e9,
           "indices_equal": True, "distance_bits_equal": True, "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
