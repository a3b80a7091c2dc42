#!/usr/bin/env python
"""One FITB test batch fed three ways on one MI355X ("Fill-in-the-blank from the table"):

  (a) dense from host memory: the reference collate's padded fp32 batch (outfit [B,16,1024], text [B,512], candidates [B,4,1024]),
      scored by engine.fitb_argmin - the path of the commit before the indexed entry;
      (a2) the half-indexed collate of that commit: the outfit as table rows, candidates and text still dense;
  (b) index form from host memory: int32 rows only, scored by engine.fitb_argmin_indexed straight from the table;
  (c) sampler.FITBDeviceSplit: the same indices, uploaded once; a batch is a set of device views.

Workload (seeded, the cfg3 shape): 1024 questions of 8 context items, 4 candidates, D = 1024, a table of --table-rows rows.  Host tensors
are pinned (the reference's DataLoader pins).  Reported per form: the whole batch through trainer.FITBEvaluator.test_epoch (copy, forward,
scoring, the one read of the counter; host clock around a call that ends in a synchronisation) and the bytes it copies to the device; and
the scoring call alone on resident data, dense against indexed: the C entries on preallocated outputs and the engine wrappers (device
events around --inner calls).  All forms give the same indices
(asserted).  The forms alternate; --rounds rounds of --reps timings each after a warm-up, one process: the figure is the median of all
timings, `round_medians` shows how far repeated medians of the same thing lie apart - a difference inside that spread is not one.
Writes profiles/fitb_eval_bench.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")
from outfitx_amd import synth  # noqa: E402
from outfitx_amd.engine import fitb_argmin, fitb_argmin_indexed  # noqa: E402
from outfitx_amd.sampler import FITBDeviceSplit  # noqa: E402
from outfitx_amd.trainer import FITBEvaluator  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=1024)
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=4)
    ap.add_argument("--table-rows", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="scoring calls per device-event timing")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fitb_eval_bench.json"))
    a = ap.parse_args()
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    B, n_it, C, NT, D, L = a.questions, a.items, a.candidates, a.table_rows, 1024, 16
    dev = torch.device("cuda", 0)
    model = OutfitX(OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip")))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.outfit_transformer_weights(7).items()}, strict=False)
    model = model.to(dev).eval()
    g = np.random.default_rng(a.seed)
    table = synth.item_embeddings(a.seed, "table", NT)
    model.set_embedding_table(torch.from_numpy(table))
    rows = g.integers(0, NT, B * n_it).astype(np.int32)
    cu_items = (np.arange(B + 1) * n_it).astype(np.int32)
    cand = g.integers(0, NT, (B, C)).astype(np.int32)
    ans = g.integers(0, C, B).astype(np.int64)
    target = cand[np.arange(B), ans].astype(np.int32)
    emb = np.zeros((B, L, D), np.float32); mask = np.ones((B, L), bool)
    emb[:, :n_it] = table[rows].reshape(B, n_it, D); mask[:, :n_it] = False
    pin = lambda x: torch.from_numpy(np.ascontiguousarray(x)).pin_memory()
    txt, cand_emb = pin(table[target, D // 2:]), pin(table[cand])
    batches = {
        "a_dense_host": {"input_dict": {"task": CIR, "outfit_embedding": pin(emb), "outfit_mask": pin(mask), "target_item_text_embedding": txt},
                         "candidate_item_embedding": cand_emb, "answer_index": pin(ans)},
        "a2_half_indexed_host": {"input_dict": {"task": CIR, "item_index": pin(rows), "cu_seqlens": pin(cu_items), "target_item_text_embedding": txt},
                                 "candidate_item_embedding": cand_emb, "answer_index": pin(ans)},
        "b_index_host": {"input_dict": {"task": CIR, "item_index": pin(rows), "cu_seqlens": pin(cu_items), "target_item_index": pin(target)},
                         "candidate_item_index": pin(cand), "answer_index": pin(ans)},
    }
    split = FITBDeviceSplit(rows, cu_items, cand, ans, device=dev, n_table=NT)
    batches["c_device_split"] = next(iter(split.batches(B)))
    h2d = {k: int(sum(t.numel() * t.element_size() for t in list(b["input_dict"].values())[1:] + [v for n, v in b.items() if n != "input_dict"]
                      if not t.is_cuda)) for k, b in batches.items()}
    ev = FITBEvaluator(model)

    # every form scores the same rows: the same indices, hence the same accuracy
    with torch.no_grad():
        y = model(**{k: (v if k == "task" else v.to(dev)) for k, v in batches["b_index_host"]["input_dict"].items()})
        cand_d, ci_d, ans_d = cand_emb.to(dev), torch.from_numpy(cand).to(dev), torch.from_numpy(ans).to(dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        i_dense, d_dense = fitb_argmin(y, cand_d, return_dist=True)
        i_index, d_index = fitb_argmin_indexed(model.embedding_table, ci_d, y, answer=ans_d, n_correct=counter, return_dist=True)
        assert torch.equal(i_dense, i_index) and torch.equal(d_dense.view(torch.int32), d_index.view(torch.int32)), "dense and indexed scoring disagree"
        assert int(counter) == int((i_dense == ans_d).sum())
    acc = {k: ev.test_epoch([b])["Accuracy"] for k, b in batches.items()}
    assert len(set(acc.values())) == 1 and acc["a_dense_host"] == int(counter) / B, acc

    def whole(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.test_epoch([batches[name]])                 # ends in the read of the counter: a synchronisation
        return (time.perf_counter() - t0) * 1e3

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        counter.zero_()                                 # the counting entries add into it on every call: it starts every timing at 0
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner * 1e3     # microseconds per call

    # the C entries themselves on preallocated outputs (ctypes, a few microseconds of host time per call: the device is the bound), and the
    # engine wrappers, whose Python work per call (checks, output allocation) can exceed the kernel's time: then the host is the bound
    from outfitx_amd import _lib
    lib, st = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    tab, ci32 = model.embedding_table, ci_d.contiguous()
    idx_o = torch.empty(B, dtype=torch.int64, device=dev)
    p = lambda t: t.data_ptr()
    scoring = {"dense": lambda: lib.ofx_fitb_argmin(p(y), p(cand_d), B, C, D, p(idx_o), None, st),
               "indexed": lambda: lib.ofx_fitb_argmin_indexed(p(tab), tab.stride(0), NT, p(ci32), p(y), B, C, D, None, p(idx_o), None, None, st),
               "indexed_counting": lambda: lib.ofx_fitb_argmin_indexed(p(tab), tab.stride(0), NT, p(ci32), p(y), B, C, D, p(ans_d), p(idx_o), None,
                                                                       p(counter), st),
               "engine_dense": lambda: fitb_argmin(y, cand_d), "engine_indexed": lambda: fitb_argmin_indexed(tab, ci_d, y),
               "engine_indexed_counting": lambda: fitb_argmin_indexed(tab, ci_d, y, answer=ans_d, n_correct=counter)}
    assert scoring["dense"]() == 0 and scoring["indexed"]() == 0 and scoring["indexed_counting"]() == 0
    torch.cuda.synchronize()
    assert torch.equal(idx_o, i_dense)
    with torch.no_grad():
        for _ in range(a.warmup):
            for k in batches:
                whole(k)
            for fn in scoring.values():
                events(fn)
        t_whole = {k: [[] for _ in range(a.rounds)] for k in batches}
        t_score = {k: [[] for _ in range(a.rounds)] for k in scoring}
        for r in range(a.rounds):
            for _ in range(a.reps):
                for k in batches:
                    t_whole[k][r].append(whole(k))
                for k, fn in scoring.items():
                    t_score[k][r].append(events(fn))

    def summary(rounds):
        flat = [t for r in rounds for t in r]
        return {"median": statistics.median(flat), "round_medians": [statistics.median(r) for r in rounds], "min_max": [min(flat), max(flat)]}
    out = {"workload": f"{B} questions x {n_it} context items (padded to {L} in the dense form), {C} candidates, D={D}, table of {NT} rows",
           "seed": a.seed, "reps": a.reps, "rounds": a.rounds, "scoring_calls_per_timing": a.inner,
           "whole_batch_ms": {k: summary(v) for k, v in t_whole.items()}, "h2d_bytes_per_batch": h2d,
           "scoring_call_us": {k: summary(v) for k, v in t_score.items()},
           "scoring_bytes_read": {"dense": B * (C + 1) * D * 4, "indexed": B * (C + 1) * D * 4 + B * C * 4},
           "accuracy": acc["a_dense_host"], "indices_equal": True, "distance_bits_equal": True, "device": torch.cuda.get_device_name(0)}
    sd, si = out["scoring_call_us"]["dense"], out["scoring_call_us"]["indexed"]
    spread = max(max(s["round_medians"]) - min(s["round_medians"]) for s in (sd, si))
    out["indexed_minus_dense_us"] = si["median"] - sd["median"]
    out["spread_between_round_medians_us"] = spread
    out["indexed_slower_than_the_spread"] = bool(si["median"] - sd["median"] > spread)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
