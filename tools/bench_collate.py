#!/usr/bin/env python3
"""N3 measurement: batch hand-over to the CP forward, padded tensors vs indices into a device-resident table.

  padded : processor pads fp32 [B,16,1024] on the host (outfitx_amd.processor, the reference's collate output) ->
           pinned H2D copy -> forward
  indexed: OutfitXIndexedProcessor emits int32 indices + offsets -> H2D of a few KB -> forward gathers rows in HBM

    python tools/bench_collate.py [--batch 3072] [--items 8]

--task cir: the CIR training batch (complementary_item_retrieval_processor.py; the reference's per-GPU batch 3072 with --negatives 10,
10 % of the lists one short), HOST ONLY - no GPU is touched: collate time and batch bytes of the reference-shaped dense collate against
OutfitXIndexedProcessor(CIR, run_mode='train'), whose samples carry negative item ids instead of embeddings.

    python tools/bench_collate.py --task cir [--batch 3072] [--items 8] [--negatives 10] [--out profiles/cir_indexed_collate_bench.json]
"""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outfitx_amd import synth
from outfitx_amd.embedding_store import EmbeddingTable


def batch_bytes(batch):
    ts = [v for t in batch.values() for v in (t.values() if isinstance(t, dict) else [t]) if isinstance(v, torch.Tensor)]
    return int(sum(v.numel() * v.element_size() for v in ts))


def cir_main(a):
    """Host-only: dense against indexed CIR collate."""
    from outfitx_amd.configs import ItemEncoderConfig, OutfitXConfig
    from outfitx_amd.datatypes import FashionItem, OutfitComplementaryItemRetrievalTask as CIR
    from outfitx_amd.processor import OutfitXIndexedProcessor, OutfitXProcessorFactory
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    g = np.random.default_rng(0)
    emb = synth.item_embeddings(5, "table", a.table)
    table = EmbeddingTable(np.arange(a.table), emb)
    n = g.integers(max(1, a.items - 4), a.items + 5, a.batch).clip(1, 16)
    item = lambda i: FashionItem(item_id=int(i), embedding=emb[i], text_embedding=emb[i, 512:])
    dense_batch, index_batch = [], []
    for k in n:
        ids, tgt = g.integers(0, a.table, k), int(g.integers(0, a.table))
        negs = [int(j) for j in g.integers(0, a.table, a.negatives - (g.random() < 0.1))]
        dense_batch.append((CIR(outfit=[item(i) for i in ids], target_item=item(tgt)), [emb[j] for j in negs]))
        index_batch.append((CIR(outfit=[FashionItem(item_id=int(i)) for i in ids], target_item=FashionItem(item_id=tgt)), negs))
    pd = OutfitXProcessorFactory.get_processor(CIR, cfg, run_mode="train")
    pi = OutfitXIndexedProcessor(CIR, cfg, id_to_row=table.index(), run_mode="train")

    def t(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); out = fn(); ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(min(ts)), float(max(ts)), out

    res = {"task": "cir", "batch": a.batch, "negatives": a.negatives, "mean_items": float(n.mean()), "reps": a.reps, "cpus": os.cpu_count()}
    for name, fn in (("dense", lambda: pd(dense_batch)), ("indexed", lambda: pi(index_batch))):
        res[f"ms_collate_{name}"], res[f"ms_collate_{name}_min"], res[f"ms_collate_{name}_max"], out = t(fn)
        res[f"batch_bytes_{name}"] = batch_bytes(out)
    res["collate_dense_over_indexed"] = res["ms_collate_dense"] / res["ms_collate_indexed"]
    line = json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=["cp", "cir"], default="cp")
    ap.add_argument("--negatives", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the JSON line to this file (CIR task)")
    ap.add_argument("--batch", type=int, default=3072)      # the reference's CP batch size (base_train_config.py)
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--table", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if a.task == "cir":
        return cir_main(a)
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    from src.models.datatypes import FashionItem, OutfitCompatibilityPredictionTask as CP
    from src.models.processor import OutfitXProcessorFactory
    from outfitx_amd.processor import OutfitXIndexedProcessor
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    m = OutfitX(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.outfit_transformer_weights(7).items()}, strict=False)
    m = m.cuda().eval()
    g = np.random.default_rng(0)
    emb = synth.item_embeddings(5, "table", a.table)
    table = EmbeddingTable(np.arange(a.table), emb)
    m.set_embedding_table(torch.from_numpy(emb))
    n = g.integers(max(1, a.items - 4), a.items + 5, a.batch).clip(1, 16)
    ids = [g.integers(0, a.table, k) for k in n]
    dense_batch = [(CP(outfit=[FashionItem(item_id=int(i), embedding=emb[i]) for i in r]), 0.0) for r in ids]
    index_batch = [(CP(outfit=[FashionItem(item_id=int(i)) for i in r]), 0.0) for r in ids]
    pd = OutfitXProcessorFactory.get_processor(CP, cfg)
    pi = OutfitXIndexedProcessor(CP, cfg, id_to_row=table.index())

    def t(fn):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps): out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3, out

    res = {"batch": a.batch, "mean_items": float(n.mean())}
    res["ms_collate_padded"], bd = t(lambda: pd(dense_batch))
    res["ms_collate_indexed"], bi = t(lambda: pi(index_batch))
    e, k = bd["input_dict"]["outfit_embedding"].pin_memory(), bd["input_dict"]["outfit_mask"].pin_memory()
    res["h2d_bytes_padded"] = e.numel() * 4 + k.numel()
    res["h2d_bytes_indexed"] = bi["input_dict"]["item_index"].numel() * 4 + bi["input_dict"]["cu_seqlens"].numel() * 4
    with torch.no_grad():
        res["ms_h2d_forward_padded"], ya = t(lambda: m(task=CP, outfit_embedding=e.cuda(non_blocking=True), outfit_mask=k.cuda(non_blocking=True)))
        ii, cc = bi["input_dict"]["item_index"].pin_memory(), bi["input_dict"]["cu_seqlens"].pin_memory()
        res["ms_h2d_forward_indexed"], yb = t(lambda: m(task=CP, item_index=ii, cu_seqlens=cc))
        ed, kd = e.cuda(), k.cuda()
        res["ms_forward_resident_padded"], _ = t(lambda: m(task=CP, outfit_embedding=ed, outfit_mask=kd))
    res["identical"] = bool(torch.equal(ya, yb))
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
