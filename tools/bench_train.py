#!/usr/bin/env python3
"""BASELINE config 5 on one GPU: the CP trainer step on precomputed embeddings (cp_trainer:57-81) —
forward -> FocalLoss(.75, 2) -> backward -> clip_grad_norm_(1.0) -> AdamW step — through src.models.OutfitX in train() mode
(HIP tape forward + hand-written backward).  Per-GPU batch 256 (= 2048 / 8 ranks) by default.

    python tools/bench_train.py [--batch 256] [--items 8] [--steps 20] [--precision bf16] [--eager]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 tools/bench_train.py   (DP, RCCL)

ms_step is the reference-shaped step (torch clip_grad_norm_ + default AdamW on per-tensor grads); ms_step_dp is the
outfitx_amd.trainer.CPTrainer step (flat gradient arena, one all-reduce, fused AdamW), accumulation 1 = an optimizer step
and an all-reduce on EVERY micro-batch (the worst case; the reference default accumulates 4).

--task cir: the reference's other training job (complementary_item_retrieval_trainer.py:66-116, K = 10 negatives per query): the
outfitx_amd.trainer.CIRTrainer step at per-GPU batch 256 and 3072 (the reference config's batch), and SetWiseRankingLoss forward +
backward ALONE in the fused form (ofx_set_rank_loss) and in the eager torch form, alternating, medians over --loss-reps device-event
timings.  `loss_kernel_GBps` is (B K D 4 + 3 B D 4) bytes - neg read once, y / y_hat read, dy_hat written - over the two-launch call.

    python tools/bench_train.py --task cir [--cir-batches 256,3072] [--negatives 10] [--loss-reps 30]

It then times the INDEX form of the same batches (positives, negatives, target text and outfit rows named by row of a device-resident
table of --table rows; outfitx_amd/csrc/rank_loss.hip TableRows) against the dense batches GATHERED FROM THE SAME ROWS, alternating in one
process: the loss forward + backward through the class (`ms_loss_fwd_bwd_indexed_*` / `_dense_*`) and as raw engine calls
(`ms_loss_call_indexed_*` / `_dense_*`, with the dense call's own spread over its timings: `_dense_min/_p25/_p75/_max`), the CIRTrainer
step on device-resident batches (`ms_step_indexed_*` / `ms_step_dense_*`) and on batches handed over from pinned host memory on every step,
as a DataLoader does (`ms_step_hostfed_*`), and the bytes per batch of both forms, computed here (`batch_bytes_*`).  Those keys are also
written to --indexed-out (profiles/cir_indexed_bench.json).

Last, the batches DRAWN ON THE DEVICE (outfitx_amd/sampler.py, ofx_cir_sample_batch): --device-batch queries (3072) from outfits of
--items + 1 items over the --table rows in --pools negative pools.  `ms_batch_build_*` is the build of one batch alone (device events;
`_wall`: host and device, calls back to back); `ms_step_resident_*` / `ms_step_hostfed_*` / `ms_step_devicefed_*` are the CIRTrainer step on
one fixed device-resident index batch, on that batch handed over from pinned host memory on every step, and on a fresh batch drawn by
`CIRDeviceDataset.batch` before every step - --device-rounds rounds, the three alternating inside every round, medians over the rounds
with every round's value in `*_rounds_*`.  `devicefed_inside_resident_range_*` says whether the device-fed median lies between the
smallest and the largest resident round of this session.  `ms_host_collate_indexed_committed` repeats the host collate of one such batch
from profiles/cir_indexed_collate_bench.json (before the caller's own sampling).  --device-only runs this leg alone; --device-out writes its
line (profiles/cir_device_batches_bench.json).

The CP run also times the accumulation BOUNDARY alone at the CP arena's real size (51.3 M floats) in its two forms, alternating in
one process, medians over --boundary-reps device-event timings after a warm-up: `ms_boundary_torch` (vector_norm -> mul_ -> fused AdamW
over the per-tensor views -> zero_, plus the div_ by the world size when there is more than one rank) and `ms_boundary_hip`
(optim.FlatAdamW: one ofx_adamw_step call).  `boundary_bytes_*` are the bytes each form has to move, computed here from the arena's
length n: 44 n (52 n with the world divide) and 36 n; `boundary_GBps_*` the resulting rates; `us_boundary_hip_norm_pass` /
`us_boundary_hip_update_pass` the device times of the call's two kernels (torch.profiler, one step; absent if it records none).
`ms_step_dp_hip` / `ms_step_dp_accum4_hip` are the trainer steps with CPTrainConfig(hip_optimizer=True).  `ms_boundary_hip_scaled` is the
loss-scaled call (FlatAdamW(loss_scaling=True): ofx_adamw_step_scaled, on the same gradient x 65536) timed BETWEEN two groups of the plain
call, `ms_boundary_hip_plain_a` / `_plain_b`, the three alternating inside every repetition: the scaled call moves the same bytes, so the
distance between the two plain groups (`boundary_plain_spread`) is the margin `boundary_scaled_over_plain` is read against.  The line is
also written to --boundary-out when given (profiles/optimizer_step_bench.json).

--eager also times the same step written with plain torch modules (nn.TransformerEncoder under bf16 autocast, what the
reference's trainer executes) on the same GPU, for a like-for-like ratio.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outfitx_amd import synth  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def median_ms(fns, reps, warmup, prep=None):
    """Device-event time of each callable, the callables ALTERNATING inside every repetition -> list of medians (ms).  prep (optional)
    runs before every timed call, outside the timed span."""
    return [float(np.median(t)) for t in sample_ms(fns, reps, warmup, prep)]


def sample_ms(fns, reps, warmup, prep=None):
    """The timings behind median_ms: one list of `reps` device-event times (ms) per callable."""
    for _ in range(warmup):
        for fn in fns:
            if prep:
                prep()
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            if prep:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return ts


def boundary_bench(params, world, reps, res):
    """The accumulation boundary alone, torch's sequence against the one ofx_adamw_step call, on a freshly filled arena of the real size."""
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import FlatGrads
    grads = FlatGrads(params)
    flat, n = grads.flat, grads.flat.numel()
    opt_t = torch.optim.AdamW(grads.params, lr=2e-5, fused=True)
    opt_h = FlatAdamW(grads, lr=2e-5, max_norm=1.0)
    opt_h.grad_scale = 1.0 / world
    fill = torch.randn(n, device=flat.device) * 1e-3            # norm about 7: every timed boundary clips
    for o, p in zip(grads.offsets, grads.params):               # keep the padding zero, as the backward leaves it
        fill[o + p.numel():o + (p.numel() + 63) // 64 * 64] = 0

    def torch_form():
        if world > 1:
            flat.div_(world)
        grads.clip_norm_(1.0)
        opt_t.step()
        grads.zero_()

    t_t, t_h = median_ms([torch_form, opt_h.step], reps, 5, prep=lambda: flat.copy_(fill))
    b_t, b_h = (52 if world > 1 else 44) * n, 36 * n
    res.update(boundary_floats=n, boundary_reps=reps, ms_boundary_torch=t_t, ms_boundary_hip=t_h, boundary_bytes_torch=b_t, boundary_bytes_hip=b_h,
               boundary_GBps_torch=b_t / (t_t * 1e-3) / 1e9, boundary_GBps_hip=b_h / (t_h * 1e-3) / 1e9, boundary_torch_over_hip=t_t / t_h)
    try:                                                        # device time of each of the call's two kernels
        from torch.profiler import ProfilerActivity, profile
        flat.copy_(fill)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            opt_h.step()
            torch.cuda.synchronize()
        for e in prof.events():
            for key, name in (("adamw_norm_kernel", "us_boundary_hip_norm_pass"), ("adamw_update_kernel", "us_boundary_hip_update_pass")):
                if key in e.name:
                    res[name] = float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
    except Exception as e:                                      # noqa: BLE001 - the per-kernel split is a diagnostic; the medians above are the result
        res["boundary_profile_error"] = repr(e)[:200]
    # the loss-scaled call (ofx_adamw_step_scaled) between two groups of the plain call, all three alternating: the scaled call moves
    # the same bytes, so what separates the two plain groups from each other is the margin it is judged by
    opt_s = FlatAdamW(grads, lr=2e-5, max_norm=1.0, loss_scaling=True)
    opt_s.grad_scale = 1.0 / world
    fill_s = fill * opt_s.loss_scale                            # the arena a scaled backward leaves: the same gradient x 65536
    ts = [[] for _ in range(3)]
    for rep in range(5 + reps):
        for i, (opt, src) in enumerate(((opt_h, fill), (opt_s, fill_s), (opt_h, fill))):
            flat.copy_(src)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); opt.step(); b.record()
            b.synchronize()
            if rep >= 5:
                ts[i].append(a.elapsed_time(b))
    t_a, t_s, t_b = (float(np.median(t)) for t in ts)
    res.update(ms_boundary_hip_plain_a=t_a, ms_boundary_hip_scaled=t_s, ms_boundary_hip_plain_b=t_b, boundary_scaled_over_plain=t_s / min(t_a, t_b),
               boundary_plain_spread=abs(t_a - t_b) / min(t_a, t_b), boundary_scaled_skipped=int(opt_s.skipped),
               boundary_scaled_scale=float(opt_s.loss_scale))
    del opt_t, opt_h, opt_s, grads


def eager_set_rank_loss(batch_y, batch_y_hat, batch_negative_samples, batch_negative_mask, margin=2.0):
    """The torch expression of outfitx_amd.losses.SetWiseRankingLoss (its CPU / fallback path), whatever the tensors' device."""
    d_pos = torch.linalg.vector_norm(batch_y_hat - batch_y + 1e-6, dim=-1)
    d_neg = torch.linalg.vector_norm(batch_y_hat[:, None, :] - batch_negative_samples, dim=-1)
    valid = ~batch_negative_mask
    n_valid = valid.sum().clamp(min=1)
    hinge_all = torch.relu(d_pos[:, None] - d_neg + margin) * valid
    hardest = d_neg.masked_fill(batch_negative_mask, float("inf")).amin(dim=1)
    return hinge_all.sum() / n_valid + torch.relu(d_pos - hardest + margin).mean()


def cir_indexed_bench(a, m, params, B, K, res):
    """Index-form batches against the dense batches gathered from the same table rows (module docstring)."""
    from outfitx_amd.engine import set_rank_loss, set_rank_loss_indexed
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    from src.losses import SetWiseRankingLoss
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    D, L = 1024, a.pad
    g = np.random.default_rng(99)
    table = torch.from_numpy(synth.item_embeddings(99, "table", a.table) * 3.0)
    n_items = np.full(B, a.items)
    idx = torch.from_numpy(g.integers(0, a.table, int(n_items.sum())).astype(np.int32))
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(n_items)]).astype(np.int32))
    pos = torch.from_numpy(g.integers(0, a.table, B).astype(np.int32))
    neg = g.integers(0, a.table, (B, K)).astype(np.int32)
    neg[g.random((B, K)) < 0.1] = -1
    neg = torch.from_numpy(neg)
    emb = torch.zeros(B, L, D); mask = torch.ones(B, L, dtype=torch.bool)
    emb[:, :a.items] = table[idx.long()].view(B, a.items, D); mask[:, :a.items] = False
    host = {"indexed": {"input_dict": {"task": CIR, "item_index": idx, "cu_seqlens": cu, "target_item_index": pos.clone()},
                        "pos_item_index": pos, "neg_items_index": neg},
            "dense": {"input_dict": {"task": CIR, "outfit_embedding": emb, "outfit_mask": mask,
                                     "target_item_text_embedding": table[pos.long(), D // 2:].contiguous()},
                      "pos_item_embedding": table[pos.long()], "neg_items_embedding": table[neg.clamp(min=0).long()], "neg_items_mask": neg < 0}}
    move = lambda b, f: {k: ({n: (v if n == "task" else f(v)) for n, v in t.items()} if k == "input_dict" else f(t)) for k, t in b.items()}
    nbytes = lambda b: sum(v.numel() * v.element_size() for t in b.values() for v in (t.values() if isinstance(t, dict) else [t]) if isinstance(v, torch.Tensor))
    for form in host:
        res[f"batch_bytes_{form}_b{B}"] = int(nbytes(host[form]))
    pinned = {f: move(b, lambda v: v.pin_memory()) for f, b in host.items()}
    dev = {f: move(b, lambda v: v.cuda()) for f, b in host.items()}
    m.set_embedding_table(table)
    tab = m.embedding_table
    # ---- the loss alone: class forward + backward, and the raw two-launch calls
    y_hat0 = torch.from_numpy(synth.item_embeddings(99, "y_hat", B) * 3.0).cuda()
    di, dd = dev["indexed"], dev["dense"]
    fn = SetWiseRankingLoss(margin=2.0)

    def loss_indexed():
        yh = y_hat0.detach().requires_grad_(True)
        fn.forward_indexed(yh, tab, di["pos_item_index"], di["neg_items_index"]).backward()
        return yh.grad

    def loss_dense():
        yh = y_hat0.detach().requires_grad_(True)
        fn(batch_y=dd["pos_item_embedding"], batch_y_hat=yh, batch_negative_samples=dd["neg_items_embedding"], batch_negative_mask=dd["neg_items_mask"]).backward()
        return yh.grad

    res[f"loss_grad_indexed_equals_dense_b{B}"] = bool(torch.equal(loss_indexed(), loss_dense()))
    call_i = lambda: set_rank_loss_indexed(tab, di["pos_item_index"], di["neg_items_index"], y_hat0, 2.0)
    call_d = lambda: set_rank_loss(dd["pos_item_embedding"], y_hat0, dd["neg_items_embedding"], dd["neg_items_mask"], 2.0)
    ts = sample_ms([loss_indexed, loss_dense, call_i, call_d], a.loss_reps, 5)
    for name, t in zip(("loss_fwd_bwd_indexed", "loss_fwd_bwd_dense", "loss_call_indexed", "loss_call_dense"), ts):
        res[f"ms_{name}_b{B}"] = float(np.median(t))
        for tag, q in (("min", 0), ("p25", 25), ("p75", 75), ("max", 100)):
            res[f"ms_{name}_{tag}_b{B}"] = float(np.percentile(t, q))
    res[f"loss_call_indexed_over_dense_b{B}"] = res[f"ms_loss_call_indexed_b{B}"] / res[f"ms_loss_call_dense_b{B}"]
    # ---- the trainer step: device-resident batches, then batches that cross from pinned host memory on every step
    for where, forms in (("", dev), ("hostfed_", pinned)):
        for form in ("indexed", "dense"):
            tr = CIRTrainer(m, steps_per_epoch=10 ** 9, cfg=CIRTrainConfig(accumulation_steps=1), params=params)
            k = [0]
            def step():
                tr.micro_step(forms[form], k[0]); k[0] += 1
            res[f"ms_step_{where}{form}_b{B}"] = timed(step, a.steps, a.warmup)
            del tr
    del m.embedding_table


def cir_device_bench(a, m, params, B, K):
    """Batches drawn on the device (outfitx_amd.sampler, ofx_cir_sample_batch) feeding CIRTrainer (module docstring) -> the result dict."""
    from outfitx_amd.sampler import CIRDeviceDataset, CIRNegativePools
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    g = np.random.default_rng(99)
    n_outfits = max(4 * B, 16384)
    outfits = g.integers(0, a.table, (n_outfits, a.items + 1)).tolist()          # one item becomes the positive, a.items remain
    pools = CIRNegativePools(g.integers(0, a.pools, a.table))
    ds = CIRDeviceDataset(outfits, pools, None, max_length=a.pad, negatives=K, seed=99)
    m.set_embedding_table(torch.from_numpy(synth.item_embeddings(99, "table", a.table) * 3.0))
    res = {"workload": f"CIR batches of {B} drawn on the device from {n_outfits} outfits of {a.items + 1} items, a {a.table}-row table in {a.pools} pools, "
                       f"{K} negatives per query, feeding the CIRTrainer step", "precision": a.precision, "steps": a.steps, "rounds": a.device_rounds,
           "loss_reps": a.loss_reps}
    order = ds.order(0)
    ids = order[:B]
    k = [0]

    def build():
        k[0] += 1
        return ds.batch(ids, k[0])

    ts = sample_ms([build], a.loss_reps, 5)[0]                                  # device time of one batch build (two launches + four allocations)
    res[f"ms_batch_build_b{B}"] = float(np.median(ts))
    res[f"ms_batch_build_min_b{B}"], res[f"ms_batch_build_max_b{B}"] = float(np.min(ts)), float(np.max(ts))
    res[f"ms_batch_build_wall_b{B}"] = timed(build, a.steps, a.warmup)           # host + device, back to back
    one = ds.batch(ids, 0)
    total = int(one["input_dict"]["cu_seqlens"][-1])
    compact = lambda f: {"input_dict": {n: (v if n == "task" else f(v[:total] if n == "item_index" else v)) for n, v in one["input_dict"].items()},
                         "pos_item_index": f(one["pos_item_index"]), "neg_items_index": f(one["neg_items_index"])}
    resident, pinned = compact(lambda v: v.clone()), compact(lambda v: v.cpu().pin_memory())
    res[f"batch_bytes_b{B}"] = int(sum(v.numel() * 4 for v in (*[t for n, t in resident["input_dict"].items() if n != "task"], resident["neg_items_index"])))
    n_steps = ds.steps_per_epoch(B, drop_last=True)
    legs = {"resident": [], "hostfed": [], "devicefed": []}
    for r in range(a.device_rounds):                                            # the three feeds alternate: each round times every one of them
        for leg in legs:
            tr = CIRTrainer(m, steps_per_epoch=10 ** 9, cfg=CIRTrainConfig(accumulation_steps=1), params=params)
            s = [0]

            def step():
                i = s[0]; s[0] += 1
                if leg == "devicefed":
                    b = ds.batch(order[(i % n_steps) * B:(i % n_steps + 1) * B], ds.draw_of(r, i))
                else:
                    b = resident if leg == "resident" else pinned
                tr.micro_step(b, i)
            legs[leg].append(timed(step, a.steps, a.warmup))
            del tr
    for leg, t in legs.items():
        res[f"ms_step_{leg}_b{B}"] = float(np.median(t))
        res[f"ms_step_{leg}_rounds_b{B}"] = [float(v) for v in t]
    lo, hi = min(legs["resident"]), max(legs["resident"])
    res[f"devicefed_inside_resident_range_b{B}"] = bool(lo <= res[f"ms_step_devicefed_b{B}"] <= hi)
    res[f"devicefed_over_resident_b{B}"] = res[f"ms_step_devicefed_b{B}"] / res[f"ms_step_resident_b{B}"]
    try:                                                                        # the committed host-side figure the device build replaces
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cir_indexed_collate_bench.json")) as f:
            c = json.loads(f.readline())
        res["ms_host_collate_indexed_committed"], res["host_collate_batch"] = c["ms_collate_indexed"], c["batch"]
    except (OSError, ValueError, KeyError):
        pass
    del m.embedding_table
    return res


def cir_main(a, m, params):
    from outfitx_amd.engine import set_rank_loss
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    from src.losses import SetWiseRankingLoss
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    K, D = a.negatives, 1024
    off = {id(m.outfit_token)} | {id(p) for p in m.cp_ffn.parameters()}
    params = [p for p in params if id(p) not in off]
    res = {"workload": f"CIR trainer step, outfits x {a.items} items (padded {a.pad}), {K} negatives per query, precomputed embeddings",
           "precision": a.precision, "loss_reps": a.loss_reps}

    def device_leg():
        dres = cir_device_bench(a, m, params, a.device_batch, K)
        if a.device_out:
            with open(a.device_out, "w") as f:
                f.write(json.dumps(dres) + "\n")
        return dres

    if a.device_only:
        print(json.dumps(device_leg()))
        return
    for B in [int(v) for v in a.cir_batches.split(",")]:
        emb, mask = synth.outfit_batch(99, B, a.pad, a.items)
        batch = {"input_dict": {"task": CIR, "outfit_embedding": torch.from_numpy(emb).cuda(), "outfit_mask": torch.from_numpy(mask).cuda(),
                                "target_item_text_embedding": torch.from_numpy(synth.unit_rows(99, "target_text", B, 512)).cuda()},
                 "pos_item_embedding": torch.from_numpy(synth.item_embeddings(99, "pos", B) * 3.0).cuda(),
                 "neg_items_embedding": torch.from_numpy(synth.item_embeddings(99, "neg", B * K).reshape(B, K, D) * 3.0).cuda(),
                 "neg_items_mask": torch.from_numpy(np.random.default_rng(99).random((B, K)) < 0.1).cuda()}
        for acc in (1, 4):
            tr = CIRTrainer(m, steps_per_epoch=10 ** 9, cfg=CIRTrainConfig(accumulation_steps=acc), params=params)
            k = [0]
            def dp_step():
                tr.micro_step(batch, k[0]); k[0] += 1
            res[f"ms_step_dp_b{B}" if acc == 1 else f"ms_step_dp_accum4_b{B}"] = timed(dp_step, a.steps if acc == 1 else 4 * max(a.steps // 4, 1), a.warmup if acc == 1 else 4)
            del tr
        # the loss alone, forward + backward
        y_hat0 = torch.from_numpy(synth.item_embeddings(99, "y_hat", B) * 3.0).cuda()
        y, neg, nm = batch["pos_item_embedding"], batch["neg_items_embedding"], batch["neg_items_mask"]
        fused = SetWiseRankingLoss(margin=2.0)

        def loss_fused():
            yh = y_hat0.detach().requires_grad_(True)
            fused(batch_y=y, batch_y_hat=yh, batch_negative_samples=neg, batch_negative_mask=nm).backward()
            return yh.grad

        def loss_eager():
            yh = y_hat0.detach().requires_grad_(True)
            eager_set_rank_loss(y, yh, neg, nm).backward()
            return yh.grad

        ga, gb = loss_fused(), loss_eager()
        res[f"loss_grad_fused_vs_eager_b{B}"] = float((ga - gb).abs().max() / gb.abs().max())
        t_f, t_e, t_k = median_ms([loss_fused, loss_eager, lambda: set_rank_loss(y, y_hat0, neg, nm, 2.0)], a.loss_reps, 5)
        nbytes = B * K * D * 4 + 3 * B * D * 4
        res[f"ms_loss_fwd_bwd_fused_b{B}"], res[f"ms_loss_fwd_bwd_eager_b{B}"], res[f"ms_loss_kernel_call_b{B}"] = t_f, t_e, t_k
        res[f"loss_eager_over_fused_b{B}"] = t_e / t_f
        res[f"loss_kernel_GBps_b{B}"] = nbytes / (t_k * 1e-3) / 1e9
    ires = {"workload": f"index-form CIR batches against the dense batches gathered from the same rows of a {a.table}-row table, "
                        f"{a.items} items per outfit (padded {a.pad}), {K} negatives per query, 10 % padded", "precision": a.precision,
            "loss_reps": a.loss_reps, "steps": a.steps}
    for B in [int(v) for v in a.cir_batches.split(",")]:
        cir_indexed_bench(a, m, params, B, K, ires)
    res.update({k: v for k, v in ires.items() if k not in res})
    res.update({k: v for k, v in device_leg().items() if k not in res})
    print(json.dumps(res))
    if a.indexed_out:
        with open(a.indexed_out, "w") as f:
            f.write(json.dumps(ires) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=["cp", "cir"], default="cp")
    ap.add_argument("--cir-batches", default="256,3072")
    ap.add_argument("--negatives", type=int, default=10)
    ap.add_argument("--loss-reps", type=int, default=30)
    ap.add_argument("--table", type=int, default=100_000, help="rows of the device-resident embedding table (CIR task, index form)")
    ap.add_argument("--indexed-out", default="", help="also write the index-form keys to this file (CIR task)")
    ap.add_argument("--pools", type=int, default=32, help="negative pools the table's rows fall into (CIR task, device-built batches)")
    ap.add_argument("--device-batch", type=int, default=3072, help="batch of the device-built leg (CIR task)")
    ap.add_argument("--device-rounds", type=int, default=5, help="rounds over the resident / host-fed / device-fed steps, alternating (CIR task)")
    ap.add_argument("--device-out", default="", help="also write the device-built leg's line to this file (CIR task)")
    ap.add_argument("--device-only", action="store_true", help="CIR task: the device-built leg alone")
    ap.add_argument("--boundary-reps", type=int, default=30)
    ap.add_argument("--boundary-out", default="", help="also write the JSON line to this file (CP task)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--pad", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--polyvore", action="store_true", help="SURVEY.md §8d config 5 inputs: outfit lengths uniform{2..8} padded to 16, labels Bernoulli(0.5)")
    a = ap.parse_args()
    from src.losses import FocalLoss
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    cfg.transformer.dropout = 0.0
    m = OutfitX(cfg, train_precision=a.precision)
    sd = synth.outfit_transformer_weights(7)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    m = m.cuda().train()
    params = [v for k, v in m.named_parameters() if not k.startswith("item_encoder.")]
    if a.task == "cir":
        return cir_main(a, m, params)
    opt = torch.optim.AdamW(params, lr=2e-5)
    n_items = synth.ragged_lengths(99, a.batch, 2, 8) if a.polyvore else a.items
    emb, mask = synth.outfit_batch(99, a.batch, a.pad, n_items)
    emb, mask = torch.from_numpy(emb).cuda(), torch.from_numpy(mask).cuda()
    labels = (torch.from_numpy(np.random.default_rng(99).random(a.batch) < 0.5).float() if a.polyvore else (torch.arange(a.batch) % 2).float()).cuda()
    loss_fn = FocalLoss(alpha=0.75, gamma=2, reduction="mean")

    def fwd_bwd():
        y = m(task=CP, outfit_embedding=emb, outfit_mask=mask).squeeze(-1)
        loss = loss_fn(y_hat=y, y_true=labels)
        loss.backward()
        return loss

    def step():
        opt.zero_grad(set_to_none=True)
        fwd_bwd()
        torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
        opt.step()

    def fwd_only():
        eng = m._engine(a.precision)
        eng.train_fwd("cp", (emb, mask))

    what = "2..8 items (uniform)" if a.polyvore else f"{a.items} items"
    res = {"workload": f"CP trainer step, {a.batch} outfits x {what} (padded {a.pad}), precomputed embeddings",
           "precision": a.precision}
    res["ms_step"] = timed(step, a.steps, a.warmup)
    res["ms_fwd_bwd"] = timed(lambda: (opt.zero_grad(set_to_none=True), fwd_bwd()), a.steps, a.warmup)
    res["ms_tape_fwd"] = timed(fwd_only, a.steps, a.warmup)
    res["outfits_per_s"] = a.batch / res["ms_step"] * 1e3
    # the DP trainer's step (world size from the launcher; 1 = no collective)
    import torch.distributed as dist
    from outfitx_amd.trainer import CPTrainConfig, CPTrainer
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl")
    opt.zero_grad(set_to_none=True)
    batch = {"input_dict": {"task": CP, "outfit_embedding": emb, "outfit_mask": mask}, "label": labels}
    for acc in (1, 4):
        tr = CPTrainer(m, steps_per_epoch=10 ** 9, cfg=CPTrainConfig(accumulation_steps=acc), params=params)
        k = [0]
        def dp_step():
            tr.micro_step(batch, k[0]); k[0] += 1
        res["ms_step_dp" if acc == 1 else "ms_step_dp_accum4"] = timed(dp_step, a.steps if acc == 1 else 4 * max(a.steps // 4, 1), a.warmup if acc == 1 else 4)
        del tr
    for acc in (1, 4):                                          # the same steps with the fused boundary (CPTrainConfig.hip_optimizer)
        tr = CPTrainer(m, steps_per_epoch=10 ** 9, cfg=CPTrainConfig(accumulation_steps=acc, hip_optimizer=True), params=params)
        k = [0]
        def dp_step_hip():
            tr.micro_step(batch, k[0]); k[0] += 1
        res["ms_step_dp_hip" if acc == 1 else "ms_step_dp_accum4_hip"] = timed(dp_step_hip, a.steps if acc == 1 else 4 * max(a.steps // 4, 1), a.warmup if acc == 1 else 4)
        del tr
    boundary_bench(params, world, a.boundary_reps, res)
    res["world"] = world
    res["outfits_per_s_dp"] = world * a.batch / res["ms_step_dp"] * 1e3
    rows = int(np.sum(n_items) + a.batch) if a.polyvore else a.batch * (a.items + 1)
    D, Fp = 1024, 2048
    res["gemm_tflop_per_step"] = 3 * 2 * rows * (4 * D * D + 2 * Fp * D) * 6 / 1e12
    res["tflops"] = res["gemm_tflop_per_step"] / (res["ms_fwd_bwd"] * 1e-3)

    if a.eager:
        layer = torch.nn.TransformerEncoderLayer(d_model=1024, nhead=16, dim_feedforward=2024, dropout=0.0, batch_first=True,
                                                 norm_first=True, activation=torch.nn.functional.mish)
        enc = torch.nn.TransformerEncoder(layer, num_layers=6, enable_nested_tensor=False).cuda().train()
        tok = torch.nn.Parameter(torch.randn(1024, device="cuda") * 0.02)
        head = torch.nn.Linear(1024, 1).cuda()
        eparams = list(enc.parameters()) + [tok] + list(head.parameters())
        eopt = torch.optim.AdamW(eparams, lr=2e-5)
        km = torch.cat([torch.zeros(a.batch, 1, dtype=torch.bool, device="cuda"), mask], 1)

        def eager_step():
            eopt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                x = torch.cat([tok.view(1, 1, -1).expand(a.batch, 1, -1), emb], 1)
                y = head(enc(x, src_key_padding_mask=km)[:, 0]).squeeze(-1)
                ce = torch.nn.functional.binary_cross_entropy_with_logits(y.float(), labels, reduction="none")
                p = torch.sigmoid(y.float())
                pt = p * labels + (1 - p) * (1 - labels)
                loss = ((0.75 * labels + 0.25 * (1 - labels)) * ce * (1 - pt) ** 2).mean()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(eparams, max_norm=1.0)
            eopt.step()

        res["ms_step_torch_eager_bf16"] = timed(eager_step, a.steps, a.warmup)
        res["speedup_vs_torch_eager"] = res["ms_step_torch_eager_bf16"] / res["ms_step"]
    if int(os.environ.get("RANK", "0")) == 0:
        print(json.dumps(res))
        if a.boundary_out:
            with open(a.boundary_out, "w") as f:
                f.write(json.dumps(res) + "\n")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
