#!/usr/bin/env python3
"""Headline benchmark: outfits/sec, CP forward with CLIP ViT-B/32 image + text encode
(BASELINE.json configs[1]: 256 outfits x 8 items per GPU, 224^2) on N MI355X, in the operand scheme that holds the north star's
1e-3 parity bound (f16 MFMA operands with split weights / three-product arithmetic where the error budget needs them).

One "step" = one pass of the hot path over one batch: item encoder (ViT-B/32 + text tower + concat
fuser) -> 6-layer outfit transformer -> CP head, through the drop-in `src.models.OutfitX` API.
Inputs are synthetic and already resident in HBM when the timed region starts (token ids stay on
the host like the reference's tokenizer output: 1 MB, copied inside the step).  Weak scaling: each
rank scores its own 256 outfits; the forward has no data-path collective.

    python bench.py --gpus 1 --steps 5 --warmup 2 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and reports the headline; --full adds everything
else (live roofline sample inside the timed region, breakdown step, parity against the oracle and the reference's fixture, CPU
baseline, launch-by-launch and secondary-rung figures, and for N > 1 the CIR leg).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

from outfitx_amd import synth  # noqa: E402

W_SEED = 7
PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters"

# ---- algorithmic (useful, pad-free) FLOPs, SURVEY.md §8(d) -------------------------------------
VIT_GEMM = 12 * 50 * 14_155_776 + 49 * 2 * 3072 * 768 + 2 * 768 * 512        # per image, GEMM kernel only
VIT_ATTN = 12 * 4 * 50 * 50 * 768


def txt_gemm(T): return 12 * T * 6_291_456 + 2 * 512 * 512
def txt_attn(T): return 12 * 4 * T * T * 512
def ot_gemm(n): return 6 * (1 + n) * 16_678_912 + 2 * 1024 * 0
def ot_attn(n): return 6 * 4 * (1 + n) ** 2 * 1024 + 2 * 1024


def oracle_logits(px, ids, att, mask, n_outfits):
    """fp32 numpy oracle (oracle/np_oracle.py, pinned to the reference's golden vectors) on the first outfits of the batch, the way
    the reference executes them (texts padded to 64 tokens): the parity number printed next to the throughput."""
    from oracle import np_oracle as O
    emb = O.item_encoder(px[:n_outfits], ids[:n_outfits], att[:n_outfits], synth.vision_weights(W_SEED), synth.text_weights(W_SEED))
    return O.cp_forward(emb, mask[:n_outfits], synth.outfit_transformer_weights(W_SEED))


def bench_reference_logits(w_seed, B, n, in_crc):
    """The reference's own CP logits of this batch (tests/golden/cfg2_bench_logits.npz: src.models.OutfitX run on the CPU in fp32 in the
    build container by oracle/gen_bench_golden.py) - or None when the run is not the fixture's configuration."""
    path = os.path.join(ROOT, "tests", "golden", "cfg2_bench_logits.npz")
    if not os.path.exists(path):
        return None
    z = np.load(path)
    if f"w{w_seed}" not in z or int(z["outfits"]) != B or int(z["items"]) != n:
        return None
    if (str(z["px_crc"]), str(z["ids_crc"])) != in_crc:
        raise RuntimeError("bench batch differs from the fixture's inputs (checksum mismatch)")
    return z[f"w{w_seed}"].astype(np.float32)


def host_cores():
    """CPU cores this process may actually use: the affinity mask capped by the cgroup CPU quota (a GPU box hands one job a 16-core
    share of a 256-thread host; 256 torch threads on that share run several times slower than 16)."""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                quota, period = txt[0], float(txt[1])
            else:
                quota, period = txt[0], float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota not in ("max", "-1") and float(quota) > 0:
                n = max(1, min(n, int(-(-float(quota) // period))))
            break
        except Exception:
            continue
    return n


def _log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _median_ms(fn, warm, iters):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def cpu_baseline(px, ids, att, n_items, cfg2_outfits):
    """our own plain-PyTorch fp32 restatement of the reference's CPU path (oracle/torch_ref.py, pinned to the
    reference's golden vectors - not the reference's files, which never travel to the GPU box), on this box's host cores,
    torch.set_num_threads(os.cpu_count()) and 1 thread, warm-up + timed iterations, median.
      cfg1: _cp_forward (outfit_x.py:120-144) on BASELINE configs[0]: 32 outfits, 8 items padded to 16 (S = 17 as the reference's
            processor feeds them), 3 warm-up + 10 timed;
      cfg2: a bounded sample of THIS bench's workload (towers + fuser + CP forward, texts padded to 64 tokens), 1 warm-up + 5 timed.
    Baseline only: a GPU/CPU ratio says nothing about kernel quality (the roofline fraction does)."""
    from oracle import torch_ref as T
    ncpu = os.cpu_count() or 1
    cores = host_cores()
    Wt, Wv, Wx = synth.outfit_transformer_weights(W_SEED), synth.vision_weights(W_SEED), synth.text_weights(W_SEED)
    rs, rv, rt = T.TorchRef(Wt), T.TorchRef(Wv), T.TorchRef(Wx)
    emb1, mask1 = synth.outfit_batch(1235, 32, 16, 8)
    emb1, mask1 = torch.from_numpy(emb1), torch.from_numpy(mask1)
    k = cfg2_outfits
    pxs, idss, atts = px[:k].cpu(), ids[:k], att[:k]
    m2 = torch.zeros(k, n_items, dtype=torch.bool)
    out = {}
    prev = torch.get_num_threads()
    with torch.no_grad():
        # thread count of the "all threads" leg: every core this process may use - unless that over-subscribes a CPU share the
        # process cannot see (a GPU box gives one job 16 cores of a 256-thread host without a visible cgroup quota): one probe
        # forward at each candidate, keep the faster; the count used is reported
        cand, best = sorted({min(ncpu, cores), min(ncpu, cores, 32), min(ncpu, cores, 16)}, reverse=True), None
        for nt in cand:
            torch.set_num_threads(nt)
            rs.cp(emb1[:8], mask1[:8])
            t0 = time.perf_counter(); rs.cp(emb1, mask1); dt = time.perf_counter() - t0
            _log(f"cpu baseline: probe {nt} threads: {dt * 1e3:.0f} ms")
            if best is None or dt < best[1]:
                best = (nt, dt)
        for name, nt in (("all_threads", best[0]), ("one_thread", 1)):
            torch.set_num_threads(nt)
            _log(f"cpu baseline: cfg1 on {nt} thread(s)")
            ms1 = _median_ms(lambda: rs.cp(emb1, mask1), 3, 10)
            out[name] = {"threads": nt, "cfg1": {"outfits": 32, "iters": 10, "warmup": 3, "median_ms": round(ms1, 2), "outfits_per_s": round(32e3 / ms1, 1)}}
            if name == "all_threads":
                _log(f"cpu baseline: cfg2 sample of {k} outfits on {nt} thread(s)")
                ms2 = _median_ms(lambda: rs.cp(T.item_encoder(rv, rt, pxs, idss, atts), m2), 1, 5)
                out[name]["cfg2_sample"] = {"outfits": k, "iters": 5, "warmup": 1, "median_ms": round(ms2, 1), "outfits_per_s": round(k * 1e3 / ms2, 3)}
    torch.set_num_threads(prev)
    a = out["all_threads"]
    return {"value": a["cfg2_sample"]["outfits_per_s"], "unit": "outfits/s", "cores": a["threads"], "kind": "port",
            "threads": a["threads"], "host_logical_cpus": ncpu, "iters": 5, "median_ms": a["cfg2_sample"]["median_ms"],
            "sample": f"{k} outfits x {n_items} items of the same batch ({k * n_items} images 224^2, {k * n_items} texts padded to 64 tokens as the reference feeds "
                      f"them), plain-PyTorch fp32 restatement (oracle/torch_ref.py), median of 5 after 1 warm-up on {a['threads']} threads",
            "cfg1_cp_forward_32_outfits": {"all_threads": a["cfg1"], "one_thread": out["one_thread"]["cfg1"],
                                           "note": "BASELINE configs[0] / BASELINE.md section 3: S = 17 rows as the reference's processor feeds them, 3 warm-up + 10 timed, median"}}


def cir_leg(a, rank, world, dev, rehearsal, fence):
    """BASELINE configs[3] on N ranks, after (never inside) the timed region: 1,000 query embeddings against a 100k-row pool that is
    ROW-SHARDED over the ranks; every rank scores all queries against its shard (fp32-exact distances + local top-50), ONE
    all_gather_into_tensor of the packed per-shard candidate lists (RCCL over xGMI; 600 KB per rank), deterministic merge
    (outfitx_amd/parallel.py::cir_topk; reference call site: complementary_item_retrieval_trainer.py:240-249, which scores on one GPU).
    Reports the time per call (MAX over ranks) and whether rank 0's UNSHARDED top-k of the first 100 queries over the whole pool is
    torch.equal to the sharded result."""
    import torch.distributed as dist
    from outfitx_amd.engine import Engine
    from outfitx_amd.parallel import cir_topk, shard_range
    nq, npool, k = a.cir_queries, a.cir_pool, 50
    lo, hi = shard_range(npool, rank, world)
    eng = Engine(dev)
    Q = torch.from_numpy((synth.item_embeddings(1244, "cir_queries", nq) * 3.0).astype(np.float32)).to(dev)
    shards = [synth.item_embeddings(1244, f"cir_pool_shard{r}", shard_range(npool, r, world)[1] - shard_range(npool, r, world)[0]) if (r == rank or rank == 0) else None
              for r in range(world)]                               # every shard has its own seeded stream: a rank draws its own rows, rank 0 all of them
    mine = torch.from_numpy(shards[rank]).to(dev)
    for _ in range(2):
        idx, dst = cir_topk(eng, Q, mine, k, lo)
    fence()
    iters = 10
    t0 = time.perf_counter()
    for _ in range(iters):
        idx, dst = cir_topk(eng, Q, mine, k, lo)
    torch.cuda.synchronize(dev)
    dt = torch.tensor([(time.perf_counter() - t0) / iters], device="cpu" if rehearsal else dev, dtype=torch.float64)
    dist.all_reduce(dt, op=dist.ReduceOp.MAX)
    t1 = time.perf_counter()
    for _ in range(iters):
        li, ld = eng.l2_topk(Q, mine, k, index_base=lo)           # the same call without the collective and the merge
    torch.cuda.synchronize(dev)
    local_ms = (time.perf_counter() - t1) / iters * 1e3
    equal = None
    if rank == 0:
        P = torch.from_numpy(np.concatenate(shards, 0)).to(dev)
        sub = min(100, nq)
        ui, ud = eng.l2_topk(Q[:sub], P, k)
        equal = bool(torch.equal(ui, idx[:sub]) and torch.equal(ud, dst[:sub]))
        del P
    fence()
    return {"cir_allgather_ms": round(float(dt.item()) * 1e3, 3), "cir_local_topk_ms_rank0": round(local_ms, 3), "cir_equal": equal,
            "cir_note": f"{nq} queries x {npool} pool rows x 1024 row-sharded over {world} ranks, k = {k}: local fp32-exact top-k + ONE all-gather of the packed candidate lists "
                        f"({nq * k * 12} B per rank) + merge, per call, MAX over ranks, 10 calls after 2; cir_equal: rank 0's unsharded top-k of the first {min(100, nq)} queries "
                        "over the whole pool is torch.equal (indices and distances) to the sharded result"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--outfits", type=int, default=256, help="outfits per GPU per step")
    ap.add_argument("--items", type=int, default=8)
    ap.add_argument("--precision", default="bf16x3", help="outfit transformer MFMA operand format")
    ap.add_argument("--tower-precision", default="f16w2x", help="CLIP towers operand scheme (outfitx_amd/_lib.py tower_scheme): f16w2x (default: f16 operands, split (hi, lo) weights on every ViT "
                    "GEMM, three-product text tower and projections - at this batch size inside 1e-3 of the reference on all 100 weight seeds swept: median 2.5e-4, p90 4.5e-4, worst 6.3e-4, "
                    "profiles/r04_seed_sweep_bench_scale.json) | f16w2h (the qkv correction on ViT layers 0-5 only: 3 %% faster, same sweep: median 3.0e-4, worst 7.35e-4; reported as `secondary_rung`) | "
                    "f16w2 (split weights on patch / out-proj / fc2 only: faster, worst seeds at 1.0e-3) | f16x3 | f16 | bf16 (single product, faster, 0.7-2.8e-3 / 7e-3 end to end: outside the bound)")
    ap.add_argument("--rung", default="f16w2h", help="a second, cheaper 1e-3-compliant-at-this-batch-size rung measured after the timed region and reported as `secondary_rung` (never `value`); '' = skip")
    ap.add_argument("--cpu-outfits", type=int, default=8, help="outfits of the batch checked against the fp32 oracle (0 = skip the oracle check and the CPU baseline)")
    ap.add_argument("--cpu-cfg2-outfits", type=int, default=2, help="sample size of the CPU baseline's cfg2 leg")
    ap.add_argument("--vit-streams", type=int, default=1, help="split the image batch over this many HIP streams (CLIPImageEncoder.vit_streams)")
    ap.add_argument("--graph", type=int, default=1, help="1 (default): the drop-in call replays - OutfitX._cp_forward captures a repeated eval-mode call into ONE HIP graph on its second "
                    "occurrence (OutfitX.graph_replay, outfitx_amd/graphs.py) and every later call is one graph launch - same kernels, same streams, bit-identical logits; the step that "
                    "carries the live roofline sample is issued launch by launch (events ride on the launches).  0: every step launch by launch (also reported, after the timed "
                    "region, as `launch_by_launch` in the --full line)")
    ap.add_argument("--cir-queries", type=int, default=1000, help="N > 1 only: queries of the BASELINE configs[3] retrieval leg run after the timed region (pool row-sharded over the ranks, "
                    "ONE all-gather of the per-shard candidate lists: the only data-path collective the north star names); 0 = skip")
    ap.add_argument("--cir-pool", type=int, default=100_000, help="pool rows of that leg (whole job; sharded over the ranks)")
    ap.add_argument("--overlap-towers", type=int, default=1, help="1 (default): the text tower runs on a side HIP stream beside the ViT (ItemEncoder.overlap_towers; "
                    "31.85 vs 32.85 ms/step); the ONE step sampled for the roofline and the breakdown step run single-stream so that launch times do not overlap")
    ap.add_argument("--secondary", default="bf16", help="tower scheme of the secondary (non-headline) measurement after the timed region ('' = skip)")
    ap.add_argument("--ln-fold", type=int, default=2, help="2 (product default): towers' LayerNorms folded into the GEMM epilogues and the residual stream kept as a (hi, lo) operand-type pair; 1: folded, fp32 stream; 0: materialised (A/B)")
    ap.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline figure (off by default: see the module docstring); "
                    "--cpu-outfits, --cpu-cfg2-outfits, --rung, --secondary and --cir-* only act with it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the CP logits of the last timed step to DIR/cp_logits.npy (float32; rank r > 0: "
                    "cp_logits_rank<r>.npy): the same arguments give the same inputs, so two builds can be compared output for output")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", 0)); world = int(os.environ.get("WORLD_SIZE", 1)); local = int(os.environ.get("LOCAL_RANK", 0))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    # OFX_BENCH_REHEARSAL=1: every rank uses GPU 0 and the collectives go over gloo - a control-flow rehearsal of the
    # N>1 path on a one-GPU box (its numbers mean nothing).  Normal runs: one rank per GPU over RCCL.
    rehearsal = os.environ.get("OFX_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local = 0
    if world > 1:            # N ranks share one host: each takes its share of the cores (token staging, pinned copies, the input generator)
        torch.set_num_threads(max(1, host_cores() // world))
        os.environ.setdefault("OMP_NUM_THREADS", str(max(1, host_cores() // world)))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    from outfitx_amd import _lib as L
    L.load().ofx_tune(6, a.ln_fold)

    model = OutfitX(OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip")), precision=a.precision,
                    tower_precision=a.tower_precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.full_state_dict(W_SEED).items()}, strict=True)
    model = model.to(dev).eval()
    model.item_encoder.image_enc.vit_streams = a.vit_streams
    model.item_encoder.overlap_towers = bool(a.overlap_towers)

    B, n = a.outfits, a.items
    seed = 1236 + rank                                                    # rank-local batch (weak scaling)
    # host-generated (numpy PCG64) so that the build container - where the reference itself can be imported,
    # oracle/gen_bench_golden.py - and this box see the same batch; preprocessing excluded from the timing
    px_np, ids_np, att_np = synth.bench_batch(seed, B, n)                 # [B,n,3,224,224] fp32; BOS + 6 words + EOS, padded to 64
    in_crc = (synth.checksum(px_np[:2]), synth.checksum(ids_np)) if a.full else None
    px = torch.from_numpy(px_np).to(dev)
    del px_np
    texts = {"input_ids": torch.from_numpy(ids_np).view(B, n, 64).pin_memory(), "attention_mask": torch.from_numpy(att_np).view(B, n, 64).pin_memory()}
    mask = torch.zeros(B, n, dtype=torch.bool, device=dev)

    def step():
        with torch.no_grad():
            return model(task=CP, outfit_embedding=None, outfit_mask=mask, encoder_input_dict={"images": px, "texts": texts})

    def fence():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    _log("model packed, inputs resident; warm-up")
    out = None
    for i in range(a.warmup):
        # the first warm-up step runs the towers on one stream, as the sampled step of the timed region does: torch's caching allocator then
        # already holds the blocks that step takes from the main stream's pool (no hipMalloc inside the timed region: `device_allocs_in_timed_region`)
        model.item_encoder.overlap_towers = bool(a.overlap_towers) and i != 0
        out = step()
    model.item_encoder.overlap_towers = bool(a.overlap_towers)
    fence()
    # --graph 1 (default): nothing to set up - the drop-in call itself replays.  OutfitX._cp_forward (eval mode) captures a repeated call on its
    # second occurrence and launches ONE HIP graph per call from the third on (outfitx_amd/graphs.py ForwardReplay); the timed steps below are
    # plain `model(task=CP, ...)` calls.  Untimed here: make sure the capture has happened and check its logits against the launch-by-launch ones.
    model.graph_replay = bool(a.graph)
    graph_on, graph_note = False, "off (--graph 0): every step launch by launch"
    if a.graph:
        eager_out = (out if out is not None else step()).clone()     # --warmup 0: one launch-by-launch step to compare the replay with
        for _ in range(6):
            rp = model._replay
            if rp is not None and rp.stats["replays"] >= 2:
                break
            out = step()
        torch.cuda.synchronize(dev)
        rp = model._replay
        if rp is not None and rp.stats["replays"] >= 1:
            if not torch.equal(out, eager_out):
                raise RuntimeError("replayed step's logits differ from the launch-by-launch step's")
            graph_on = True
            graph_note = ("one HIP graph launch per step: the drop-in call model(task=CP, ...) replays the step it captured on its second occurrence "
                          "(OutfitX.graph_replay, default on); logits bit-identical to the launch-by-launch step (checked before timing)")
        else:
            graph_note = f"capture failed ({rp.stats if rp is not None else 'call not eligible'}); steps issued launch by launch"
            _log(graph_note)
        fence()
    _log("timed region")
    lib = L.load()
    # --full only - live roofline sample: HIP events bracket every GEMM launch of ONE timed step (the middle one) on the launch
    # stream.  Bracketing all K steps costs ~1 ms/step of serialisation (246 event markers), so it is sampled.
    sample = a.steps // 2 if a.full else -1
    allocs0 = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)        # hipMalloc calls of torch's caching allocator so far
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)] if a.full else None     # one marker per step on torch's stream: the spread of the K steps
    t0 = time.perf_counter()
    if a.full:
        marks[0].record()
    host_t = [time.perf_counter()]
    for i in range(a.steps):
        if i == sample:
            model.item_encoder.overlap_towers = False        # per-launch events of concurrent kernels would count the shared time twice
            lib.ofx_profile_enable(1)
        out = step()                                        # the drop-in call: one graph launch (the sampled step: launch by launch, events ride on the launches)
        if i == sample:
            lib.ofx_profile_enable(0)
            model.item_encoder.overlap_towers = bool(a.overlap_towers)
        if a.full:
            marks[i + 1].record()
            host_t.append(time.perf_counter())
    fence()
    elapsed = time.perf_counter() - t0
    if a.dump_outputs:                                      # what the caller of the timed path received from its last step
        os.makedirs(a.dump_outputs, exist_ok=True)
        np.save(os.path.join(a.dump_outputs, "cp_logits.npy" if rank == 0 else f"cp_logits_rank{rank}.npy"), out.float().cpu().numpy())
    if a.full:
        per_step = [marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps)]
        allocs_timed = torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - allocs0
        recs = (L.ProfRecord * 4096)()
        nrec = lib.ofx_profile_records(recs, 4096)              # per-launch records of the sampled step (before read() clears them)
        ms, fl, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_longlong * 4)()
        L.check(lib.ofx_profile_read(ms, fl, cnt), "ofx_profile_read")
        # one extra, untimed step with every category bracketed: the per-step breakdown
        lib.ofx_profile_enable(15)
        model.item_encoder.overlap_towers = False
        step(); fence()
        model.item_encoder.overlap_towers = bool(a.overlap_towers)
        bms, bfl, bcnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_longlong * 4)()
        L.check(lib.ofx_profile_read(bms, bfl, bcnt), "ofx_profile_read")
        lib.ofx_profile_enable(0)
    rank_info = None
    if world > 1:
        # whole-job time = the slowest rank's; every rank's own time, batch seed and host thread count travel to rank 0 for the line
        mine = torch.tensor([elapsed, float(seed), float(torch.get_num_threads()), 1.0 if graph_on else 0.0], device="cpu" if rehearsal else dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        rank_info = {"elapsed_s": [round(float(x[0]), 6) for x in allr], "batch_seeds": [int(x[1]) for x in allr], "host_threads": [int(x[2]) for x in allr],
                     "graph_launch": [bool(x[3]) for x in allr]}
        t = torch.tensor([elapsed], device="cpu" if rehearsal else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        if a.full and a.cir_queries > 0:
            rank_info.update(cir_leg(a, rank, world, dev, rehearsal, fence))

    if rank == 0:
        T_real = 8
        alg_gemm_outfit = n * (VIT_GEMM + txt_gemm(T_real)) + ot_gemm(n)
        alg_all_outfit = alg_gemm_outfit + n * (VIT_ATTN + txt_attn(T_real)) + ot_attn(n)
        padded_outfit = n * (VIT_GEMM + VIT_ATTN + txt_gemm(64) + txt_attn(64)) + ot_gemm(16) + ot_attn(16)
        scheme = {"f16w2h": "f16w2h = f16 MFMA operands; split (hi, lo) weights on every ViT GEMM (patch embedding, qkv, out-proj, fc1, fc2): A hi^T in f16 + the correction A lo^T "
                            "on the block-scaled fp8 matrix instruction (gemm_w2f8_kernel, e5m2 activation image); the qkv correction on ViT layers 0-5 only (layers 6-11: fused single-product QKV + "
                            "attention kernel); text tower, ViT projection tail and the outfit transformer in three-product arithmetic",
                  "f16w2x": "f16w2x = f16 MFMA operands; split (hi, lo) weights on every ViT GEMM (patch embedding, qkv, out-proj, fc1, fc2): A hi^T in f16 + the correction A lo^T "
                            "on the block-scaled fp8 matrix instruction (gemm_w2f8_kernel; f16 lo product on small grids); text tower, ViT projection tail and the outfit "
                            "transformer in three-product arithmetic",
                  "f16w2": "f16w2 = f16 MFMA operands; split (hi, lo) weights (2 products per weight) on the ViT patch-embedding / out-proj / fc2 GEMMs; text tower, "
                           "ViT projection tail and the outfit transformer in three-product arithmetic",
                  "f16": "f16, one MFMA product per term", "bf16": "bf16, one MFMA product per term"}.get(a.tower_precision, a.tower_precision)
        op = "bf16" if a.tower_precision.startswith("bf16") else "f16"
        res = {
            "metric": "outfits/sec CP forward (8-item sets, 224^2, bf16)",      # BASELINE.json's metric name, verbatim; the arithmetic type is `dtype`
            "value": round(world * B * a.steps / elapsed, 2),
            "unit": "outfits/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(elapsed / a.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": op,
            "data": "synthetic (seeded uniform-uint8 images after CLIP normalise, 8-token ids, random-init weights of the reference architecture)",
            "config": {"workload": "BASELINE configs[1]: CP forward with CLIP ViT-B/32 image+text encode, 256 outfits x 8 items per GPU, 224^2",
                       "outfits_per_gpu": B, "items": n, "parallelism": f"dp{world} (batch sharded, no data-path collective)",
                       "tower_precision": scheme, "launch": graph_note,
                       "outfit_precision": (model._tower_fed() or a.precision) + (f" (set transformer fed by the in-call {op} towers)" if model._tower_fed() else ""),
                       "parity_bound": "north star: <= 1e-3 max|d| / max|ref| over the batch on the CP logit vs the fp32 reference path; measured on THIS batch by --full "
                                       "(parity_rel_err_vs_reference, all logits) and at this batch size on weight seeds 7/44/89/97/99 by "
                                       "tests/test_gpu_model.py::test_cfg2_bench_batch_within_1e3_of_the_reference (+ weights with massive ViT channels); over 100 weight seeds the error is a distribution "
                                       "(profiles/r04_seed_sweep_bench_scale.json: median 2.5e-4, p90 4.5e-4, worst 6.3e-4, none at or above 8e-4; lognormal fit: P(>= 1e-3) 0.12 % per weight draw); conditional on the random-init network's near-uniform attention: with q, k x 1.5 (logits x 2.25) 4 of 40 weight draws read >= 1e-3 (f16x3: none), DESIGN.md section 2"},
            "whole_step_tflops_useful": round(alg_all_outfit * world * B * a.steps / elapsed / 1e12, 2),
            # SURVEY.md 8(d) "report both": the FLOPs the reference's own execution spends on the same outfits (texts padded to
            # 64 tokens, sets padded to 1 + 16 rows) - context for the north star's "40 % of MFMA peak", never used for `achieved`
            "reference_padded_flop_count": {
                "gflop_per_outfit": round(padded_outfit / 1e9, 2),
                "tflops_equiv_per_gpu": round(padded_outfit * B * a.steps / elapsed / 1e12, 2),
                "frac_of_peak": round(padded_outfit * B * a.steps / elapsed / 1e12 / PEAK_BF16_TFLOPS, 4)},
        }
        if a.full:
            gemm_ms, gemm_launches = ms[0], int(cnt[0])
            achieved_fixed = alg_gemm_outfit * B / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0   # SURVEY 8(d)'s per-outfit count x outfits, one sampled step
            executed = fl[0] / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
            # per-shape table of the sampled step: shape -> kernel -> launches, us per launch, useful TF/s (2 M N K_logical) and its
            # fraction of the dense peak, executed TF/s (x kmul: split weights run 2, three-product GEMMs 3 MFMA products per term),
            # algorithmic HBM bytes per launch as the launch's own epilogue configuration implies (ofx_prof_record.bytes)
            KIND = {1: "gemm_128x128_kernel", 2: "gemm_big_kernel<2,4,2>", 3: "gemm_big_kernel<2,2,1>", 4: "gemm_pp_kernel", 6: "gemm_w2_kernel",
                    7: "fused_qkv_attn_kernel (N = q|k|v columns; its attention FLOPs are not in useful_tflops)", 8: "gemm_w2f8_kernel", 9: "gemm_x3_kernel"}
            shapes = {}
            for i in range(nrec):
                r = recs[i]
                if r.cat != 0:
                    continue
                e = shapes.setdefault((r.M, r.N, r.K, r.kmul, r.kind), [0, 0.0, 0.0])
                e[0] += 1; e[1] += r.ms; e[2] += r.bytes
            table, by_kernel = [], {}
            launched_flop = 0.0          # useful FLOPs of the shapes actually launched (the pruned last ViT layer runs fewer rows than 8(d) counts)
            for (M_, N_, K_, km_, kind_), (c_, t_, b_) in sorted(shapes.items(), key=lambda kv: -kv[1][1]):
                useful = 2.0 * M_ * N_ * K_ * c_ / (t_ * 1e-3) / 1e12
                launched_flop += 2.0 * M_ * N_ * K_ * c_
                # matrix-pipe work in f16-rate product equivalents: the fp8 correction product of gemm_w2f8_kernel runs at twice the f16 rate
                pe_ = 1.5 if kind_ == 8 else float(km_)
                table.append({"M": M_, "N": N_, "K": K_, "products_per_term": km_, "f16_rate_product_equivalents": pe_, "kernel": KIND.get(kind_, str(kind_)), "launches": c_,
                              "us_per_launch": round(t_ * 1e3 / c_, 1), "ms_per_step": round(t_, 3), "useful_tflops": round(useful, 1),
                              "frac_useful": round(useful / PEAK_BF16_TFLOPS, 4), "executed_tflops": round(useful * pe_, 1),
                              "algorithmic_mb_per_launch": round(b_ / c_ / 1e6, 1), "algorithmic_tb_per_s": round(b_ / (t_ * 1e-3) / 1e12, 2)})
                k_ = by_kernel.setdefault(KIND.get(kind_, str(kind_)).split(" ")[0], [0, 0.0, 0.0, 0.0])
                k_[0] += c_; k_[1] += t_; k_[2] += b_; k_[3] += 2.0 * M_ * N_ * K_ * c_
            achieved = launched_flop / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0      # useful FLOPs of the launched shapes: the graded figure
            alg_total = sum(v[2] for v in shapes.values())
            assert abs(alg_total - sum(v[2] for v in by_kernel.values())) <= 1e-6 * max(alg_total, 1.0)
            alg_per_launch = alg_total / max(gemm_launches, 1)
            # PMC counters cannot be read inside a timed run: `traffic` refers to the committed rocprofv3 --pmc passes of this same
            # command (tools/profile_r03.sh -> tools/pmc_mfma_util.py), per launch over every GEMM kernel, FETCH_SIZE x2 + WRITE_SIZE
            traffic, traffic_src, traffic_by_kernel = None, None, None
            for name in ("r04_mfma_util.json", "r03_mfma_util.json", "r02_mfma_util.json"):
                try:
                    with open(os.path.join(ROOT, "profiles", name)) as f:
                        pm = json.load(f)
                    traffic = round(pm["gemm_kernels"]["gemm_hbm_bytes_per_launch"]); traffic_src = name
                    traffic_by_kernel = pm.get("per_kernel_traffic")
                    break
                except Exception:
                    continue
            kernels = {kn: {"launches": v[0], "us_per_launch": round(v[1] * 1e3 / v[0], 1), "ms_per_step": round(v[1], 3),
                            "useful_tflops": round(v[3] / (v[1] * 1e-3) / 1e12, 1), "algorithmic_mb_per_launch": round(v[2] / v[0] / 1e6, 1)}
                       for kn, v in sorted(by_kernel.items(), key=lambda kv: -kv[1][1])}
            dom = max(by_kernel.items(), key=lambda kv: kv[1][1])[0] if by_kernel else None
            res.update({
                "step_ms_spread": {"min": round(min(per_step), 3), "median": round(sorted(per_step)[len(per_step) // 2], 3), "max": round(max(per_step), 3),
                                   "sampled_step": round(per_step[sample], 3), "all": [round(t, 2) for t in per_step],
                                   "device_allocs_in_timed_region": int(allocs_timed),
                                   "host_issue_ms": [round((host_t[i + 1] - host_t[i]) * 1e3, 2) for i in range(a.steps)],
                                   "note": "stream markers after each of the K timed steps (rank 0); the sampled step runs the towers on one stream with "
                                           "every GEMM launch bracketed by events (the live roofline sample) and is inside the timed region"},
                "roofline": {"bound": "mfma", "kernel": "every dense contraction of the step: " + " / ".join(sorted({t_["kernel"] for t_ in table})),
                             "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
                             "traffic_note": (f"bytes per GEMM launch, FETCH_SIZE x2 + WRITE_SIZE, read from the committed profiles/{traffic_src} (separate rocprofv3 --pmc passes of this "
                                              "command, tools/profile_r03.sh) - a reference to that file, not a measurement of this run") if traffic else "no PMC pass committed for this build yet",
                             "algorithmic_bytes_per_launch": round(alg_per_launch),
                             "traffic_over_algorithmic": round(traffic / alg_per_launch, 3) if traffic else None,
                             "note": "achieved = useful (pad-free, one product per term) FLOPs of the GEMM shapes actually LAUNCHED / summed GEMM launch time of one sampled step "
                                     "(HIP events on the launches); achieved_fixed_count uses SURVEY 8(d)'s per-outfit count instead (the pruned last ViT layer launches fewer rows "
                                     "than that count assumes: no pruning credit is taken in `achieved`); executed_tflops counts the extra MFMA products the 1e-3-compliant scheme "
                                     "spends (split weights x2, three-product x3)",
                             "achieved_fixed_count": round(achieved_fixed, 2), "frac_fixed_count": round(achieved_fixed / PEAK_BF16_TFLOPS, 4),
                             "executed_tflops": round(executed, 2), "executed_frac": round(executed / PEAK_BF16_TFLOPS, 4),
                             "launches_per_step": gemm_launches, "sampled_steps": 1,
                             "avg_launch_us": round(gemm_ms * 1e3 / max(gemm_launches, 1), 2),
                             "algorithmic_gflop_per_outfit": round(alg_gemm_outfit / 1e9, 3),
                             "launched_gflop_per_outfit": round(launched_flop / B / 1e9, 3),
                             "power_limited_reference": {"mfma_only_loop_tflops_random_f16_operands": [1790.8, 1833.9], "mfma_only_loop_tflops_zero_operands": 2404.7,
                                                         "note": "not measured by this run: tools/mfma_power_probe.hip on one MI355X (profiles/r03_power_limited_clock.txt) - a "
                                                                 "register-resident v_mfma_f32_16x16x32_f16 loop on every CU sustains 0.72-0.73 of `peak` on random operands (the clock the "
                                                                 "matrix pipe's switching power leaves); this bench's GEMMs run 22-29 % faster on constant operands. `peak` stays the guide's figure"},
                             "dominant_kernel": dom, "per_kernel": kernels, "per_kernel_traffic_pmc": traffic_by_kernel,
                             "per_shape": table},
                "step_breakdown_ms": {"gemm": round(bms[0], 3), "norm_embed": round(bms[1], 3), "attention": round(bms[2], 3),
                                      "other": round(bms[3], 3), "note": "one extra untimed step with all launches bracketed"},
            })
        if rank_info is not None:
            res["ranks"] = dict(rank_info, note="value = all ranks' outfits / max(elapsed_s): the slowest rank sets the whole-job time")
        if a.full and a.cpu_outfits > 0 and world == 1:      # parity + CPU baseline: single-GPU-run data (rank 0, N = 1 only), outside the timed region
            try:
                got_all = out.float().cpu().numpy().reshape(-1)
                ref_all = bench_reference_logits(W_SEED, B, n, in_crc)
                if ref_all is not None:         # ALL logits of the batch against the reference's own fp32 CPU output (committed fixture)
                    res["parity_rel_err_vs_reference"] = float(np.abs(got_all - ref_all).max() / np.abs(ref_all).max())
                    res["parity_abs_err_vs_reference"] = float(np.abs(got_all - ref_all).max())
                    res["parity_note"] = (f"max|d| / max|ref| over ALL {B} CP logits of the timed batch vs the reference itself (src.models.OutfitX on the CPU in fp32, "
                                          f"tests/golden/cfg2_bench_logits.npz from oracle/gen_bench_golden.py; input checksums verified), weight seed {W_SEED}")
                k = min(a.cpu_outfits, B)
                _log(f"timed region done: {elapsed / a.steps * 1e3:.2f} ms/step; live oracle check on {k} outfits")
                torch.set_num_threads(min(host_cores(), 32))
                ref = oracle_logits(px[:k].cpu().numpy(), texts["input_ids"][:k].numpy(), texts["attention_mask"][:k].numpy(), mask[:k].cpu().numpy(), k)
                got = out[:k].float().cpu().numpy()
                res["parity_rel_err_vs_oracle"] = float(np.abs(got - ref).max() / np.abs(ref).max())
                res["parity_oracle_note"] = f"the first {k} outfits recomputed live on this box by the fp32 numpy oracle (oracle/np_oracle.py): max|d| / max|ref| over those {k}"
                if ref_all is not None:
                    res["oracle_vs_reference_fixture"] = float(np.abs(ref.reshape(-1) - ref_all[:k]).max() / np.abs(ref_all[:k]).max())
                res["cpu_baseline"] = cpu_baseline(px, texts["input_ids"], texts["attention_mask"], n, min(a.cpu_cfg2_outfits, B))
                if a.graph:
                    # the same call with graph replay off (what --graph 0 times): 10 steps after 2, outside the timed region
                    model.graph_replay = False
                    for _ in range(2):
                        o1 = step()
                    fence()
                    t1 = time.perf_counter()
                    for _ in range(10):
                        o1 = step()
                    fence()
                    dt1 = (time.perf_counter() - t1) / 10
                    model.graph_replay = True
                    res["launch_by_launch"] = {"outfits_per_s": round(B / dt1, 1), "ms_per_step": round(dt1 * 1e3, 3), "steps": 10, "warmup": 2,
                                               "bit_identical_to_replayed": bool(torch.equal(o1, out)),
                                               "note": "the same drop-in call with OutfitX.graph_replay = False (what --graph 0 times): ~250 launches per step issued by the host"}
                if a.rung and a.rung != a.tower_precision:
                    # a cheaper rung of the same ladder (compliant at this batch size on its 100-seed sweep), same batch, the drop-in call as timed above:
                    # 2 launch-by-launch calls (the second is captured) + 2 replays untimed, then 10 replays timed; parity of ITS logits vs the fixture
                    _log(f"secondary measurement: rung {a.rung}")
                    model.item_encoder.set_precision(a.rung)
                    for _ in range(4):
                        o3 = step()
                    fence()
                    t1 = time.perf_counter()
                    for _ in range(10):
                        o3 = step()
                    fence()
                    dt3 = (time.perf_counter() - t1) / 10
                    g3 = o3.float().cpu().numpy().reshape(-1)
                    res["secondary_rung"] = {"tower_precision": a.rung + " (qkv correction on ViT layers 0-5 only; outfitx_amd/_lib.py)" if a.rung == "f16w2h" else a.rung,
                                             "outfits_per_s": round(B / dt3, 1), "ms_per_step": round(dt3 * 1e3, 3), "steps": 10,
                                             "parity_rel_err_vs_reference": (float(np.abs(g3 - ref_all).max() / np.abs(ref_all).max()) if ref_all is not None else None),
                                             "note": "not `value`: the default keeps the correction on every layer because this rung leaves 1e-3 on one small-logit 8-outfit weight draw "
                                                     "(tests/test_gpu_model.py, seed 99: 1.5e-3); at this batch size its 100-seed sweep reads median 3.0e-4, worst 7.35e-4"}
                    model.item_encoder.set_precision(a.tower_precision)
                if a.secondary and a.secondary != a.tower_precision:
                    # secondary, NON-compliant mode for context (never `value`): single-product towers, same batch, 5 steps after 2 warm-up
                    _log(f"secondary measurement: {a.secondary} towers")
                    model.graph_replay = False                 # launch by launch, as every earlier round's secondary figure
                    model.item_encoder.set_precision(a.secondary)
                    for _ in range(2):
                        o2 = step()
                    fence()
                    t1 = time.perf_counter()
                    for _ in range(5):
                        o2 = step()
                    fence()
                    dt2 = (time.perf_counter() - t1) / 5
                    g2 = o2.float().cpu().numpy().reshape(-1)
                    r2 = ref_all if ref_all is not None else ref.reshape(-1)
                    g2 = g2[:len(r2)]
                    res["secondary_single_product"] = {"tower_precision": a.secondary + ", one MFMA product per term (the round-1 headline mode)",
                                                       "outfits_per_s": round(B / dt2, 1), "ms_per_step": round(dt2 * 1e3, 3),
                                                       "parity_rel_err": float(np.abs(g2 - r2).max() / np.abs(r2).max()),
                                                       "note": "faster but outside the 1e-3 bound: reported for context only"}
                    model.item_encoder.set_precision(a.tower_precision)
                    model.graph_replay = bool(a.graph)
            except Exception as exc:      # the throughput line must survive a failure of the (host-side) checker / baseline legs
                res["post_timing_error"] = f"{type(exc).__name__}: {exc}"
                _log(f"post-timing leg failed: {exc!r}")
        print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
