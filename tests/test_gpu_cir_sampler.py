"""CIR training batches drawn on a real MI355X: ofx_cir_sample_batch (outfitx_amd/csrc/cir_sample.hip) against its numpy restatement
(tests/cir_sampler_ref.py) with torch.equal on all four outputs - the draw is counter-based, a pure function of its arguments, so there
is no tolerance -, its refusals, and sampler.CIRDeviceDataset feeding CIRTrainer.  Outputs of raw calls sit between guard words and are
poisoned first: what the call does not own, the unwritten tail of item_index included, must still hold the poison."""
import warnings

import numpy as np
import pytest
import torch

import cir_sampler_ref as R

warnings.simplefilter("ignore")
pytestmark = pytest.mark.gpu
OFX_EINVAL, OFX_ESHAPE = -1, -2
POISON, GUARD = 0x5A5A5A5A, 64
TABLES = ("outfit_cu", "outfit_rows", "pos_cu", "pos_slots", "pool_cu", "pool_rows", "row_pool", "row_slot")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# pool sizes m: 5000; m - 1 = K and K + 1 for K = 10, 64 and 1; m - 1 < K; a pool of the target alone
POOL_SIZES = [5000, 11, 12, 65, 66, 2, 3, 5, 1]


def make_world():
    """-> (row_key, outfits, positive_idx_lists, name -> outfit id).  Rows of pool g are contiguous; 12 rows lie in no pool."""
    g = np.random.default_rng(42)
    key = np.concatenate([np.full(m, 7 * i + 2) for i, m in enumerate(POOL_SIZES)] + [np.full(12, -1)])
    first = np.concatenate([[0], np.cumsum(POOL_SIZES)])
    n_table = len(key)
    outfits, pos, name = [], [], {}

    def add(tag, rows, p):
        name[tag] = len(outfits)
        outfits.append([int(r) for r in rows]); pos.append(list(p))

    for i, m in enumerate(POOL_SIZES):                                   # the target at the first / the last slot of every pool, P = 1
        add(f"first{i}", [first[i], first[i + 1] - 1 if m > 1 else 0, 17], [0])
        add(f"last{i}", [3, first[i + 1] - 1], [1])
    add("no_pool", [n_table - 1, 5], [0])                                # a target without a pool: all -1
    add("two", [5000, 40], [0, 1])                                       # 2 items: one remains
    add("n64", g.choice(n_table, 64, replace=False), range(64))          # 64 items, P = n
    add("n17", g.choice(n_table, 17, replace=False), range(17))          # n - 1 = 16
    add("n18", g.choice(n_table, 18, replace=False), [0, 17])            # n - 1 = 17
    add("n33", g.choice(n_table, 33, replace=False), range(0, 33, 2))    # n - 1 = 32 > 31
    for k in range(40):
        n = int(g.integers(2, 25))
        add(f"r{k}", g.choice(n_table, n, replace=False), sorted(g.choice(n, int(g.integers(1, n + 1)), replace=False).tolist()))
    return key, outfits, pos, name


@pytest.fixture(scope="module")
def world():
    key, outfits, pos, name = make_world()
    split, pools = R.build_split(outfits, pos), R.build_pools(key)
    dev = {k: cu(v) for k, v in {**split, **pools}.items()}
    return {"key": key, "outfits": outfits, "pos": pos, "name": name, "split": split, "pools": pools, "dev": dev}


def guarded(n):
    """-> (whole buffer, the n-element view the call gets): GUARD poisoned words on either side; the view starts 16-byte aligned."""
    whole = torch.full((GUARD + max(n, 1) + GUARD,), POISON, dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def raw_call(dev, ids, seed, draw, K, max_len, B=None, null=(), shift=(), null_neg=False, **counts):
    """ofx_cir_sample_batch on device tables -> (rc, outputs, whole guarded buffers).  null / shift: names of pointers passed as NULL /
    4 bytes off; counts: n_outfits ... n_table overriding what the tensors' lengths say."""
    from outfitx_amd import _lib as L
    lib = L.load()
    tid = cu(np.asarray(ids, np.int32))
    B = len(ids) if B is None else B
    n = max(len(ids), 1)
    outs = {"item_index": guarded(n * max(max_len, 1)), "cu_seqlens": guarded(n + 1), "target_item_index": guarded(n), "neg_items_index": guarded(n * max(K, 1))}
    ptr = {k: dev[k].data_ptr() for k in TABLES}
    ptr["outfit_ids"] = tid.data_ptr()
    ptr.update({k: v[1].data_ptr() for k, v in outs.items()})
    if K <= 0 or null_neg:
        ptr["neg_items_index"] = None
    for k in null:
        ptr[k] = None
    for k in shift:
        ptr[k] += 4
    c = {"n_outfits": dev["outfit_cu"].numel() - 1, "n_outfit_rows": dev["outfit_rows"].numel(), "n_pos_slots": dev["pos_slots"].numel(),
         "n_pools": dev["pool_cu"].numel() - 1, "n_pool_rows": dev["pool_rows"].numel(), "n_table": dev["row_pool"].numel()}
    c.update(counts)
    rc = lib.ofx_cir_sample_batch(ptr["outfit_cu"], ptr["outfit_rows"], c["n_outfits"], c["n_outfit_rows"], ptr["pos_cu"], ptr["pos_slots"], c["n_pos_slots"],
                                  ptr["pool_cu"], ptr["pool_rows"], c["n_pools"], c["n_pool_rows"], ptr["row_pool"], ptr["row_slot"], c["n_table"],
                                  ptr["outfit_ids"], B, seed, draw, K, max_len, ptr["item_index"], ptr["cu_seqlens"], ptr["target_item_index"],
                                  ptr["neg_items_index"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: v[1] for k, v in outs.items()}, {k: v[0] for k, v in outs.items()}


def untouched(t):
    return bool((t == POISON).all())


def check_against_restatement(w, ids, seed, draw, K, max_len):
    rc, out, whole = raw_call(w["dev"], ids, seed, draw, K, max_len)
    assert rc == 0
    item, cus, tgt, neg = R.sample_batch(w["split"], w["pools"], ids, seed, draw, K, max_len)
    B, total = len(ids), int(cus[-1])
    assert torch.equal(out["cu_seqlens"], cu(cus)), "cu_seqlens"
    assert torch.equal(out["target_item_index"], cu(tgt)), "target_item_index"
    assert torch.equal(out["item_index"][:total], cu(item)), "item_index"
    assert untouched(out["item_index"][total:]), "the tail of item_index was written"
    if K:
        assert torch.equal(out["neg_items_index"].view(B, K), cu(neg)), "neg_items_index"
    else:
        assert untouched(out["neg_items_index"])
    for k, t in whole.items():                                           # nothing outside the arrays
        assert untouched(t[:GUARD]) and untouched(t[-GUARD:]), k
    return item, cus, tgt, neg


@pytest.mark.parametrize("K,max_len", [(10, 16), (0, 1), (1, 31), (64, 16), (64, 31), (10, 1)])
def test_one_query_of_every_kind_equals_the_restatement(world, K, max_len):
    """B = 1, query by query: every pool-size regime with the target at the first and at the last slot, a target without a pool, outfits
    of 2, 17, 18, 33 and 64 items (one remains; n - 1 = max_len; truncation), P = 1 and P = n."""
    for tag in [t for t in world["name"] if not t.startswith("r")]:
        item, cus, tgt, neg = check_against_restatement(world, [world["name"][tag]], 77, 5, K, max_len)
        n = len(world["outfits"][world["name"][tag]])
        assert cus[1] == min(n - 1, max_len), tag
        if K and tag[:-1] in ("first", "last"):
            m1 = POOL_SIZES[int(tag[-1])] - 1
            assert int((neg >= 0).sum()) == min(m1, K), tag
        if tag == "no_pool":
            assert (neg == -1).all()


@pytest.mark.parametrize("B,K,max_len", [(5, 10, 16), (5, 0, 31), (300, 10, 16), (300, 64, 31), (300, 1, 1), (1027, 3, 16)])
def test_batches_equal_the_restatement(world, B, K, max_len):
    """B = 5: one block, three of its waves idle in the second; B = 300: 75 blocks of four waves, and a scan in which most threads own
    nothing; B = 1027: scan threads that own two slots, a ragged last block.  Outfit ids repeat within the batch."""
    g = np.random.default_rng(B + K)
    ids = g.integers(0, len(world["outfits"]), B)
    ids[:: max(B // 4, 1)] = world["name"]["n64"]
    for draw in (0, 2 ** 32 - 1):
        check_against_restatement(world, ids, 123456789, draw, K, max_len)


def test_one_outfit_in_every_slot_draws_differently_and_a_draw_repeats(world):
    ids = [world["name"]["n64"]] * 40
    a = check_against_restatement(world, ids, 9, 1, 10, 31)
    b = check_against_restatement(world, ids, 9, 1, 10, 31)
    c = check_against_restatement(world, ids, 9, 2, 10, 31)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[3], c[3])
    assert len({tuple(r) for r in a[0].reshape(40, 31).tolist()}) == 40 and len(set(a[2].tolist())) > 10 and len({tuple(r) for r in a[3].tolist()}) > 30


def test_outfit_ids_outside_the_split_are_clamped_into_it(world):
    """n_outfits = 20 of the allocated split: ids 20 .. give the bits of the call with the ids clamped to 19.  Every address an unclamped
    kernel would read is inside the allocations, so a missing clamp fails the comparison instead of faulting."""
    ids = np.array([3, 25, 19, 40, 20, 7], np.int32)
    got = raw_call(world["dev"], ids, 5, 6, 10, 16, n_outfits=20)
    want = raw_call(world["dev"], np.minimum(ids, 19), 5, 6, 10, 16, n_outfits=20)
    free = raw_call(world["dev"], ids, 5, 6, 10, 16)
    assert got[0] == 0 and want[0] == 0 and free[0] == 0
    assert all(torch.equal(got[1][k], want[1][k]) for k in got[1])
    assert not torch.equal(free[1]["target_item_index"], got[1]["target_item_index"])


def test_refusals_return_their_code_and_launch_nothing(world):
    from outfitx_amd import _lib as L
    lib = L.load()
    ids = [0, 1, 2, 3]
    pointers = TABLES + ("outfit_ids", "item_index", "cu_seqlens", "target_item_index")
    cases = [(dict(null=(k,)), OFX_EINVAL) for k in pointers] + [(dict(shift=(k,)), OFX_EINVAL) for k in pointers + ("neg_items_index",)]
    cases += [(dict(null_neg=True), OFX_EINVAL), (dict(B=0), OFX_EINVAL), (dict(B=-3), OFX_EINVAL),
              (dict(K=-1), OFX_ESHAPE), (dict(K=65), OFX_ESHAPE), (dict(max_len=0), OFX_ESHAPE), (dict(max_len=32), OFX_ESHAPE),
              (dict(n_outfits=0), OFX_ESHAPE), (dict(n_table=0), OFX_ESHAPE), (dict(n_pools=-1), OFX_ESHAPE), (dict(n_pool_rows=-1), OFX_ESHAPE)]
    for kw, code in cases:
        kw = dict(kw)
        K, max_len = kw.pop("K", 10), kw.pop("max_len", 16)
        rc, out, whole = raw_call(world["dev"], ids, 1, 2, K, max_len, **kw)
        assert rc == code and b"cir_sample_batch" in lib.ofx_last_error(), (kw, K, max_len, rc, lib.ofx_last_error())
        assert all(untouched(t) for t in whole.values()), (kw, K, max_len)
    rc, out, whole = raw_call(world["dev"], ids, 1, 2, 0, 16)             # K = 0 takes the NULL neg_items_index
    assert rc == 0 and untouched(whole["neg_items_index"]) and not untouched(out["cu_seqlens"])
    from outfitx_amd.engine import Engine                                # the wrapper has no CPU form
    host = {k: torch.from_numpy(v) for k, v in {**world["split"], **world["pools"]}.items()}
    with pytest.raises(L.OfxError):
        Engine.cir_sample_batch(host, host, torch.zeros(2, dtype=torch.int32), 0, 0, 10, 16)
    got = Engine.cir_sample_batch(world["dev"], world["dev"], cu(np.asarray(ids, np.int32)), 1, 2, 10, 16)
    rc, out, _ = raw_call(world["dev"], ids, 1, 2, 10, 16)
    total = int(out["cu_seqlens"][-1])
    assert torch.equal(got[1], out["cu_seqlens"]) and torch.equal(got[2], out["target_item_index"]) and torch.equal(got[3].reshape(-1), out["neg_items_index"])
    assert torch.equal(got[0][:total], out["item_index"][:total]) and got[0].numel() == 4 * 16


# ------------------------------------------------------------------------------------------------ dataset and trainer
def small_dataset(negatives=5, seed=3):
    from outfitx_amd.sampler import CIRDeviceDataset, CIRNegativePools
    g = np.random.default_rng(31)
    n_table = 200
    easy = g.integers(0, 3, n_table); hard = easy * 4 + g.integers(0, 4, n_table)
    easy[:5] = -1; hard[:5] = -1
    outfits = [g.choice(n_table, int(g.integers(2, 22)), replace=False).tolist() for _ in range(20)]
    pos = [sorted(g.choice(len(o), int(g.integers(1, len(o) + 1)), replace=False).tolist()) for o in outfits]
    pools = {"easy": CIRNegativePools(easy), "hard": CIRNegativePools(hard)}
    ds = CIRDeviceDataset(outfits, pools["easy"], pos, max_length=16, negatives=negatives, seed=seed)
    return ds, pools, outfits, pos, {"easy": easy, "hard": hard}


def host_form(batch):
    """The batch as a host-side index collate would hand it over: CPU tensors, item_index cut to its compact part."""
    i = batch["input_dict"]
    total = int(i["cu_seqlens"][-1])
    return {"input_dict": {"task": i["task"], "item_index": i["item_index"][:total].cpu(), "cu_seqlens": i["cu_seqlens"].cpu(),
                           "target_item_index": i["target_item_index"].cpu()},
            "pos_item_index": batch["pos_item_index"].cpu(), "neg_items_index": batch["neg_items_index"].cpu()}


def test_dataset_batches_equal_the_restatement_and_set_pools_changes_the_negatives_only():
    ds, pools, outfits, pos, keys = small_dataset()
    split = R.build_split(outfits, pos)
    ids = np.array([4, 4, 0, 19, 7, 11, 11], np.int32)
    easy = ds.batch(cu(ids), 9)
    assert easy["pos_item_index"] is easy["input_dict"]["target_item_index"] and easy["neg_items_index"].shape == (7, 5)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in (easy["neg_items_index"], *[v for k, v in easy["input_dict"].items() if k != "task"]))
    ds.set_pools(pools["hard"])
    hard = ds.batch(ids.tolist(), 9)                                     # a host list is converted
    for b, name in ((easy, "easy"), (hard, "hard")):
        item, cus, tgt, neg = R.sample_batch(split, R.build_pools(keys[name]), ids, ds.seed, 9, 5, 16)
        h = host_form(b)
        assert np.array_equal(h["input_dict"]["item_index"].numpy(), item) and np.array_equal(h["input_dict"]["cu_seqlens"].numpy(), cus), name
        assert np.array_equal(h["pos_item_index"].numpy(), tgt) and np.array_equal(h["neg_items_index"].numpy(), neg), name
    he, hh = host_form(easy), host_form(hard)
    assert all(torch.equal(he["input_dict"][k], hh["input_dict"][k]) for k in ("item_index", "cu_seqlens", "target_item_index"))
    assert not torch.equal(he["neg_items_index"], hh["neg_items_index"])
    # an epoch: steps_per_epoch batches in the order of `order`, the last one ragged, draws by draw_of; the ranks split the same permutation
    order = ds.order(2).cpu().numpy()
    assert sorted(order.tolist()) == list(range(20)) and not np.array_equal(order, np.arange(20)) and np.array_equal(order, ds.order(2).cpu().numpy())
    assert not np.array_equal(order, ds.order(3).cpu().numpy()) and np.array_equal(ds.order(2, shuffle=False).cpu().numpy(), np.arange(20))
    batches = list(ds.epoch(8, 2))
    assert [b["pos_item_index"].numel() for b in batches] == [8, 8, 4] and ds.steps_per_epoch(8) == 3
    assert len(list(ds.epoch(8, 2, drop_last=True))) == 2
    for step, b in enumerate(batches):
        want = R.sample_batch(split, R.build_pools(keys["hard"]), order[8 * step:8 * step + 8], ds.seed, ds.draw_of(2, step), 5, 16)
        h = host_form(b)
        got = (h["input_dict"]["item_index"], h["input_dict"]["cu_seqlens"], h["pos_item_index"], h["neg_items_index"])
        assert all(np.array_equal(x.numpy(), y) for x, y in zip(got, want)), step
    parts = [ds.order(2, rank=r, world=3).cpu().numpy() for r in range(3)]
    assert all(len(p) == 7 for p in parts) and np.array_equal(np.stack(parts, 1).reshape(-1)[:20], order)
    ranked = list(ds.epoch(4, 2, rank=1, world=3))
    assert len(ranked) == ds.steps_per_epoch(4, world=3) == 2 and ds.draw_of(2, 1, 1, 3) == (2 * 2654435761 + 4) % 2 ** 32
    want = R.sample_batch(split, R.build_pools(keys["hard"]), parts[1][4:], ds.seed, ds.draw_of(2, 1, 1, 3), 5, 16)
    assert np.array_equal(host_form(ranked[1])["neg_items_index"].numpy(), want[3])


def test_a_batch_is_built_without_waiting_for_the_device():
    """ds.batch under torch's sync debug mode 'error': any synchronising call torch makes (a copy to the host, .item(), a blocking
    allocation path) raises.  The C entry itself issues two launches and nothing else (cir_sample.hip: no copy, no allocation, no
    event or stream wait), which the mode cannot see and the source states."""
    ds, _, _, _, _ = small_dataset()
    ids = cu(np.arange(16, dtype=np.int32))
    ds.batch(ids, 0)                                                      # library load and the allocator's first blocks happen here
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                                # this build has no such mode: the statement above is all there is
        print(f"torch.cuda.set_sync_debug_mode is not supported here: {e}")
        return
    try:
        b = ds.batch(ids, 1)
        sliced = ds.batch(ids[3:9], 2)                                    # a misaligned view: copied on the device
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert b["neg_items_index"].shape == (16, 5) and sliced["neg_items_index"].shape == (6, 5)


def test_cir_trainer_fed_from_the_device_equals_the_same_batches_fed_from_the_host():
    """CIRTrainer.train_epoch(ds.epoch(..)): three batches (8, 8, 4), accumulation 2 -> two optimizer steps on a one-layer model.  The
    same batches copied to host tensors (item_index cut to its compact part) and fed through the existing index-form path give the same
    epoch loss and the same parameters, bit for bit: the over-allocated item_index and the device-side cu_seqlens change nothing."""
    from outfitx_amd import synth
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    from test_gpu_cir_indexed import make_model, trainable
    ds, _, _, _, _ = small_dataset()
    table = synth.item_embeddings(31, "table", 200) * 3.0
    m = make_model()
    m.set_embedding_table(torch.from_numpy(table))
    start = {k: v.detach().clone() for k, v in trainable(m).items()}
    on_path = [p for p in CIRTrainer._default_params(m) if any(p is q for q in trainable(m).values())]
    runs = {}
    for name in ("device", "host"):
        with torch.no_grad():
            for k, v in trainable(m).items():
                v.copy_(start[k])
        m.mark_weights_changed()
        tr = CIRTrainer(m, steps_per_epoch=ds.steps_per_epoch(8), cfg=CIRTrainConfig(learning_rate=2e-5, accumulation_steps=2, n_epochs=1), params=on_path)
        batches = ds.epoch(8, 1) if name == "device" else [host_form(b) for b in ds.epoch(8, 1)]
        loss = tr.train_epoch(batches)["loss"]
        runs[name] = (loss, {k: v.detach().clone() for k, v in trainable(m).items()})
    (ld, pd), (lh, ph) = runs["device"], runs["host"]
    print("epoch loss", ld, lh)
    assert np.isfinite(ld) and ld == lh, (ld, lh)
    moved = [k for k in pd if not torch.equal(pd[k], start[k])]
    assert len(moved) >= len(pd) - 3, moved
    assert all(torch.equal(pd[k], ph[k]) for k in pd), [k for k in pd if not torch.equal(pd[k], ph[k])]
