"""Model-level tests on a real MI355X of the wide outfit transformer - d_model 1536, 16 heads of 96, dim_feedforward 2024: what
`OutfitXConfig()` describes, the model the reference's users train and serve - built without towers (`item_towers=False`) and fed
precomputed embeddings.  Weights: synth at d_model = 1536, 2 layers everywhere except the one 6-layer test.  Reference: the float64
restatement of tests/wide_set_cases.py (pinned on torch's own nn.TransformerEncoder by tests/test_cpu_wide_set.py).

Tolerances are the project's own per operand scheme, max|d| / max|ref| over the batch: bf16x3 and f16w2 1e-3 (the
north-star bound), f16 3e-3, bf16 3e-2 - operand-rounding floors relative to the signal, not functions of the width.  Every test prints
what it measured; DESIGN.md's parity table holds the numbers.

Batch sizes and the GEMM kernel each reaches (csrc/gemm.hip, ofx_launch_gemm; M = 17 B rows with 16 items per outfit, the pruned last
layer's out-proj / linear1 / linear2 run on M = B rows; N in {4608, 1536, 2048}; K in {1536, 2048}, x 3 in bf16x3, x 2 in f16w2):
  B = 1     M = 17 / 1      gemm_128x128, 128-row tiles, split-K at its deepest (up to 16 slices), second pass on the consumers
  B = 6     M = 49 / 6      ragged 1, 16, 5, 8, 2, 11: the same kernel, split-K with the fused consumers (slab attention, reduce + LayerNorm)
  B = 32    M = 544 / 32    gemm_128x128 with 64-row tiles (M > 64 and <= 384 tiles) and split-K where the plan wants it
  B = 256   M = 4352 / 256  bf16x3: gemm_x3 - persistent at N = 4608 / 2048 (612 / 272 tiles > CUs), one block per tile at N = 1536 (204);
                            f16 / bf16: 256x128 at N = 4608 (t3 = 612), gemm_128x128 unsplit at N = 1536 / 2048; f16w2: the dual-weight 256x256
                            kernel at N = 4608 (t2 = 306), gemm_128x128 with the wrapping A index at N = 1536 / 2048
  B = 1024  M = 17408 / 1024  bf16x3: gemm_x3 persistent; f16w2: the dual-weight 256x256 kernel (t2 >= 256 at every N); f16 / bf16: the 256x256
                            kernel at N = 4608 (t2 = 1224), 256x128 at N = 1536 / 2048; the B-row tail of the last layer: gemm_128x128 again
(the ping-pong kernel takes K <= 1024 only, and gemm_w2f8 needs the fp8 copies the outfit transformer does not keep: neither is
selectable at this width.)  At B >= 256 a 48-outfit subset is compared with the oracle.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import wide_set_cases as WS
from oracle import np_oracle as O
from outfitx_amd import synth

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

D = WS.D_WIDE
LENS6 = [1, 16, 5, 8, 2, 11]
TOL = {"bf16x3": 1e-3, "f16w2": 1e-3, "f16": 3e-3, "bf16": 3e-2}
W_SEED = 7


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tasks():
    from src.models.datatypes import (OutfitCompatibilityPredictionTask, OutfitComplementaryItemRetrievalTask, OutfitFillInTheBlankTask)
    return OutfitCompatibilityPredictionTask, OutfitComplementaryItemRetrievalTask, OutfitFillInTheBlankTask


@functools.lru_cache(maxsize=None)
def weights(d_model, n_layers):
    return synth.outfit_transformer_weights(W_SEED, d_model=d_model, n_layers=n_layers)


def build(enc_type, d_model, n_layers):
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig, TransformerConfig
    m = OutfitX(OutfitXConfig(item_encoder=ItemEncoderConfig(type=enc_type), transformer=TransformerConfig(n_layers=n_layers)), item_towers=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(d_model, n_layers).items()}, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return build("slip", D, 2)


def run(model, task, prec="bf16x3", **kw):
    model.precision = prec
    try:
        with torch.no_grad():
            return model(task=task, **kw)
    finally:
        model.precision = "bf16x3"


@functools.lru_cache(maxsize=None)
def batch(B, lens=None):
    """(emb, mask, txt) of B outfits; lens None: ragged 1 .. 16 from the seed."""
    n = synth.ragged_lengths(40 + B, B, 1, 16) if lens is None else np.asarray(lens)
    emb, mask = synth.outfit_batch(40 + B, B, 16, n, d_model=D)
    return emb, mask, synth.unit_rows(40 + B, "t", B, D // 2)


@functools.lru_cache(maxsize=None)
def oracle(B, lens=None, n_layers=2):
    """float64 CP logits and CIR embeddings of (at most 48 outfits of) batch(B, lens) -> (subset rows, cp, cir)."""
    emb, mask, txt = batch(B, lens)
    sub = np.arange(B) if B <= 48 else np.arange(0, B, B // 48)[:48]
    Wt = weights(D, n_layers)
    return sub, WS.cp_forward(emb[sub], mask[sub], Wt, n_layers=n_layers), WS.cir_forward(emb[sub], mask[sub], txt[sub], Wt, n_layers=n_layers)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("prec", ["bf16x3", "f16w2", "f16", "bf16"])
def test_cp_cir_fitb_vs_float64_all_precisions(model, prec):
    CP, CIR, FITB = tasks()
    emb, mask, txt = batch(6, tuple(LENS6))
    _, want_cp, want_cir = oracle(6, tuple(LENS6))
    cp = run(model, CP, prec, outfit_embedding=cu(emb), outfit_mask=cu(mask))
    cir = run(model, CIR, prec, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(txt))
    fitb = run(model, FITB, prec, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(txt))
    assert cp.shape == (6, 1) and cir.shape == (6, D) and cp.dtype == torch.float32
    e_cp, e_cir = WS.rel_err(cp.cpu().numpy(), want_cp), WS.rel_err(cir.cpu().numpy(), want_cir)
    print(f"PARITY d1536 2 layers B=6 ragged {prec}: cp {e_cp:.2e} cir {e_cir:.2e} (bound {TOL[prec]:g})")
    assert e_cp < TOL[prec] and e_cir < TOL[prec]
    assert torch.equal(cir, fitb)            # FITB dispatches to the same forward (outfit_x.py:87)


@pytest.mark.parametrize("B", [1, 32, 256, 1024])
def test_every_gemm_kernel_of_the_dispatcher_vs_float64(model, B):
    """The (M -> kernel) table of the module docstring, CP and CIR, every operand scheme."""
    CP, CIR, _ = tasks()
    emb, mask, txt = batch(B, (16,) if B == 1 else None)
    sub, want_cp, want_cir = oracle(B, (16,) if B == 1 else None)
    e, m, t = cu(emb), cu(mask), cu(txt)
    for prec, tol in TOL.items():
        cp = run(model, CP, prec, outfit_embedding=e, outfit_mask=m).cpu().numpy()
        cir = run(model, CIR, prec, outfit_embedding=e, outfit_mask=m, target_item_text_embedding=t).cpu().numpy()
        e_cp, e_cir = WS.rel_err(cp[sub], want_cp), WS.rel_err(cir[sub], want_cir)
        print(f"PARITY d1536 2 layers B={B} {prec}: cp {e_cp:.2e} cir {e_cir:.2e} (bound {tol:g})")
        assert e_cp < tol and e_cir < tol, (prec, e_cp, e_cir)


def test_six_layers_as_the_reference_builds_it():
    CP, CIR, _ = tasks()
    six = build("slip", D, 6)
    emb, mask, txt = batch(6, tuple(LENS6))
    _, want_cp, want_cir = oracle(6, tuple(LENS6), 6)
    cp = run(six, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask)).cpu().numpy()
    cir = run(six, CIR, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(txt)).cpu().numpy()
    e_cp, e_cir = WS.rel_err(cp, want_cp), WS.rel_err(cir, want_cir)
    print(f"PARITY d1536 6 layers B=6 ragged bf16x3: cp {e_cp:.2e} cir {e_cir:.2e}")
    assert e_cp < 1e-3 and e_cir < 1e-3


# ------------------------------------------------------------------------------------------------ properties, bit for bit
def test_pad_rows_are_inert_and_batches_permute(model):
    CP = tasks()[0]
    emb, mask, _ = batch(32)
    a = run(model, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask))
    emb2 = emb.copy(); emb2[mask] = 1e6                         # garbage in padded rows
    b = run(model, CP, outfit_embedding=cu(emb2), outfit_mask=cu(mask))
    emb3 = np.concatenate([emb2[:, 8:], emb2[:, :8]], 1); mask3 = np.concatenate([mask[:, 8:], mask[:, :8]], 1)       # padding wherever it sits
    c = run(model, CP, outfit_embedding=cu(emb3), outfit_mask=cu(mask3))
    assert torch.equal(a, b)
    assert WS.rel_err(c.cpu().numpy(), WS.cp_forward(emb3, mask3, weights(D, 2), n_layers=2)) < 1e-3
    perm = np.random.default_rng(0).permutation(32)
    shuf = run(model, CP, outfit_embedding=cu(emb[perm]), outfit_mask=cu(mask[perm]))
    assert torch.equal(a[torch.from_numpy(perm).cuda()], shuf)


def indexed_batch(seed, n_items, n_table=300):
    g = np.random.default_rng(seed)
    table = synth.item_embeddings(seed, "table", n_table, d_model=D)
    idx = [g.integers(0, n_table, n) for n in n_items]
    cus = np.concatenate([[0], np.cumsum(n_items)]).astype(np.int32)
    emb = np.zeros((len(n_items), 16, D), np.float32); mask = np.ones((len(n_items), 16), bool)
    for b, r in enumerate(idx):
        emb[b, :len(r)] = table[r]; mask[b, :len(r)] = False
    return table, torch.from_numpy(np.concatenate(idx).astype(np.int32)), torch.from_numpy(cus), emb, mask


def test_index_form_equals_padded_form_and_fitb_equals_cir(model):
    CP, CIR, FITB = tasks()
    n_items = [3, 16, 0, 1, 9, 16, 2, 7]
    table, idx, cus, emb, mask = indexed_batch(31, n_items)
    txt = synth.unit_rows(31, "target_text", len(n_items), D // 2)
    model.set_embedding_table(torch.from_numpy(table))
    a = run(model, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask))
    b = run(model, CP, item_index=idx, cu_seqlens=cus)
    c = run(model, CIR, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(txt))
    d = run(model, FITB, item_index=idx.cuda(), cu_seqlens=cus.cuda(), target_item_text_embedding=cu(txt), max_len=16)
    assert torch.equal(a, b) and torch.equal(c, d)
    tgt = torch.tensor([5, 0, 299, 7, 7, 12, 100, 3], dtype=torch.int32)
    e = run(model, CIR, item_index=idx, cu_seqlens=cus, target_item_index=tgt)
    f = run(model, CIR, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(table[tgt.numpy(), D // 2:]))
    assert torch.equal(e, f)


def test_small_batch_split_k_consumers_match_the_separate_passes(model):
    """ofx_tune(10, v) as tests/test_gpu_model.py has it at 1024: bit 0 (the set attention sums the q | k | v slabs) changes no bit; bit 1
    (reduce + LayerNorm in one launch, block-wide sums) is equal to fp32 rounding at bf16x3's 2^-16 floor."""
    from outfitx_amd import _lib as L
    lib = L.load()
    CP, CIR, _ = tasks()
    for B, lens in ((6, tuple(LENS6)), (1, (7,))):
        emb, mask, txt = batch(B, lens)
        out = {}
        try:
            for v in (3, 1, 0):
                lib.ofx_tune(10, v)
                out[v] = (run(model, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask)).cpu().numpy(),
                          run(model, CIR, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(txt)).cpu().numpy())
        finally:
            lib.ofx_tune(10, 3)
        assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1]), B
        assert WS.rel_err(out[3][0], out[0][0]) < 2e-5 and WS.rel_err(out[3][1], out[0][1]) < 2e-5, B


# ------------------------------------------------------------------------------------------------ retrieval on 1536-wide rows
def f32_sqrt(d2):
    return np.sqrt(np.asarray(d2, np.float64)).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_retrieval_is_exact_on_the_lattice_at_1536(model):
    from outfitx_amd.engine import fitb_argmin, fitb_argmin_indexed
    eng = model._engine()
    Q, P = O.lattice(1536, 8, D, -4, 4), O.lattice(1537, 640, D, -4, 4)
    k = 50
    idx, dist = eng.l2_topk(cu(Q), cu(P), k)
    ei, ed2 = O.l2_topk_exact(Q, P, k)
    assert np.array_equal(idx.cpu().numpy(), ei) and same_bits(dist.cpu().numpy(), f32_sqrt(ed2))
    off = [0, 100, 320, 640]                                    # 3 groups
    grp = [0, 1, 2, 2, 1, 0, 1, 2]
    gidx, gdist, _ = eng.l2_topk_grouped(cu(Q), grp, cu(P), off, k)
    for i, g in enumerate(grp):
        wi, wd2 = O.l2_topk_exact(Q[i:i + 1], P[off[g]:off[g + 1]], k, off[g])
        assert np.array_equal(gidx[i].cpu().numpy(), wi[0]) and same_bits(gdist[i].cpu().numpy(), f32_sqrt(wd2[0])), i
    y, table = O.lattice(1538, 9, D, -4, 4), O.lattice(1539, 60, D, -4, 4)
    ci = np.random.default_rng(5).integers(0, 60, (9, 4))
    ci[0, 3] = ci[0, 0]                                         # a duplicate: the first wins
    table[ci[1, 2]] = y[1]                                      # an exact hit
    cand = table[ci]
    wi, wd2 = O.fitb_argmin_exact(y, cand)
    i1, d1 = fitb_argmin(cu(y), cu(cand), return_dist=True)
    i2, d2 = fitb_argmin_indexed(cu(table), torch.from_numpy(ci.astype(np.int32)), cu(y), return_dist=True)
    for i_, d_ in ((i1, d1), (i2, d2)):
        assert np.array_equal(i_.cpu().numpy(), wi) and same_bits(d_.cpu().numpy(), f32_sqrt(wd2))


def test_fitb_evaluator_at_1536(model):
    from outfitx_amd.engine import fitb_argmin
    from outfitx_amd.trainer import FITBEvaluator
    FITB = tasks()[2]
    n_items = [3, 16, 1, 9, 2, 7]
    table, idx, cus, emb, mask = indexed_batch(77, n_items)
    B = len(n_items)
    g = np.random.default_rng(3)
    tgt = torch.from_numpy(g.integers(0, 300, B).astype(np.int32))
    ci = torch.from_numpy(g.integers(0, 300, (B, 4)).astype(np.int32))
    ans = torch.from_numpy(g.integers(0, 4, B).astype(np.int64))
    model.set_embedding_table(torch.from_numpy(table))
    y = run(model, FITB, item_index=idx, cu_seqlens=cus, target_item_index=tgt)
    want = fitb_argmin(y, cu(table)[ci.cuda().long()]).cpu()
    b = {"input_dict": {"task": FITB, "item_index": idx, "cu_seqlens": cus, "target_item_index": tgt}, "candidate_item_index": ci, "answer_index": ans}
    acc = FITBEvaluator(model).test_epoch([b, b])["Accuracy"]
    assert acc == float((want == ans).sum()) / B


# ------------------------------------------------------------------------------------------------ two widths in one process; training
def test_a_1024_model_keeps_its_bits_beside_a_1536_model(model):
    CP, CIR, _ = tasks()
    narrow = build("clip", 1024, 2)
    emb, mask = synth.outfit_batch(21, 6, 16, LENS6)
    txt = synth.unit_rows(21, "t", 6, 512)
    wemb, wmask, wtxt = batch(6, tuple(LENS6))
    first = run(narrow, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask))
    first_cir = run(narrow, CIR, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(txt))
    assert WS.rel_err(first.cpu().numpy(), WS.cp_forward(emb, mask, weights(1024, 2), n_layers=2)) < 1e-3
    wide_first = run(model, CP, outfit_embedding=cu(wemb), outfit_mask=cu(wmask))
    for _ in range(2):
        run(model, CIR, outfit_embedding=cu(wemb), outfit_mask=cu(wmask), target_item_text_embedding=cu(wtxt))
        assert torch.equal(run(narrow, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask)), first)
        assert torch.equal(run(model, CP, outfit_embedding=cu(wemb), outfit_mask=cu(wmask)), wide_first)
        assert torch.equal(run(narrow, CIR, outfit_embedding=cu(emb), outfit_mask=cu(mask), target_item_text_embedding=cu(txt)), first_cir)


def test_training_is_refused_and_scoring_goes_on(model):
    from outfitx_amd.trainer import CPTrainer
    CP = tasks()[0]
    emb, mask, _ = batch(6, tuple(LENS6))
    before = run(model, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask))
    engines = dict(model._engines)
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="training at d_model 1536"):
            model(task=CP, outfit_embedding=cu(emb), outfit_mask=cu(mask))
        with pytest.raises(NotImplementedError, match="training at d_model 1536"):
            CPTrainer(model, steps_per_epoch=4)
    finally:
        model.eval()
    assert dict(model._engines) == engines                       # no training engine was created: nothing was packed or launched
    assert torch.equal(run(model, CP, outfit_embedding=cu(emb), outfit_mask=cu(mask)), before)
    assert WS.rel_err(before.cpu().numpy(), oracle(6, tuple(LENS6))[1]) < 1e-3
