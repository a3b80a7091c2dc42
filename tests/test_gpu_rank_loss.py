"""Fused SetWiseRankingLoss (ofx_set_rank_loss, outfitx_amd/csrc/rank_loss.hip) and the CIR training loop built on it.

Reference for every comparison: `ref_rank_loss` below, a float64 numpy restatement of the reference's
src/losses/set_wise_ranking_loss.py:15-36 and of its gradient with respect to y_hat.  The restatement is itself held to the reference
on the committed fixture (tests/golden/train_step_cir.npz, written by the reference's own loss): first test, CPU, unmarked.

Tolerances (fp32 kernel vs float64): loss |d| <= 2e-5 |ref|; d_pos, d_neg 2e-5 relative; gradient max|d| / max|ref| <= 2e-5 over the
compared rows - 2e-5 is the project's fp32-vs-fixture bound (tests/test_oracle_golden.py).  The gradient is discontinuous where a hinge
crosses zero or two negatives tie for hardest, so a row is left out of the GRADIENT comparison (never of the loss) only if, in float64,
some valid |h_k| < 1e-4, or |h_hard| < 1e-4, or its two smallest valid distances differ by less than 1e-4 (about 100x the fp32
error of a distance near 6); at most 5 % of the rows may be left out.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from conftest import W_SEED, golden
from outfitx_amd import synth

warnings.simplefilter("ignore")
gpu = pytest.mark.gpu
TOL = 2e-5
NEAR = 1e-4
OFX_ESHAPE, OFX_EWORKSPACE = -2, -4


# ------------------------------------------------------------------------------------------------ float64 restatement
def ref_rank_loss(y, y_hat, neg, mask, margin, dtype=np.float64):
    """set_wise_ranking_loss.py:21-36 and d loss / d y_hat.  mask: True = padded.  Returns a dict: loss, grad [B,D], d_pos [B],
    d_neg [B,K] (+inf on padded entries), skip [B] (rows near a discontinuity of the gradient, see the module docstring)."""
    y, y_hat, neg = (np.asarray(a, dtype) for a in (y, y_hat, neg))
    margin = dtype(margin)
    B, D = y_hat.shape
    K = neg.shape[1]
    valid = ~np.asarray(mask, bool).reshape(B, K)
    pd = y_hat - y + dtype(1e-6)                                   # F.pairwise_distance adds eps to the difference
    d_pos = np.sqrt((pd * pd).sum(-1))
    nd = y_hat[:, None, :] - neg
    d_neg = np.sqrt((nd * nd).sum(-1))
    n_valid = dtype(max(int(valid.sum()), 1))
    h = d_pos[:, None] - d_neg + margin
    l_all = (np.maximum(h, 0) * valid).sum() / n_valid
    d_inf = np.where(valid, d_neg, np.inf)
    any_valid = valid.any(1)
    kstar = np.argmin(d_inf, axis=1) if K else np.zeros(B, np.int64)     # first index attaining the minimum
    hardest = d_inf[np.arange(B), kstar] if K else np.full(B, np.inf)
    h_hard = np.where(any_valid, d_pos - np.where(any_valid, hardest, 0) + margin, -np.inf)
    l_hard = np.maximum(h_hard, 0).sum() / dtype(B)
    with np.errstate(divide="ignore", invalid="ignore"):
        u_pos = np.where(d_pos[:, None] > 0, pd / d_pos[:, None], 0)       # a zero distance contributes a zero direction
        u_neg = np.where(d_neg[..., None] > 0, nd / d_neg[..., None], 0)
    w = ((h > 0) & valid).astype(dtype) / n_valid                          # relu'(0) = 0
    if K:
        w[np.arange(B), kstar] += (h_hard > 0).astype(dtype) / dtype(B)
    grad = w.sum(1)[:, None] * u_pos - (w[..., None] * u_neg).sum(1)
    skip = np.zeros(B, bool)
    if K:
        skip |= ((np.abs(h) < NEAR) & valid).any(1)
        skip |= np.abs(h_hard) < NEAR
        two = np.sort(d_inf, axis=1)[:, :2]
        if K > 1:
            skip |= np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] < NEAR)
    return {"loss": float(l_all + l_hard), "grad": grad, "d_pos": d_pos, "d_neg": d_inf, "skip": skip, "h": h, "valid": valid}


def inputs(seed, B, K, D=1024):
    """y, y_hat, neg as the CIR train test feeds them: item-encoder-shaped rows * 3."""
    y = synth.item_embeddings(seed, "pos", B)[:, :D] * 3.0
    y_hat = synth.item_embeddings(seed, "y_hat", B)[:, :D] * 3.0
    neg = synth.item_embeddings(seed, "neg", B * K).reshape(B, K, 1024)[:, :, :D] * 3.0
    return np.ascontiguousarray(y), np.ascontiguousarray(y_hat), np.ascontiguousarray(neg)


def make_mask(kind, seed, B, K):
    g = np.random.default_rng(seed)
    if kind == "none":
        return np.zeros((B, K), bool)
    if kind == "random":
        return g.random((B, K)) < 0.3
    if kind == "one_row":
        m = g.random((B, K)) < 0.3
        m[B // 2] = True
        return m
    assert kind == "all"
    return np.ones((B, K), bool)


def test_restatement_reproduces_the_reference_loss_of_the_cir_fixture():
    """CPU: the float64 restatement on the committed CIR train fixture's y_hat / neg_mask and the pos / neg inputs of
    tests/test_gpu_train.py::test_cir_train_step_vs_reference_golden gives the loss the REFERENCE computed, to 2e-5 relative."""
    g = golden("train_step_cir")
    seed, K, B = int(g["seed"]), int(g["K"]), len(g["n_items"])
    pos = synth.item_embeddings(seed, "pos", B) * 3.0
    neg = synth.item_embeddings(seed, "neg", B * K).reshape(B, K, 1024) * 3.0
    r = ref_rank_loss(pos, g["y_hat"], neg, g["neg_mask"], 2.0)
    print("fixture loss", float(g["loss"]), "restatement", r["loss"])
    assert abs(r["loss"] - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    # and its gradient is the derivative of its value: central differences in float64 along a few random directions
    gen = np.random.default_rng(0)
    yh = np.asarray(g["y_hat"], np.float64)
    for _ in range(3):
        v = gen.standard_normal(yh.shape)
        e = 1e-6
        num = (ref_rank_loss(pos, yh + e * v, neg, g["neg_mask"], 2.0)["loss"] - ref_rank_loss(pos, yh - e * v, neg, g["neg_mask"], 2.0)["loss"]) / (2 * e)
        assert abs(num - (r["grad"] * v).sum()) <= 1e-6 * max(abs(num), 1e-3)


# ------------------------------------------------------------------------------------------------ the C ABI
def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def abi_call(y, y_hat, neg, mask, margin, upstream=1.0, want_grad=True, want_d=True, ws_bytes=None, shape=None):
    """ofx_set_rank_loss on device copies of numpy inputs -> (rc, loss tensor, dy, d_pos, d_neg)."""
    from outfitx_amd import _lib as L
    lib = L.load()
    B, D = shape[0::2] if shape else y_hat.shape
    K = shape[1] if shape else neg.shape[1]
    ty, th = cu(y), cu(y_hat)
    tn = cu(neg) if neg is not None and neg.size else None
    tm = cu(np.asarray(mask, np.uint8)) if mask is not None and mask.size else None
    loss = torch.full((), float("nan"), device="cuda")
    dy = torch.full_like(th, float("nan")) if want_grad else None
    dp = torch.full((max(B, 1),), float("nan"), device="cuda") if want_d else None
    dn = torch.full((max(B, 1), max(K, 1)), float("nan"), device="cuda") if want_d else None
    n = lib.ofx_set_rank_loss_ws_bytes(B, K, D) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.ofx_set_rank_loss(p(ty), p(th), p(tn), p(tm), B, K, D, C.c_float(margin), C.c_float(upstream), p(loss), p(dy), p(dp), p(dn),
                               p(ws), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, loss, dy, dp, (dn[:, :K] if dn is not None else None)


def compare(tag, r, loss, dy, dp, dn, upstream=1.0):
    """Print every figure, then assert the module's bounds."""
    B = r["grad"].shape[0]
    e_loss = abs(float(loss) - r["loss"])
    keep = ~r["skip"]
    gref = r["grad"][keep] * upstream
    e_grad = float(np.abs(dy.cpu().numpy().astype(np.float64)[keep] - gref).max()) if keep.any() and gref.size else 0.0
    s_grad = float(np.abs(gref).max()) if gref.size else 0.0
    e_pos = float((np.abs(dp.cpu().numpy() - r["d_pos"]) / r["d_pos"]).max())
    fin = np.isfinite(r["d_neg"])
    got_dn = dn.cpu().numpy().astype(np.float64)
    e_neg = float((np.abs(got_dn[fin] - r["d_neg"][fin]) / np.maximum(r["d_neg"][fin], 1e-30)).max()) if fin.any() else 0.0
    active = float(((r["h"] > 0) & r["valid"]).sum() / max(r["valid"].sum(), 1))
    print(f"{tag}: loss {float(loss):.7g} ref {r['loss']:.7g} rel {e_loss / max(abs(r['loss']), 1e-30):.2e} | grad max|d|/max|ref| "
          f"{e_grad / max(s_grad, 1e-30):.2e} (max|ref| {s_grad:.3e}) | d_pos {e_pos:.2e} d_neg {e_neg:.2e} | rows left out {int(r['skip'].sum())}/{B} "
          f"| hinges active {active:.0%}")
    assert r["skip"].mean() <= 0.05, (tag, int(r["skip"].sum()), B)
    assert e_loss <= TOL * abs(r["loss"]), (tag, float(loss), r["loss"])
    assert e_pos <= TOL and e_neg <= TOL, (tag, e_pos, e_neg)
    assert np.array_equal(np.isinf(got_dn), ~fin), tag                        # padded entries read +inf, nothing else does
    assert torch.isfinite(dy).all(), tag
    assert e_grad <= TOL * s_grad, (tag, e_grad, s_grad)


# (B, K, D): K * D <= 10240 floats keeps the row's negatives in LDS (K <= 10 at D = 1024); (64, 40, 1024) and (32, 11, 1024) re-read them;
# (48, 40, 256) is LDS-resident with more than one 32-negative distance chunk
SHAPES = [(10, 6, 1024), (256, 10, 1024), (3072, 10, 1024), (64, 40, 1024), (32, 11, 1024), (48, 40, 256)]


@gpu
@pytest.mark.parametrize("B,K,D", SHAPES)
def test_op_parity_through_the_c_abi(B, K, D):
    need_gpu()
    y, y_hat, neg = inputs(40 + K, B, K, D)
    for margin in (2.0, 0.0):
        for kind in ("none", "random", "one_row", "all"):
            mask = make_mask(kind, B + K, B, K)
            r = ref_rank_loss(y, y_hat, neg, mask, margin)
            rc, loss, dy, dp, dn = abi_call(y, y_hat, neg, mask, margin)
            assert rc == 0
            compare(f"B{B} K{K} D{D} margin {margin} mask {kind}", r, loss, dy, dp, dn)
            if kind == "all":
                assert float(loss) == 0.0 and not dy.any()
            if kind == "one_row":
                assert not dy[B // 2].any()                                   # a row without a valid negative: zero gradient
    if D == 1024:
        # the two margins exercise different branches: every hinge is active at margin 2 on these inputs, about half at margin 0
        r2, r0 = ref_rank_loss(y, y_hat, neg, np.zeros((B, K), bool), 2.0), ref_rank_loss(y, y_hat, neg, np.zeros((B, K), bool), 0.0)
        assert (r2["h"] > 0).all() and 0.2 < (r0["h"] > 0).mean() < 0.8


def test_float32_numpy_evaluation_of_the_restatement_sits_inside_the_bound():
    """CPU.  What fp32 arithmetic alone costs: the same restatement evaluated in float32 numpy against float64 - printed so the kernel's
    figures can be read against it (numpy's pairwise sums; the kernel's lane -> wave -> LDS tree is comparable)."""
    B, K = 256, 10
    y, y_hat, neg = inputs(40 + K, B, K)
    for margin in (2.0, 0.0):
        mask = make_mask("random", B + K, B, K)
        r64, r32 = ref_rank_loss(y, y_hat, neg, mask, margin), ref_rank_loss(y, y_hat, neg, mask, margin, np.float32)
        keep = ~r64["skip"]
        eg = np.abs(r32["grad"][keep].astype(np.float64) - r64["grad"][keep]).max() / np.abs(r64["grad"][keep]).max()
        el = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
        print(f"float32 numpy vs float64, margin {margin}: loss rel {el:.2e}, grad max|d|/max|ref| {eg:.2e}")
        assert el <= TOL and eg <= TOL


@gpu
def test_edges_k0_zero_distance_upstream_null_grad_determinism_and_bad_shapes():
    need_gpu()
    B, K, D = 24, 7, 1024
    y, y_hat, neg = inputs(9, B, K)
    mask = make_mask("random", 9, B, K)
    mask[3, 2] = False
    # --- K = 0: both terms are 0, the gradient is 0
    rc, loss, dy, dp, _ = abi_call(y, y_hat, None, None, 2.0, shape=(B, 0, D))
    assert rc == 0 and float(loss) == 0.0 and not dy.any()
    assert np.abs(dp.cpu().numpy() - ref_rank_loss(y, y_hat, neg[:, :0], mask[:, :0], 2.0)["d_pos"]).max() <= TOL * 10
    # --- one negative EQUAL to y_hat: d_k = 0 exactly, hinge active, hardest; finite gradient with a zero direction for it
    neg0 = neg.copy()
    neg0[3, 2] = y_hat[3]
    for margin in (2.0, 0.0):
        r = ref_rank_loss(y, y_hat, neg0, mask, margin)
        rc, loss, dy, dp, dn = abi_call(y, y_hat, neg0, mask, margin)
        assert rc == 0 and float(dn[3, 2]) == 0.0 and r["d_neg"][3, 2] == 0.0
        compare(f"zero distance, margin {margin}", r, loss, dy, dp, dn)
        assert not r["skip"][3]
    # --- upstream scales the gradient, not the loss: a power of two exactly, any other value to rounding
    rc, loss1, dy1, _, _ = abi_call(y, y_hat, neg, mask, 2.0, 1.0)
    rc, loss4, dy4, _, _ = abi_call(y, y_hat, neg, mask, 2.0, 0.25)
    rc, loss3, dy3, _, _ = abi_call(y, y_hat, neg, mask, 2.0, 1.0 / 3.0)
    assert torch.equal(loss1, loss4) and torch.equal(dy4, dy1 * 0.25)
    assert torch.equal(loss1, loss3) and float((dy3 - dy1 / 3.0).abs().max()) <= 4e-7 * float(dy1.abs().max())
    # --- dy_hat = NULL (and no distances wanted): the same loss bits
    rc, loss_n, dy_n, dp_n, dn_n = abi_call(y, y_hat, neg, mask, 2.0, want_grad=False, want_d=False)
    assert rc == 0 and dy_n is None and torch.equal(loss_n, loss1)
    # --- two runs: bit-identical loss, gradient and distances (no floating-point atomics), on the large case too
    yb, hb, nb = inputs(50, 3072, 10)
    mb = make_mask("random", 1, 3072, 10)
    a, b = abi_call(yb, hb, nb, mb, 0.0), abi_call(yb, hb, nb, mb, 0.0)
    assert a[0] == 0 and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
    # --- a NULL mask means nothing is padded
    rc, loss_m, dy_m, _, _ = abi_call(y, y_hat, neg, None, 2.0)
    rc, loss_z, dy_z, _, _ = abi_call(y, y_hat, neg, np.zeros((B, K), bool), 2.0)
    assert torch.equal(loss_m, loss_z) and torch.equal(dy_m, dy_z)
    # --- bad shapes: OFX_ESHAPE with a message, nothing launched; short workspace: OFX_EWORKSPACE
    from outfitx_amd import _lib as L
    lib = L.load()
    for shape in ((B, K, 1022), (B, K, 4100), (B, K, 0), (0, K, D), (B, -1, D)):
        rc = abi_call(y, y_hat, neg, mask, 2.0, shape=shape, ws_bytes=1 << 20)[0]
        assert rc == OFX_ESHAPE and b"set_rank_loss" in lib.ofx_last_error(), shape
        assert lib.ofx_set_rank_loss_ws_bytes(*shape) == 0
    assert abi_call(y, y_hat, neg, mask, 2.0, ws_bytes=lib.ofx_set_rank_loss_ws_bytes(B, K, D) - 16)[0] == OFX_EWORKSPACE
    assert lib.ofx_set_rank_loss_ws_bytes(B, K, D) >= 16 + 8 * B + 4 * B * K


# ------------------------------------------------------------------------------------------------ the drop-in class
def torch_expression_f64(y, y_hat, neg, mask, margin):
    """set_wise_ranking_loss.py:21-36 in float64 torch on the CPU, with autograd -> (loss, d loss / d y_hat)."""
    import torch.nn.functional as F
    ty, tn, tm = torch.from_numpy(y).double(), torch.from_numpy(neg).double(), torch.from_numpy(mask)
    th = torch.from_numpy(y_hat).double().requires_grad_(True)
    pos_dist = F.pairwise_distance(th, ty)
    neg_dists = torch.norm(th.unsqueeze(1) - tn, dim=2)
    valid = (~tm).double()
    l_all = (F.relu(pos_dist.unsqueeze(1) - neg_dists + margin) * valid).sum() / valid.sum().clamp(min=1)
    hardest = neg_dists.masked_fill(tm, torch.inf).min(dim=1).values
    loss = l_all + F.relu(pos_dist - hardest + margin).mean()
    loss.backward()
    return float(loss), th.grad.numpy()


@gpu
@pytest.mark.parametrize("margin", [2.0, 0.0])
def test_drop_in_class_on_hip_tensors_matches_the_torch_expression_in_float64(margin):
    need_gpu()
    from src.losses import SetWiseRankingLoss
    B, K = 256, 10
    y, y_hat, neg = inputs(77, B, K)
    mask = make_mask("one_row", 77, B, K)
    r = ref_rank_loss(y, y_hat, neg, mask, margin)
    want_loss, want_grad = torch_expression_f64(y, y_hat, neg, mask, margin)
    assert abs(want_loss - r["loss"]) <= 1e-12 * abs(want_loss)            # the restatement and torch's float64 autograd agree
    keep = ~r["skip"]
    assert np.abs(want_grad[keep] - r["grad"][keep]).max() <= 1e-12
    th = cu(y_hat).requires_grad_(True)
    loss = SetWiseRankingLoss(margin=margin)(batch_y=cu(y), batch_y_hat=th, batch_negative_samples=cu(neg), batch_negative_mask=cu(mask))
    assert "SetRank" in type(loss.grad_fn).__name__, type(loss.grad_fn).__name__        # the kernel, not the eager expression
    (loss * 0.5).backward()
    e_loss = abs(float(loss) - want_loss) / abs(want_loss)
    e_grad = np.abs(th.grad.cpu().numpy()[keep] - 0.5 * want_grad[keep]).max() / np.abs(0.5 * want_grad[keep]).max()
    print(f"class, margin {margin}: loss rel {e_loss:.2e}, y_hat.grad max|d|/max|ref| {e_grad:.2e}, rows left out {int(r['skip'].sum())}/{B}")
    assert r["skip"].mean() <= 0.05 and e_loss <= TOL and e_grad <= TOL
    # no gradient wanted: value only
    with torch.no_grad():
        l2 = SetWiseRankingLoss(margin=margin)(cu(y), cu(y_hat), cu(neg), cu(mask))
    assert torch.equal(l2, loss.detach())


@gpu
def test_drop_in_class_keeps_the_eager_paths():
    need_gpu()
    from src.losses import SetWiseRankingLoss
    B, K = 16, 5
    y, y_hat, neg = inputs(78, B, K)
    mask = make_mask("random", 78, B, K)
    want_loss, _ = torch_expression_f64(y, y_hat, neg, mask, 2.0)
    fn = SetWiseRankingLoss(margin=2.0)
    # CPU tensors: the torch expression, gradients into everything
    th, tn = torch.from_numpy(y_hat).requires_grad_(True), torch.from_numpy(neg).requires_grad_(True)
    l_cpu = fn(torch.from_numpy(y), th, tn, torch.from_numpy(mask))
    assert "SetRank" not in type(l_cpu.grad_fn).__name__ and abs(float(l_cpu) - want_loss) <= TOL * abs(want_loss)
    l_cpu.backward()
    assert th.grad.abs().sum() > 0 and tn.grad.abs().sum() > 0
    # HIP tensors with a gradient wanted into the negatives (or the positives): still the eager expression, still a gradient there
    gh, gn, gy = cu(y_hat).requires_grad_(True), cu(neg).requires_grad_(True), cu(y).requires_grad_(True)
    l_neg = fn(cu(y), gh, gn, cu(mask))
    assert "SetRank" not in type(l_neg.grad_fn).__name__
    l_neg.backward()
    assert gn.grad is not None and gn.grad.abs().sum() > 0 and gh.grad.abs().sum() > 0
    l_pos = fn(gy, cu(y_hat), cu(neg), cu(mask))
    l_pos.backward()
    assert gy.grad is not None and gy.grad.abs().sum() > 0
    assert abs(float(l_neg) - want_loss) <= TOL * abs(want_loss) and abs(float(l_pos) - want_loss) <= TOL * abs(want_loss)
    # other dtypes: eager as well
    l_h = fn(cu(y).double(), cu(y_hat).double().requires_grad_(True), cu(neg).double(), cu(mask))
    assert l_h.dtype == torch.float64 and abs(float(l_h) - want_loss) <= 1e-9 * abs(want_loss)
    # engine.set_rank_loss refuses CPU tensors (the kernel has no CPU form)
    from outfitx_amd import _lib as L
    from outfitx_amd.engine import set_rank_loss
    with pytest.raises(L.OfxError):
        set_rank_loss(torch.from_numpy(y), torch.from_numpy(y_hat), torch.from_numpy(neg), torch.from_numpy(mask), 2.0)
    loss_e, dy_e = set_rank_loss(cu(y), cu(y_hat), cu(neg), cu(mask), 2.0, upstream=2.0)
    l_ref, dy_ref = set_rank_loss(cu(y), cu(y_hat), cu(neg), cu(mask), 2.0, need_grad=True)
    assert torch.equal(loss_e, l_ref) and torch.equal(dy_e, dy_ref * 2.0) and set_rank_loss(cu(y), cu(y_hat), cu(neg), cu(mask), 2.0, need_grad=False)[1] is None


# ------------------------------------------------------------------------------------------------ the training loop
def make_model(train_precision):
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    cfg.transformer.dropout = 0.0
    m = OutfitX(cfg, train_precision=train_precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.full_state_dict(W_SEED).items()}, strict=True)
    return m.cuda().train()


def trainable(m):
    return {k: v for k, v in m.named_parameters() if not k.startswith("item_encoder.")}


@gpu
@pytest.mark.parametrize("prec,ltol", [("f16", 2e-3), ("bf16", 1e-2)])
def test_cir_trainer_equals_the_reference_loop_written_out_by_hand(prec, ltol):
    """CIRTrainer (accumulation 2, 4 micro-batches of the train_step_cir problem, dropout 0) against
    complementary_item_retrieval_trainer.py:66-100 written out: model call, SetWiseRankingLoss, / accumulation, backward,
    clip_grad_norm_(1.0), AdamW, zero_grad, OneCycleLR.  Both sides run the same model arithmetic in `prec`; they differ in how the
    gradients are kept (arena + gradient sink vs autograd accumulation), clipped (one norm vs per-tensor norms) and stepped (fused vs
    foreach AdamW).  Bound on the parameters after the two optimizer steps: the one tests/test_gpu_train.py::
    test_cp_train_step_vs_reference_golden puts on post-AdamW weights for both precisions - AdamW's first steps move every weight by about
    lr * sign(g), so compare the UPDATE: at most 1 % of a tensor's elements may differ by more than 0.1 * lr.  ltol = that file's CIR step
    tolerance on the loss against the fixture."""
    need_gpu()
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    from src.losses import SetWiseRankingLoss
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    g = golden("train_step_cir")
    n, seed, K = g["n_items"], int(g["seed"]), int(g["K"])
    B = len(n)
    batches = []
    for i in range(4):
        emb, mask = synth.outfit_batch(seed + i, B, 16, n)
        batches.append({"input_dict": {"task": CIR, "outfit_embedding": torch.from_numpy(emb), "outfit_mask": torch.from_numpy(mask),
                                       "target_item_text_embedding": torch.from_numpy(synth.unit_rows(seed + i, "target_text", B, 512))},
                        "pos_item_embedding": torch.from_numpy(synth.item_embeddings(seed + i, "pos", B) * 3.0),
                        "neg_items_embedding": torch.from_numpy(synth.item_embeddings(seed + i, "neg", B * K).reshape(B, K, 1024) * 3.0),
                        "neg_items_mask": torch.from_numpy(g["neg_mask"])})
    LR, ACC = 2e-5, 2
    # ---- the trainer
    m = make_model(prec)
    before = {k: v.detach().clone() for k, v in trainable(m).items()}
    on_path = [p for p in CIRTrainer._default_params(m) if any(p is q for q in trainable(m).values())]
    assert len(on_path) == len(trainable(m)) - 3                       # outfit_token, cp_ffn.1.weight, cp_ffn.1.bias are left out
    tr = CIRTrainer(m, steps_per_epoch=4, cfg=CIRTrainConfig(learning_rate=LR, accumulation_steps=ACC, n_epochs=1), params=on_path)
    assert tr.cfg.margin == 2.0 and tr.layer_slices is not None and len(tr.layer_slices) == 6 and m.sink_ready("cir")
    losses = [float(tr.micro_step(b, i)[0]) for i, b in enumerate(batches)]
    got = {k: v.detach().clone() for k, v in trainable(m).items()}
    # ---- the reference's loop by hand
    model = make_model(prec)
    params = list(trainable(model).values())
    optimizer = torch.optim.AdamW(params, lr=LR)
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer=optimizer, max_lr=LR, epochs=1, steps_per_epoch=2, pct_start=0.3,
                                                    anneal_strategy="cos", div_factor=25, final_div_factor=1e4)
    loss_fn = SetWiseRankingLoss(margin=2.0)
    optimizer.zero_grad()
    want_losses = []
    for step, batch_dict in enumerate(batches):
        input_dict = {k: (v if k == "task" else v.to(0, non_blocking=True)) for k, v in batch_dict["input_dict"].items()}
        y_hats = model(**input_dict)
        loss = loss_fn(batch_y=batch_dict["pos_item_embedding"].to(0), batch_y_hat=y_hats,
                       batch_negative_samples=batch_dict["neg_items_embedding"].to(0), batch_negative_mask=batch_dict["neg_items_mask"].to(0))
        want_losses.append(float(loss.detach()))
        (loss / ACC).backward()
        if (step + 1) % ACC == 0 or step + 1 == len(batches):
            torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
            optimizer.step()
            optimizer.zero_grad()
            scheduler.step()
    want = {k: v.detach().clone() for k, v in trainable(model).items()}
    print(f"{prec}: losses {losses} by hand {want_losses} fixture {float(g['loss'])}")
    assert abs(losses[0] - float(g["loss"])) <= ltol * abs(float(g["loss"]))
    assert losses[:2] == want_losses[:2]                                 # same weights, same kernels: the first window is bit-identical
    assert all(abs(a - b) <= ltol * abs(b) for a, b in zip(losses, want_losses))
    assert abs(tr.scheduler.get_last_lr()[0] - scheduler.get_last_lr()[0]) < 1e-15
    worst = {}
    for k in want:
        du, dr = (got[k] - before[k]).cpu().numpy(), (want[k] - before[k]).cpu().numpy()
        if k in ("outfit_token", "cp_ffn.1.weight", "cp_ffn.1.bias"):
            assert not du.any() and not dr.any(), k                      # off the CIR path: never stepped, never decayed
            continue
        assert np.abs(dr).max() > 0, k
        worst[k] = (float(np.mean(np.abs(du - dr) > 0.1 * LR)), float(np.abs(du - dr).max()))
    bad = {k: v for k, v in worst.items() if not v[0] <= 0.01}
    print(f"{prec}: worst fraction of elements off by > 0.1 lr: {max(v[0] for v in worst.values()):.2e}; worst |du - dr| {max(v[1] for v in worst.values()):.2e} (lr {LR})")
    assert not bad, bad
