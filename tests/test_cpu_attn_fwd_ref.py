"""The references of the scoring path's attention forward (oracle/attn_fwd.py) and of the split-K consumers (oracle/splitk_ops.py),
pinned on the CPU.  tests/test_gpu_attention_fwd.py holds the kernels to them block by block; here
  - attn_fwd_ref is float64 torch scaled_dot_product_attention on every mask family of the GPU tests, and zero on a fully masked row;
  - attn_fwd_emul without roundings is the reference;
  - the float32 yardstick set of the fp32 kernel (A.ORDERS) covers a summation order that is NOT in the set - features in blocks of
    four, t = x0 y0 + x1 y1 + x2 y2 + x3 y3; d += t - to 1.25 x per block, on the GPU test's own inputs: the factor 2 the GPU test allows
    the kernel rests on this.  With the first three orders (seq, rev, pair) one peaked block of a short tail mask read 1.53, so the set
    grew by two (halves, evenodd) - the factor did not; now worst 1.04 over every case below;
  - the derived LayerNorm bound holds for a float32 numpy LayerNorm of the GPU test's own rows."""
import numpy as np
import pytest
import torch

from oracle import attn_fwd as A
from oracle import splitk_ops as K

SPREAD = 1.25


def sdpa64(q, k, v, dead, scale):
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    mask = None if dead is None else ~torch.tensor(np.broadcast_to(dead, q.shape[:-1] + (q.shape[-2],)).copy())
    return torch.nn.functional.scaled_dot_product_attention(t(q), t(k), t(v), attn_mask=mask, scale=scale).numpy()


def fixed_case(S, family):
    qkv = A.fixed_qkv(S).astype(np.float64)
    mask, causal = A.key_mask(family, S)
    return tuple(A.heads(qkv[:, i * A.W:(i + 1) * A.W], S) for i in range(3)) + (A.dead_of(mask, causal, S),)


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("S", sorted(set(A.FIXED_S_MFMA + A.FIXED_S_F32)))
def test_ref_is_float64_sdpa_on_every_mask_family(S, family):
    q, k, v, dead = fixed_case(S, family)
    assert dead is None or not dead.all(-1).any(), "the families of sections A and D have no fully masked query"
    ref = A.attn_fwd_ref(q, k, v, dead, A.SCALE)
    want = sdpa64(q, k, v, dead, A.SCALE)
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.array_equal(A.attn_fwd_emul(q, k, v, dead, A.SCALE, None), ref)
    assert np.array_equal(A.attn_fwd_emul(q, k, v, dead, A.SCALE, None, split3=True), ref)


@pytest.mark.parametrize("S", [1, 2, 17, 50])
def test_a_fully_masked_row_is_zero_and_the_others_are_sdpa(S):
    qkv = A.fixed_qkv(S).astype(np.float64)
    q, k, v = (A.heads(qkv[:, i * A.W:(i + 1) * A.W], S) for i in range(3))
    for name, mask, causal in A.masked_row_cases(S):
        dead = np.broadcast_to(A.dead_of(mask, causal, S), (A.NSEQ, A.H, S, S))
        full = dead.all(-1)
        assert full.any() and (S == 1 or not full.all()), name
        ref = A.attn_fwd_ref(q, k, v, dead, A.SCALE)
        assert not ref[full].any(), name
        for dt in ("bf16", "f16"):
            for split3 in (False, True):
                assert not A.attn_fwd_emul(q, k, v, dead, A.SCALE, dt, split3=split3)[full].any()
        for order in A.ORDERS:
            assert not A.attn_fwd_f32(q, k, v, dead, A.SCALE, order)[full].any()
        if not full.all():
            open_ = dead & ~full[..., None]                 # sdpa on the same mask with the fully masked rows opened: compare the others
            want = sdpa64(q, k, v, open_, A.SCALE)
            assert np.abs(ref - want)[~full].max() <= 1e-12 * np.abs(want).max(), name


def test_emulation_rounds_where_it_says():
    """P to the operand type before P . v, then the output; split3 returns hi + lo, whose residual is the rounding of o - hi."""
    S = 17
    q, k, v, dead = fixed_case(S, "causal_holes")
    for dt, u in (("bf16", 2.0 ** -8), ("f16", 2.0 ** -11)):
        r = lambda a: A.round_to(a, dt)
        s = np.where(dead, -np.inf, q @ np.swapaxes(k, -1, -2) * A.SCALE)
        P = np.exp(s - s.max(-1, keepdims=True))
        P /= P.sum(-1, keepdims=True)
        o = r(P) @ v
        assert np.array_equal(A.attn_fwd_emul(q, k, v, dead, A.SCALE, dt), r(o))
        assert np.array_equal(A.attn_fwd_emul(q, k, v, dead, A.SCALE, dt, split3=True), r(o) + r(o - r(o)))
        assert np.array_equal(A.attn_fwd_emul(q, k, v, dead, A.SCALE, dt, round_p=False), r(P @ v))
        e1 = A.block_err(A.attn_fwd_emul(q, k, v, dead, A.SCALE, dt), P @ v)
        assert (e1 > 0.05 * u).all() and (e1 < u).all()


def quad_scores(q, k):
    """The held-out order: features in blocks of four, t = x0 y0 + x1 y1 + x2 y2 + x3 y3; d += t (all float32, nothing fused)."""
    x, y = q[..., :, None, :], k[..., None, :, :]
    d = np.zeros(np.broadcast_shapes(x.shape, y.shape)[:-1], np.float32)
    for c in range(0, q.shape[-1], 4):
        t = x[..., c] * y[..., c]
        for e in (1, 2, 3):
            t = t + x[..., c + e] * y[..., c + e]
        d += t
    return d


def spread_of(q, k, v, dead, ref, orders):
    held = A.attn_fwd_f32(q, k, v, dead, A.SCALE, quad_scores)
    return A.block_err(held, ref) / A.f32_yard(ref, orders)


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("S", A.FIXED_S_F32)
def test_the_f32_yardsticks_cover_a_held_out_order_fixed(S, family):
    ref, orders, dead = A.f32_yardsticks_fixed(S, family)
    qkv = A.fixed_qkv(S)
    q, k, v = (A.heads(qkv[:, i * A.W:(i + 1) * A.W], S) for i in range(3))
    ratio = spread_of(q, k, v, dead, ref, orders)
    print(f"SPREAD fixed S={S} {family}: worst {ratio.max():.3f} median {np.median(ratio):.3f}")
    assert (ratio <= SPREAD).all(), float(ratio.max())


@pytest.mark.parametrize("max_len", sorted(A.SET_LENS))
def test_the_f32_yardsticks_cover_a_held_out_order_varlen(max_len):
    lens = A.SET_LENS[max_len]
    cu, qkv = A.varlen_qkv(lens)
    worst = []
    for b, (S, (ref, orders)) in enumerate(zip(lens, A.f32_yardsticks_varlen(max_len))):
        q, k, v = (A.seq_heads(qkv[cu[b]:cu[b + 1], i * A.W:(i + 1) * A.W], S) for i in range(3))
        worst.append(spread_of(q, k, v, None, ref, orders).max())
    print(f"SPREAD varlen max_len={max_len}: worst {max(worst):.3f}")
    assert max(worst) <= SPREAD, worst


@pytest.mark.parametrize("S", [1, 17, 50])
def test_the_f32_yardsticks_cover_a_held_out_order_masked_rows(S):
    qkv = A.fixed_qkv(S)
    q, k, v = (A.heads(qkv[:, i * A.W:(i + 1) * A.W], S) for i in range(3))
    for name, _, _ in A.masked_row_cases(S):
        ref, orders, dead = A.f32_yardsticks_fixed(S, None, name)
        live = ref.any((-1, -2))
        ratio = spread_of(q, k, v, dead, ref, orders)[live]
        assert (ratio <= SPREAD).all(), (name, float(ratio.max()))


def test_slab_sum_is_order_sensitive_on_its_own_inputs():
    """The cancelling pairs make the stated order visible: two slabs swapped give other bits."""
    g = np.random.default_rng(5)
    s = K.cancelling_slabs(g, 5, (9, 192))
    a, b = K.slab_sum(s), K.slab_sum(s[[1, 0, 2, 3, 4]])
    c = K.slab_sum(s[[0, 1, 2, 4, 3]])
    assert a.dtype == np.float32 and np.array_equal(a, b) and not np.array_equal(a, c)       # s0 + s1 commutes; the later slabs do not
    assert np.abs(a.astype(np.float64) - s.astype(np.float64).sum(0)).max() < 1e-2


@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("splits", [1, 2, 16])
def test_ln_bound_holds_for_a_float32_layernorm_of_the_same_rows(D, splits):
    slabs, bias, resid, gamma, beta = K.ln_inputs(D, splits)
    worst = 0.0
    for b in (None, bias):
        for r in (None, resid):
            x = K.slab_sum(slabs, b, r)
            ref, y32 = K.ln_ref(x, gamma, beta, 1e-5), K.ln_f32(x, gamma, beta, 1e-5)
            bound = K.ln_bound(x, gamma, beta, 1e-5)
            e = np.abs(y32.astype(np.float64) - ref)
            worst = max(worst, float((e / bound).max()))
            assert (e <= bound).all()
            for dt in ("bf16", "f16"):
                hi = A.round_to(y32, dt)
                assert (np.abs(hi - ref) <= K.ln_bound(x, gamma, beta, 1e-5, (dt, 1))).all()
                hilo = hi + A.round_to(y32.astype(np.float64) - hi, dt)
                assert (np.abs(hilo - ref) <= K.ln_bound(x, gamma, beta, 1e-5, (dt, 2))).all()
    print(f"LN float32 numpy D={D} splits={splits}: worst err / bound {worst:.3f}")
    assert worst > 1e-3, "a bound a thousand times the float32 error would hold nothing"
