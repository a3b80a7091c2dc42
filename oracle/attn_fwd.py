"""Float64 reference of the scoring path's attention forward - TEST INFRASTRUCTURE ONLY (beside oracle/attn_train.py, whose round_to
and block_err it reuses).

One (sequence, head) at a time, or any stack of them in leading axes: q, k, v are [..., S, 64]; `dead` is [..., S, S] bool (or None),
dead[i, j] = key j is ignored by query i (causal mask, key-padding mask, or both).  With s = q k^T * scale:

    P[i, j] = exp(s[i, j]) / sum over the live keys of query i,   0 on dead keys;          O = P v

A query whose keys are ALL dead has P = 0 and so a zero output row: the library's own rule (include/ofx.h, ofx_attention), stated by
both kernels (csrc/attn_wave.h, csrc/attention.hip); HF's result for such a row depends on its version.

  attn_fwd_ref    that, in float64.
  attn_fwd_emul   the same with the MFMA kernel's stated roundings - P to the operand type before P . v, the output to the operand type
                  (split3: hi = r(o), lo = r(o - hi), returned as hi + lo) - and everything between them exact.  round_p = False keeps P
                  unrounded: the fp32 VALU kernel with an operand-type output.
  attn_fwd_f32    the same formula evaluated in np.float32 with explicit accumulation loops, in five summation orders (ORDERS).  It is
                  the yardstick of the fp32 kernel: the reference restated in float32, not the kernel's loop.  The set began with three
                  orders; a held-out order then exceeded 1.25 x their envelope on one peaked block of the tests' own inputs
                  (tests/test_cpu_attn_fwd_ref.py), so the set grew by two - the factor the kernel is held to did not.

The second half builds the seeded inputs and masks of tests/test_gpu_attention_fwd.py, so that tests/test_cpu_attn_fwd_ref.py can pin the
yardsticks on exactly those inputs without a GPU.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle.attn_train import block_err, round_to  # noqa: F401  (re-exported for the tests)


def _t(a):
    return np.swapaxes(a, -1, -2)


def _probs64(q, k, dead, scale):
    s = q @ _t(k) * scale
    if dead is not None:
        s = np.where(dead, -np.inf, s)
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.exp(s - m)
    den = e.sum(-1, keepdims=True)
    return np.divide(e, den, out=np.zeros_like(e), where=den > 0)


def attn_fwd_ref(q, k, v, dead, scale):
    """-> O float64 [..., S, 64]."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    return _probs64(q, k, dead, scale) @ v


def attn_fwd_emul(q, k, v, dead, scale, dtype, split3=False, round_p=True):
    """attn_fwd_ref with the kernels' roundings (dtype None: none at all)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    P = _probs64(q, k, dead, scale)
    o = (round_to(P, dtype) if round_p else P) @ v
    hi = round_to(o, dtype)
    return hi + round_to(o - hi, dtype) if split3 else hi


ORDERS = ("seq", "rev", "pair", "halves", "evenodd")


def _scores_f32(q, k, order):
    S, d = q.shape[-2], q.shape[-1]
    if order == "pair":
        return np.sum(q[..., :, None, :] * k[..., None, :, :], axis=-1, dtype=np.float32)
    groups = {"seq": [range(d)], "rev": [range(d - 1, -1, -1)], "halves": [range(d // 2), range(d // 2, d)],
              "evenodd": [list(range(0, d, 2)) + list(range(1, d, 2))]}[order]
    total = None
    for grp in groups:                      # one accumulator per group, the groups added in turn
        acc = np.zeros(q.shape[:-2] + (S, S), np.float32)
        for c in grp:
            acc += q[..., :, None, c] * k[..., None, :, c]
        total = acc if total is None else total + acc
    return total


def attn_fwd_f32(q, k, v, dead, scale, order):
    """The formula in np.float32, every product and sum rounded to float32.  order: 'seq' - features and keys ascending; 'rev' - both
    descending; 'pair' - numpy's pairwise sum over the features; 'halves' - features 0 .. 31 and 32 .. 63 in two accumulators, then added;
    'evenodd' - the even features, then the odd ones (the last three with keys ascending); or a callable (q, k) -> float32 scores [..., S, S]
    (tests/test_cpu_attn_fwd_ref.py holds one more order out with it).  -> O float32 [..., S, 64]."""
    q, k, v = (np.ascontiguousarray(a, np.float32) for a in (q, k, v))
    S = q.shape[-2]
    s = (order(q, k) if callable(order) else _scores_f32(q, k, order)) * np.float32(scale)
    assert s.dtype == np.float32
    if dead is not None:
        s = np.where(dead, np.float32(-np.inf), s)
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, np.float32(0))
    e = np.exp(s - m)
    keys = range(S - 1, -1, -1) if order == "rev" else range(S)
    den = np.zeros(s.shape[:-1] + (1,), np.float32)
    for j in keys:
        den += e[..., j:j + 1]
    p = e * np.divide(np.float32(1), den, out=np.zeros_like(den), where=den > 0)
    o = np.zeros(q.shape, np.float32)
    for j in keys:
        o += p[..., :, j:j + 1] * v[..., j:j + 1, :]
    assert o.dtype == np.float32
    return o


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
H, DH = 3, 64                    # 3 heads: with 7 sequences 21 (sequence, head) pairs - the last MFMA block has one live wave and three dead
W = H * DH
NSEQ = 7
SCALE = 0.125
MASK_LD = 77
PEAKED = 2                       # this sequence has q x 4: a peaked softmax
FAMILIES = ("none", "causal", "tail", "holes", "causal_holes")
FIXED_S_MFMA = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 50, 63, 64)       # both sides of every 16-row tile edge of NT = 1, 2, 4; the ViT's 50
FIXED_S_F32 = (1, 8, 9, 20, 21, 32, 33, 64)                             # both sides of every SMAX edge
SET_LENS = {8: [1, 7, 8, 3, 8, 2, 5], 20: [1, 19, 20, 9, 20, 12, 17], 32: [1, 31, 32, 21, 32, 2, 25], 64: [1, 63, 64, 33, 64, 48, 40]}
VARLEN_LENS = [1, 33, 64, 48, 49, 17, 63]


def fixed_qkv(S, seed=0):
    """fp32 [NSEQ * S, 3 W] rows q | k | v, unit normal; sequence PEAKED has q x 4."""
    g = np.random.default_rng(7000 + 131 * S + seed)
    qkv = g.standard_normal((NSEQ * S, 3 * W), dtype=np.float32)
    qkv[PEAKED * S:(PEAKED + 1) * S, :W] *= 4.0
    return qkv


def varlen_qkv(lens, seed=0):
    """-> cu_seqlens int32 [NSEQ + 1], fp32 [rows, 3 W]; sequence PEAKED has q x 4."""
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    g = np.random.default_rng(9000 + 17 * int(cu[-1]) + max(lens) + seed)
    qkv = g.standard_normal((int(cu[-1]), 3 * W), dtype=np.float32)
    qkv[cu[PEAKED]:cu[PEAKED + 1], :W] *= 4.0
    return cu, qkv


def key_mask(family, S):
    """-> (key_mask int64 [NSEQ, MASK_LD] or None, causal).  Columns >= S hold 1: a kernel that trusted the mask there would let keys of
    the next sequence in.  'tail': per-sequence lengths that include 1 and S; 'holes': a random third of the keys ignored, key 0 kept (so no
    query is fully masked, under the causal mask either)."""
    causal = 1 if family in ("causal", "causal_holes") else 0
    if family in ("none", "causal"):
        return None, causal
    g = np.random.default_rng(500 + S + (0 if family == "tail" else 1000))
    m = np.ones((NSEQ, MASK_LD), np.int64)
    if family == "tail":
        lens = g.integers(1, S + 1, NSEQ)
        lens[0], lens[1] = 1, S
        for b in range(NSEQ):
            m[b, lens[b]:S] = 0
    else:
        m[:, :S] = g.random((NSEQ, S)) >= 1.0 / 3.0
        m[:, 0] = 1
    return m, causal


def masked_row_cases(S):
    """Masks with fully masked query rows -> list of (name, key_mask, causal).  'key0': causal with key 0 ignored in every sequence (query 0
    alone is fully masked) and holes behind it; 'allzero': sequence 3 ignores every key, the others have a tail mask (S = 1: sequences 0,
    3 and 5 ignore their only key)."""
    g = np.random.default_rng(800 + S)
    a = np.ones((NSEQ, MASK_LD), np.int64)
    a[:, :S] = g.random((NSEQ, S)) >= 0.25
    a[:, 0] = 0
    a[:, 1:2] = 1                                       # S >= 2: query 1 sees key 1
    z = np.ones((NSEQ, MASK_LD), np.int64)
    for b, n in enumerate(g.integers(1, S + 1, NSEQ)):
        z[b, n:S] = 0
    z[[0, 3, 5] if S == 1 else [3], :S] = 0
    return [("key0", a, 1), ("allzero", z, 0)]


def dead_of(mask, causal, S):
    """-> bool [NSEQ, 1, S, S] (broadcasts over heads), or None."""
    if mask is None and not causal:
        return None
    dead = np.zeros((NSEQ, 1, S, S), bool)
    if causal:
        dead |= np.triu(np.ones((S, S), bool), 1)
    if mask is not None:
        dead |= (mask[:, None, None, :S] == 0)
    return dead


def heads(a, S):
    """[NSEQ * S, W] -> [NSEQ, H, S, 64]."""
    return a.reshape(NSEQ, S, H, DH).transpose(0, 2, 1, 3)


def seq_heads(a, S):
    """[S, W] -> [H, S, 64]."""
    return a.reshape(S, H, DH).transpose(1, 0, 2)


@functools.lru_cache(maxsize=None)
def f32_yardsticks_fixed(S, family, masked_case=None):
    """The fp32 kernel's yardsticks on the GPU test's own inputs -> (ref float64 [NSEQ, H, S, 64], {order: O float32}, dead)."""
    qkv = fixed_qkv(S)
    if masked_case is None:
        mask, causal = key_mask(family, S)
    else:
        mask, causal = next((m, c) for n, m, c in masked_row_cases(S) if n == masked_case)
    dead = dead_of(mask, causal, S)
    q, k, v = (heads(qkv[:, i * W:(i + 1) * W], S) for i in range(3))
    ref = attn_fwd_ref(q, k, v, dead, SCALE)
    return ref, {o: attn_fwd_f32(q, k, v, dead, SCALE, o) for o in ORDERS}, dead


@functools.lru_cache(maxsize=None)
def f32_yardsticks_varlen(max_len):
    """The same for the varlen sets of SET_LENS[max_len] -> per sequence (ref [H, S, 64], {order: O})."""
    lens = SET_LENS[max_len]
    cu, qkv = varlen_qkv(lens)
    out = []
    for b, S in enumerate(lens):
        q, k, v = (seq_heads(qkv[cu[b]:cu[b + 1], i * W:(i + 1) * W], S) for i in range(3))
        out.append((attn_fwd_ref(q, k, v, None, SCALE), {o: attn_fwd_f32(q, k, v, None, SCALE, o) for o in ORDERS}))
    return out


def f32_yard(ref, orders, floor=2.0 ** -26):
    """max over the yardstick orders of the per-block error, floored at 2^-26."""
    return np.maximum(np.max([block_err(o, ref) for o in orders.values()], axis=0), floor)
