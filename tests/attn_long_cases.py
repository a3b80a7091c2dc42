"""Inputs, masks and mutants for the MFMA attention over 65 .. 256 rows (attention_mfma_long_kernel) - TEST INFRASTRUCTURE ONLY.

The method is oracle/attn_fwd.py's: 7 sequences x 3 heads (one workgroup per pair here), unit-normal q | k | v from A.fixed_qkv,
sequence 2 with q x 4 (a peaked softmax), the five mask families.  What differs is the lengths and a mask row of its own width,
MASK_LD = 264 > 256, whose columns >= S hold 1: a kernel that trusted the mask there would let keys past the sequence in.

  S     why
  65    first length past the single-tile kernel: 5 live key tiles, one live row in the last
  80,81 a key-tile edge
  128   every wave has exactly two query tiles; the 8-key-tile instance full
  129   a ninth tile; first length of the 13-key-tile instance
  196   the SigLIP B/16 grid
  197   the CLIP B/16 grid (13 tiles, 5 live rows in the last; 7 k-steps, half a k-step of zero rows)
  241   16 tiles, one live row in the last; the 16-key-tile instance
  256   the limit

"none" runs at every S, the masked families at MASKED_S.  tests/test_cpu_attention_long.py pins these inputs and shows them sharp
against the mutants below; tests/test_gpu_attention_long.py runs the kernel on them.
"""
from __future__ import annotations

import numpy as np

from oracle import attn_fwd as A
from oracle.attn_train import round_to

H, DH, W, NSEQ, SCALE = A.H, A.DH, A.W, A.NSEQ, A.SCALE
MASK_LD = 264
LENGTHS = (65, 80, 81, 128, 129, 196, 197, 241, 256)
MASKED_S = (65, 129, 197, 256)
FAMILIES = A.FAMILIES
CASES = [(S, f) for S in LENGTHS for f in FAMILIES if f == "none" or S in MASKED_S]
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
F_OP = 1.6                                  # the project's factor for the MFMA wave core (tests/test_gpu_attention_fwd.py)


def qkv(S):
    """fp32 [NSEQ * S, 3 W] rows q | k | v (A.fixed_qkv: seeded by S, sequence 2 with q x 4)."""
    return A.fixed_qkv(S)


def key_mask(family, S):
    """A.key_mask's families at MASK_LD = 264 -> (int64 [NSEQ, MASK_LD] or None, causal).  'tail': per-sequence lengths that include 1
    and S; 'holes': a random third of the keys ignored, key 0 kept (no query is fully masked, under the causal mask either)."""
    causal = 1 if family in ("causal", "causal_holes") else 0
    if family in ("none", "causal"):
        return None, causal
    g = np.random.default_rng(40500 + S + (0 if family == "tail" else 1000))
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
    """Masks with fully masked query rows -> [(name, key_mask, causal)].  'key0': causal with key 0 ignored in every sequence (query 0
    alone is fully masked) and holes behind it; 'allzero': sequence 3 ignores every key, the others have a tail mask."""
    g = np.random.default_rng(40800 + S)
    a = np.ones((NSEQ, MASK_LD), np.int64)
    a[:, :S] = g.random((NSEQ, S)) >= 0.25
    a[:, 0] = 0
    a[:, 1:2] = 1
    z = np.ones((NSEQ, MASK_LD), np.int64)
    for b, n in enumerate(g.integers(1, S + 1, NSEQ)):
        z[b, n:S] = 0
    z[3, :S] = 0
    return [("key0", a, 1), ("allzero", z, 0)]


def heads64(S, dt):
    """q, k, v of qkv(S) rounded to the operand type, float64 [NSEQ, H, S, 64] each."""
    x = round_to(qkv(S).astype(np.float64), dt)
    return tuple(A.heads(x[:, i * W:(i + 1) * W], S) for i in range(3))


# ------------------------------------------------------------------------------------------------ mutants of the emulation
MUTANTS = ("drop_last_tile", "swap_v_tiles", "max_first_64", "sum_first_64")


def emul_mutant(q, k, v, dead, scale, dtype, mutant):
    """A.attn_fwd_emul (P rounded to the operand type, the output rounded once) with one fault a multi-tile kernel can have:
      drop_last_tile   the last 16-key tile (keys >= 16 (ceil(S / 16) - 1)) never enters: a loop one tile short
      swap_v_tiles     the V rows of key tiles 0 and 1 exchanged: a wrong tile index on the P . V side only
      max_first_64     the row max taken over keys 0 .. 63 only (the single-tile kernel's extent).  softmax is invariant under the shift, so
                       with finite exponentials this fault CANNOT show in the output - on these inputs it moves nothing but the last bits
                       of float64 (the CPU test asserts exactly that, so nobody reads a pass as coverage of it)
      sum_first_64     the same fault on the other reduction: the row sum taken over keys 0 .. 63 only - that one is visible
    mutant None: the emulation itself."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    S = q.shape[-2]
    s = q @ np.swapaxes(k, -1, -2) * scale
    if dead is not None:
        s = np.where(dead, -np.inf, s)
    if mutant == "drop_last_tile":
        s = s.copy()
        s[..., 16 * ((S - 1) // 16):] = -np.inf
    m = (s[..., :64] if mutant == "max_first_64" else s).max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    e = np.exp(s - m)
    den = (e[..., :64] if mutant == "sum_first_64" else e).sum(-1, keepdims=True)
    P = np.divide(e, den, out=np.zeros_like(e), where=den > 0)
    if mutant == "swap_v_tiles":
        v = v.copy()
        v[..., 0:16, :], v[..., 16:32, :] = v[..., 16:32, :].copy(), v[..., 0:16, :].copy()
    return round_to(round_to(P, dtype) @ v, dtype)


def worst_ratio(got, ref, emul, dt):
    """max over the (sequence, head) blocks of e_got / max(e_emul, 1e-2 u): the GPU test's criterion, as a number."""
    yard = np.maximum(A.block_err(emul, ref), 1e-2 * U[dt])
    return float((A.block_err(got, ref) / yard).max())
