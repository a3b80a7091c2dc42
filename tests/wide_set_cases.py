"""Inputs and references of the wide outfit transformer - d_model 1536, 16 heads of 96, the reference's default (SigLIP) width - shared by
tests/test_cpu_wide_set.py, tests/test_gpu_wide_set_ops.py and tests/test_gpu_wide_model.py.  TEST INFRASTRUCTURE ONLY.

The oracles themselves are width-generic (oracle/attn_fwd.py: attn_fwd_ref / attn_fwd_f32 / attn_fwd_emul / f32_yard / block_err;
oracle/splitk_ops.py; oracle/np_oracle.py: outfit_encoder, lattice, l2_topk_exact, fitb_argmin_exact); only their input builders are 64
columns wide, and np_oracle.cir_forward hard-codes the 512-wide half.  So this module builds the inputs at heads of 96 exactly as
oracle/attn_fwd.py builds them at 64 (same seeds, same peaked sequence, same SET_LENS) and restates the two heads on top of
O._prefix + O.outfit_encoder with the width, depth and head count as arguments.  tests/test_cpu_wide_set.py pins both: bit for bit on
np_oracle at 1024, and on torch's own nn.TransformerEncoder in float64 at 1536.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import attn_fwd as A
from oracle import np_oracle as O

# ---- op level: 3 heads of 96, 7 sets (tests/test_gpu_attention_fwd.py's method at the other head width)
H, DH = 3, 96
W = H * DH                                                  # 288
NSEQ, PEAKED = A.NSEQ, A.PEAKED
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(DH)))    # 1 / sqrt(head_dim) as the library computes it: one float32 division
SET_LENS = A.SET_LENS                                       # every SMAX instance ships at heads of 96 too: 8, 20, 32, 64
MASK_LD = A.MASK_LD


def varlen_qkv(lens, seed=0):
    """-> cu_seqlens int32 [NSEQ + 1], fp32 [rows, 3 W] rows q | k | v, unit normal; sequence PEAKED has q x 4 (a peaked softmax)."""
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    g = np.random.default_rng(9600 + 17 * int(cu[-1]) + max(lens) + seed)
    qkv = g.standard_normal((int(cu[-1]), 3 * W), dtype=np.float32)
    qkv[cu[PEAKED]:cu[PEAKED + 1], :W] *= 4.0
    return cu, qkv


def fixed_qkv(S, seed=0):
    """fp32 [NSEQ * S, 3 W] rows q | k | v of the fixed-length mode; sequence PEAKED has q x 4."""
    g = np.random.default_rng(7600 + 131 * S + seed)
    qkv = g.standard_normal((NSEQ * S, 3 * W), dtype=np.float32)
    qkv[PEAKED * S:(PEAKED + 1) * S, :W] *= 4.0
    return qkv


def heads(a, S):
    """[NSEQ * S, W] -> [NSEQ, H, S, 96]."""
    return a.reshape(NSEQ, S, H, DH).transpose(0, 2, 1, 3)


def seq_heads(a, S):
    """[S, W] -> [H, S, 96]."""
    return a.reshape(S, H, DH).transpose(1, 0, 2)


@functools.lru_cache(maxsize=None)
def f32_yardsticks_varlen(max_len):
    """The fp32 kernel's yardsticks on the varlen sets of SET_LENS[max_len] -> per sequence (ref float64 [H, S, 96], {order: O float32})."""
    lens = SET_LENS[max_len]
    cu, qkv = varlen_qkv(lens)
    out = []
    for b, S in enumerate(lens):
        q, k, v = (seq_heads(qkv[cu[b]:cu[b + 1], i * W:(i + 1) * W], S) for i in range(3))
        out.append((A.attn_fwd_ref(q, k, v, None, SCALE), {o: A.attn_fwd_f32(q, k, v, None, SCALE, o) for o in A.ORDERS}))
    return out


def tail_mask(S):
    """One mask family of the fixed-length mode: per-sequence lengths that include 1 and S, and sequence 3 ignoring EVERY key (its query
    rows are fully masked: exactly zero by the library's rule).  -> key_mask int64 [NSEQ, MASK_LD] (columns >= S hold 1), dead bool
    [NSEQ, 1, S, S]."""
    g = np.random.default_rng(560 + S)
    m = np.ones((NSEQ, MASK_LD), np.int64)
    lens = g.integers(1, S + 1, NSEQ)
    lens[0], lens[1] = 1, S
    for b in range(NSEQ):
        m[b, lens[b]:S] = 0
    m[3, :S] = 0
    dead = np.zeros((NSEQ, 1, S, S), bool) | (m[:, None, None, :S] == 0)
    return m, dead


def quad_scores(q, k):
    """The kernel's own feature order, held out of A.ORDERS: features in blocks of four, t = x0 y0 + x1 y1 + x2 y2 + x3 y3; d += t, 24
    blocks at heads of 96 (all float32, nothing fused)."""
    x, y = q[..., :, None, :], k[..., None, :, :]
    d = np.zeros(np.broadcast_shapes(x.shape, y.shape)[:-1], np.float32)
    for c in range(0, q.shape[-1], 4):
        t = x[..., c] * y[..., c]
        for e in (1, 2, 3):
            t = t + x[..., c + e] * y[..., c + e]
        d += t
    return d


# ---- model level: the heads of the reference's OutfitX (outfit_x.py:120-172) at any width
D_WIDE, N_HEAD = 1536, 16


def cp_forward(emb, mask, Wt, dt=np.float64, n_layers=6, n_head=N_HEAD):
    """[outfit_token ; items] -> encoder -> row 0 -> Linear(D, 1): np_oracle.cp_forward with the depth and head count as arguments."""
    x, pad = O._prefix(Wt["outfit_token"].astype(dt), emb.astype(dt), mask)
    y = O.outfit_encoder(x, pad, Wt, dt, n_layers=n_layers, n_head=n_head)[:, 0]
    return y @ Wt["cp_ffn.1.weight"].astype(dt).T + Wt["cp_ffn.1.bias"].astype(dt)


def cir_forward(emb, mask, txt, Wt, dt=np.float64, n_layers=6, n_head=N_HEAD):
    """prefix = [target_item_image_emb | target text] per outfit -> encoder -> row 0 -> Linear(D, D, bias=False)."""
    img = np.broadcast_to(Wt["target_item_image_emb"].astype(dt), (len(emb), Wt["target_item_image_emb"].shape[0]))
    x, pad = O._prefix(np.concatenate([img, txt.astype(dt)], -1), emb.astype(dt), mask)
    y = O.outfit_encoder(x, pad, Wt, dt, n_layers=n_layers, n_head=n_head)[:, 0]
    return y @ Wt["cir_ffn.0.weight"].astype(dt).T


def rel_err(a, b):
    """max|a - b| / max|b| over the batch: the project's tolerance metric."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
