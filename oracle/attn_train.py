"""Float64 reference of the training step's attention, forward and backward - TEST INFRASTRUCTURE ONLY.

One (sequence, head) at a time, or any stack of them in leading axes: q, k, v, dO are [..., S, d], the dropout mask m is [..., S, S]
with entries 0 or 1 / (1 - p) (None = no dropout).  With P = softmax(q k^T * scale) over the keys, as nn.MultiheadAttention computes it
in train() mode (dropout on the attention probabilities):

    O  = (P . m) v
    dV = (P . m)^T dO
    dP = (dO v^T) . m
    dS = P . (dP - rowsum(P . dP)) * scale        (softmax backward on the UNdropped P, times d(scores)/d(q k^T))
    dQ = dS k          dK = dS^T q

attn_train_ref is that, in float64.  attn_train_emul is the same computation with the roundings the kernels state
(outfitx_amd/csrc/attention.hip: set_attention_bwd_mfma_kernel, csrc/attn_wave.h): dO rounded to the operand type, P . m and dS rounded to
the operand type before they enter a product, outputs rounded to the operand type - and everything between those points exact.  It is
the yardstick for the kernels' error: what remains between a kernel and the emulation is fp32 accumulation and the hardware exp2.
"""
from __future__ import annotations

import numpy as np


def _t(a):
    return np.swapaxes(a, -1, -2)


def attn_train_ref(q, k, v, mask, dO, scale):
    """-> O, dQ, dK, dV (float64).  only_row0 is dO with zero rows behind row 0."""
    q, k, v, dO = (np.asarray(a, np.float64) for a in (q, k, v, dO))
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    s = q @ _t(k) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    P = e / e.sum(-1, keepdims=True)
    Pd = P * m
    O = Pd @ v
    dV = _t(Pd) @ dO
    dP = (dO @ _t(v)) * m
    dS = P * (dP - (P * dP).sum(-1, keepdims=True)) * scale
    return O, dS @ k, _t(dS) @ q, dV


def round_to(a, dtype):
    """float64 -> nearest value of the operand type ('bf16' | 'f16'; None: unchanged) -> float64, by torch's conversion."""
    if dtype is None:
        return np.asarray(a, np.float64)
    import torch
    td = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    return torch.tensor(np.asarray(a, np.float64)).to(td).double().numpy()


def attn_train_emul(q, k, v, mask, dO, scale, dtype, mask_n=None):
    """attn_train_ref with the kernels' roundings (dtype None: none at all).  mask_n: the mask as the dK / dV side applies it - the MFMA
    backward recomputes the mask a second time in its [query][key] orientation, after the row statistics (max, sum, rowsum(P . dP)) were
    formed with `mask` in the [key][query] orientation; a correct kernel has mask_n == mask (the default)."""
    r = lambda a: round_to(a, dtype)
    q, k, v, dO = (np.asarray(a, np.float64) for a in (q, k, v, dO))
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    mn = m if mask_n is None else np.asarray(mask_n, np.float64)
    s = q @ _t(k) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    P = e / e.sum(-1, keepdims=True)
    O = r(r(P * m) @ v)
    g = r(dO)
    gv = g @ _t(v)
    dot = (P * (gv * m)).sum(-1, keepdims=True)
    dQ = r(r(P * (gv * m - dot) * scale) @ k)                 # [key][query] orientation of the MFMA backward
    dK = r(_t(r(P * (gv * mn - dot) * scale)) @ q)            # [query][key] orientation
    dV = r(_t(r(P * mn)) @ g)
    return O, dQ, dK, dV


def block_err(a, ref):
    """||a - ref|| / ||ref|| over the last two axes (one block = one (sequence, head, tensor)); 0 / 0 = 0, x / 0 = inf."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    num = np.sqrt(((a - ref) ** 2).sum((-1, -2)))
    den = np.sqrt((ref ** 2).sum((-1, -2)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(num == 0, 0.0, num / den)
