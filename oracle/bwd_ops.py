"""Float64 references of the non-attention kernels of the training backward (outfitx_amd/csrc/backward.hip and the training
epilogue of the GEMMs) - TEST INFRASTRUCTURE ONLY.  Plain numpy; tests/test_cpu_bwd_ops_ref.py pins every function to float64 torch
autograd, tests/test_gpu_bwd_ops.py compares the kernels with them.

    ln_bwd_ref       LayerNorm backward FROM GIVEN (mean, rstd), the kernel's definition:
                         g = dy gamma, xh = (x - mean) rstd, dx = rstd (g - mean(g) - xh mean(g xh)) [+ add]
                         dgamma = sum_r dy xh, dbeta = sum_r dy, dcols = sum_r dx . mask
    ln_bwd_dx_emul   the dx formula step by step in np.float32, row sums by np.sum on float32: the yardstick of a correct fp32 kernel
    colsum_ref       out[c] = sum_r scale[r] x[gather[r]][c] and the terms of every sum
    head_bwd_ref     gradient of  logit_b = (row0_b . m_head) . w + bias  (CP)  or a ready row gradient (CIR), and the operand copy's mask
    mish_grad        d/du [u tanh(softplus(u))]
    drop_mask        the library's stateless dropout mask (csrc/ofx_common.h: drop_mul, make_drop), values 0 or fp32(1 / (1 - p))

The second half of the file is the case tables and the seeded inputs both test files use: the CPU file asserts from the references
alone that every sum case is SHARP (each row owns a column where its term exceeds 16 x that column's error bound, so a dropped or a
doubled row cannot hide inside the bound); the GPU file relies on it.
"""
from __future__ import annotations

import functools

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------- references
def ln_bwd_ref(dy, x, mean, rstd, gamma, add=None, add_map=None, mask=None):
    """-> dict(dx, dx_drop, dgamma, dbeta, dcols, t_dgamma, t_dbeta, t_dcols), float64.  dy, x [M, D]; mean, rstd [M]; gamma [D];
    add [M, D], or [B, D] with add_map [M] (< 0: no addend); mask [M, D] (None = no dropout).  dx_drop = dx . mask is what the operand
    copy holds and what dcols sums; t_* are the [M, D] terms of the three column sums."""
    dy, x, gamma = (np.asarray(a, np.float64) for a in (dy, x, gamma))
    mean, rstd = np.asarray(mean, np.float64)[:, None], np.asarray(rstd, np.float64)[:, None]
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdims=True) - xh * (g * xh).mean(-1, keepdims=True))
    if add is not None:
        dx = dx + gathered_add(add, add_map, dx.shape[0])
    dxd = dx if mask is None else dx * np.asarray(mask, np.float64)
    return dict(dx=dx, dx_drop=dxd, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), dcols=dxd.sum(0), t_dgamma=dy * xh, t_dbeta=dy, t_dcols=dxd)


def gathered_add(add, add_map, M):
    add = np.asarray(add, np.float64)
    if add_map is None:
        return add[:M]
    add_map = np.asarray(add_map)[:M]
    return np.where((add_map >= 0)[:, None], add[np.maximum(add_map, 0)], 0.0)


def ln_bwd_dx_emul(dy, x, mean, rstd, gamma, add=None, add_map=None):
    """The dx of ln_bwd_ref with every step in np.float32 (inputs are fp32 values already) -> float32 [M, D]."""
    f = np.float32
    dy, x, gamma = (np.asarray(a, f) for a in (dy, x, gamma))
    mean, rstd = np.asarray(mean, f)[:, None], np.asarray(rstd, f)[:, None]
    D = dy.shape[1]
    xh = (x - mean) * rstd
    g = dy * gamma
    m1 = np.sum(g, -1, dtype=f, keepdims=True) * (f(1.0) / f(D))
    m2 = np.sum(g * xh, -1, dtype=f, keepdims=True) * (f(1.0) / f(D))
    o = (g - m1 - xh * m2) * rstd
    if add is not None:
        o = o + gathered_add(add, add_map, o.shape[0]).astype(f)
    assert o.dtype == f
    return o


def colsum_ref(x, gather=None, row_scale=None):
    """-> (sums [C], terms [M, C]) float64: terms[r] = row_scale[r] * x[gather[r]] (M = len(gather) or len(x))."""
    x = np.asarray(x, np.float64)
    t = x if gather is None else x[np.asarray(gather)]
    if row_scale is not None:
        t = t * np.asarray(row_scale, np.float64)[:, None]
    return t.sum(0), t


def head_bwd_ref(dlogits, w, mask_head=None):
    """Row gradients of the head, float64 [B, D].  CP (dlogits [B], w [D]): logit_b = sum_c row0[b, c] m_head[b, c] w[c] + bias, so
    d row0[b] = dlogits[b] w . m_head[b] and d bias = sum_b dlogits[b].  CIR (dlogits None, w [B, D]): d row0[b] = w[b] . m_head[b].
    -> (d_row0, d_bias or None)."""
    w = np.asarray(w, np.float64)
    m = 1.0 if mask_head is None else np.asarray(mask_head, np.float64)
    if dlogits is None:
        return w * m, None
    dl = np.asarray(dlogits, np.float64)
    return dl[:, None] * w[None, :] * m, dl.sum()


def mish_grad(u):
    """d/du [u tanh(softplus(u))] = t + u sigmoid(u) (1 - t^2), float64, without the cancellation: with w = e^u, n = w (w + 2):
    t = n / (n + 2), 1 - t = 2 / (n + 2), 1 + t = (2 n + 2) / (n + 2).  |u| <= 300 (beyond, e^2u leaves float64): 1 above, 0 below."""
    u = np.asarray(u, np.float64)
    uc = np.clip(u, -300.0, 300.0)
    w = np.exp(uc)
    n = w * (w + 2.0)
    t = n / (n + 2.0)
    sech2 = (2.0 / (n + 2.0)) * ((2.0 * n + 2.0) / (n + 2.0))
    return np.where(u > 300.0, 1.0, np.where(u < -300.0, 0.0, t + uc * (w / (1.0 + w)) * sech2))


def mish(u):
    u = np.asarray(u, np.float64)
    return u * np.tanh(np.logaddexp(0.0, u))


def _fmix32(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def drop_mask(p, seed, site, rows, cols):
    """float32 [rows, cols]: element kept iff hash(seed, site, row, col) >= p 2^32 (p taken as fp32), kept = fp32(1 / (1 - p));
    `rows` may be a count or an array of row indices.  p = 0 or site None: ones."""
    r = np.arange(rows, dtype=np.uint32) if np.isscalar(rows) else np.asarray(rows).astype(np.uint32)
    if p == 0 or site is None or site < 0:
        return np.ones((len(r), cols), np.float32)
    p32 = np.float32(p)
    with np.errstate(over="ignore"):
        h = _fmix32(np.uint32(seed) + np.uint32(site) * np.uint32(0x9E3779B9) + r * np.uint32(0x632BE5AB))
        c = np.arange(cols, dtype=np.uint32)
        h = _fmix32(h[:, None] ^ (c[None, :] * np.uint32(0x9E3779B1) + np.uint32(0x7F4A7C15)))
    thresh = np.uint32(int(float(p32) * 4294967296.0))
    return np.where(h >= thresh, np.float32(1.0) / (np.float32(1.0) - p32), np.float32(0.0)).astype(np.float32)


def round_op(a, dt):
    """fp32 / float64 values -> nearest value of the operand type ('bf16' | 'f16'), as float32, by torch's conversion."""
    import torch
    td = {"bf16": torch.bfloat16, "f16": torch.float16}[dt]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(td).float().numpy()


def sum_bound(terms, h):
    """Per column: (h + 3) 2^-24 sum_r |terms[r]| - h dependent fp32 additions, each relative 2^-24 of a partial sum that is at most
    sum |terms| (to first order), plus up to 3 roundings inside a term."""
    return (h + 3) * U32 * np.abs(np.asarray(terms, np.float64)).sum(0)


def sharp(terms, bound):
    """Does every row own a column where |its term| > 16 x that column's bound?  terms [M, C], bound [C].  Columns may be restricted by
    passing slices of both."""
    t = np.abs(np.asarray(terms, np.float64))
    return bool((t > 16.0 * np.asarray(bound)[None, :]).any(1).all()) if t.shape[0] else True


# ---------------------------------------------------------------------------------------------------- cases and inputs
SEED = 0xC0FFEE


def unit_mag(g, shape):
    """magnitudes uniform in [0.5, 2) with random signs, fp32"""
    return (g.uniform(0.5, 2.0, shape) * g.choice([-1.0, 1.0], shape)).astype(np.float32)


# ---- LayerNorm backward.  id: (D, dtype, M static, live rows (None: no m_dev), add 'none' | 'full' | 'map', p, dcols given, accumulate)
LN_SITE = 7
LN_CASES = [
    (1024, "bf16", 1, None, "none", 0.0, True, 0),       # 255 idle blocks, three idle waves in block 0
    (1024, "f16", 5, None, "full", 0.1, True, 1),
    (1024, "bf16", 1024, None, "map", 0.1, True, 0),     # exactly one row per wave
    (1024, "f16", 1025, None, "none", 0.0, False, 0),    # wave 0 of block 0 takes two rows
    (1024, "bf16", 2500, 2309, "full", 0.1, True, 1),    # device count under the static M: 2 or 3 rows per wave
    (1024, "f16", 64, 0, "full", 0.1, True, 0),          # no live row: sums are zero, nothing else written
    (512, "bf16", 1025, None, "map", 0.1, True, 1),
    (512, "f16", 5, None, "none", 0.0, False, 0),
    (512, "f16", 2500, 2309, "full", 0.1, True, 0),
    (512, "bf16", 64, 0, "none", 0.0, True, 1),          # no live row + accumulate: the prefill stays
    (768, "bf16", 2500, 2309, "full", 0.0, True, 0),
    (768, "f16", 1024, None, "map", 0.1, True, 0),
    (768, "bf16", 1, None, "full", 0.1, False, 1),
]


def ln_live(case):
    return case[2] if case[3] is None else case[3]


def ln_h(case):
    """Longest chain of dependent fp32 additions behind one element of dgamma / dbeta / dcols, from ln_bwd_kernel + colsum_final_kernel:
    ceil(live / 1024) rows per wave, + 3 (waves 1..3 onto wave 0 in LDS), + 9 (strided pass over the 256 block partials: 16 per row
    group as two interleaved chains of 8, joined), + 15 (the 16 row groups, the first onto an exact zero)."""
    return -(-ln_live(case) // 1024) + 3 + 9 + 15


@functools.lru_cache(maxsize=None)
def ln_inputs(i):
    """fp32 inputs of LN_CASES[i] over the LIVE rows (numpy): dy, x, stats (float64 mean / rstd of x rounded to fp32), gamma, add,
    add_map, prefill [3, D].  dy has magnitudes in [0.5, 2): the sharpness of dbeta and dgamma."""
    D, dt, M, live, add_kind, p, dcols, acc = LN_CASES[i]
    n = ln_live(LN_CASES[i])
    g = np.random.default_rng(1000 + i)
    dy = unit_mag(g, (n, D))
    x = (3.0 * g.standard_normal((n, D)) + 1.5).astype(np.float32)
    x[::7] += np.float32(100.0)                                    # rows far from the origin: x - mean cancels
    x64 = x.astype(np.float64)
    mean = x64.mean(-1)
    rstd = 1.0 / np.sqrt(x64.var(-1) + 1e-5)
    stats = np.stack([mean, rstd], -1).astype(np.float32)
    gamma = (1.0 + 0.25 * g.standard_normal(D)).astype(np.float32)
    add = add_map = None
    if add_kind == "full":
        add = (0.3 * g.standard_normal((n, D))).astype(np.float32)
    elif add_kind == "map":
        B = min(n, 9)
        add = (0.3 * g.standard_normal((B, D))).astype(np.float32)
        add_map = np.full(n, -1, np.int32)
        add_map[np.sort(g.choice(n, B, replace=False))[g.permutation(B)]] = np.arange(B, dtype=np.int32)
    prefill = unit_mag(g, (3, D)) * np.float32(37.0)
    return dict(dy=dy, x=x, stats=stats, gamma=gamma, add=add, add_map=add_map, prefill=prefill)


def ln_reference(i, mask=None):
    """ln_bwd_ref of case i from the fp32 stats; mask: [live, D] (default: drop_mask of the case's site)."""
    D, dt, M, live, add_kind, p, dcols, acc = LN_CASES[i]
    inp = ln_inputs(i)
    n = ln_live(LN_CASES[i])
    if mask is None:
        mask = drop_mask(p, SEED, LN_SITE, n, D)
    return ln_bwd_ref(inp["dy"], inp["x"], inp["stats"][:, 0], inp["stats"][:, 1], inp["gamma"], inp["add"], inp["add_map"], mask)


# ---- column sums.  (kind 'f32' | 'bf16' | 'f16', C, ld, M static, live (None: no m_dev), gather, row_scale, outputs (tuple of 0/1 per
# segment; seg = C / len), valid (0 = seg), accumulate)
CS_CASES = [
    ("f32", 4, 4, 1, None, 0, 0, (1,), 0, 0),                 # nchunk 1, per 1: tail loop only
    ("f32", 1020, 1020, 15, None, 0, 0, (1,), 0, 0),          # per 15: three unrolled steps + tail 3; last block of the final pass partial
    ("bf16", 1024, 1024, 16, None, 0, 0, (1,), 0, 0),         # per 16: unrolled only
    ("f16", 1024, 1024, 17, None, 0, 1, (1,), 0, 0),          # nchunk 1, per 17
    ("f32", 2048, 2048, 31, None, 0, 0, (1,), 2024, 0),       # valid < seg, two column blocks
    ("bf16", 2048, 2048, 4100, None, 0, 0, (1,), 2024, 1),    # db1's form: nchunk 256 (the cap), per 17, last chunks short
    ("f32", 3072, 3072, 100, None, 0, 0, (1, 1, 1), 0, 0),    # three outputs, nchunk 6, per 17
    ("f16", 3072, 3072, 4095, None, 0, 0, (1, 0, 1), 0, 0),   # nchunk 255 (odd count in the strided pass), per 17; middle output NULL
    ("f32", 1020, 1020, 31, None, 0, 0, (1, 1, 1), 0, 1),     # seg 340: segment borders inside a 16-column block of the final pass
    ("f32", 512, 1024, 4096, None, 1, 0, (1,), 0, 1),         # ld > C, gathered rows, nchunk 256, per 16
    ("f32", 1024, 1024, 4096, 37, 0, 0, (1,), 0, 0),          # device count 37: per 1, 219 chunks start past it
    ("bf16", 1020, 1024, 4100, None, 1, 1, (1,), 0, 1),       # gather + scale on operand-type rows
    ("f32", 4, 4, 4100, None, 0, 1, (1,), 0, 0),
    ("f16", 512, 1024, 100, 0, 0, 0, (1,), 0, 0),             # device count 0: zeros
    ("f32", 1024, 1024, 4096, 0, 0, 0, (1,), 0, 1),           # device count 0 + accumulate: the prefill stays
    ("f32", 3072, 3072, 4100, 2311, 1, 1, (1, 1, 1), 1000, 0),
]


def cs_live(case):
    return case[3] if case[4] is None else case[4]


def cs_plan(case):
    """(nchunk, per) as ofx_launch_colsum and colsum_partial_kernel compute them"""
    M, live = case[3], cs_live(case)
    nchunk = min(max(M // 16, 1), 256)
    return nchunk, -(-live // nchunk)


def cs_h(case):
    """per (rows of a chunk, one chain; the unrolled loop adds its four rows in order) + the strided pass (ceil(nchunk / 16) partials
    per row group as two chains, + 1 to join them) + 15 (16 row groups, the first onto an exact zero)."""
    nchunk, per = cs_plan(case)
    ceil = lambda a, b: -(-a // b)
    return per + (ceil(ceil(nchunk, 16), 2) + 1) + 15


@functools.lru_cache(maxsize=None)
def cs_inputs(i):
    """table [T, ld] fp32 (already rounded to the operand type for bf16 / f16; T > live when gathered), gather [live] or None,
    row_scale [live] or None, prefill [3, seg]"""
    kind, C, ld, M, live, gather, scale, outs, valid, acc = CS_CASES[i]
    n = cs_live(CS_CASES[i])
    g = np.random.default_rng(2000 + i)
    T = 2 * n + 3 if gather else n
    table = unit_mag(g, (T, ld))
    if kind != "f32":
        table = round_op(table, kind)
    gi = g.permutation(T)[:n].astype(np.int32) if gather else None          # a non-monotone subset of the larger table
    sc = unit_mag(g, (n,)) if scale else None
    prefill = unit_mag(g, (3, C // len(outs))) * np.float32(1000.0)
    return dict(table=table, gather=gi, scale=sc, prefill=prefill)


def cs_reference(i):
    inp = cs_inputs(i)
    C = CS_CASES[i][1]
    return colsum_ref(inp["table"][:, :C], inp["gather"], inp["scale"])


# ---- the mish' sweep: [256, 256] finite fp32 arguments
def mish_grad_zero():
    """the zero of mish' (near -1.1924), float64, by bisection"""
    lo, hi = -1.3, -1.1
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if mish_grad(mid) < 0 else (lo, mid)
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def mish_sweep():
    f = np.float32
    nb = lambda v: [np.nextafter(f(v), f(-np.inf)), f(v), np.nextafter(f(v), f(np.inf))]
    special = [f(0.0), f(1e-30), f(-1e-30), f(88.0), f(-88.0)] + nb(19.0) + nb(20.0) + nb(mish_grad_zero())
    u = np.concatenate([np.linspace(-30.0, 30.0, 65536 - len(special)).astype(f), np.array(special, f)])
    return np.ascontiguousarray(u.reshape(256, 256))


# ---- head backward.  (mode 'cp' | 'cir', B, D, cu, head site (-1 none), below site, accumulate (db), w aliases dX, dtype)
HEAD_P = 0.1
HEAD_CASES = [
    ("cp", 1, 4, 0, 24, -1, 0, 0, "bf16"),
    ("cp", 7, 1024, 1, 24, 23, 1, 0, "f16"),           # cu[b] != b: the two sites' row indices differ
    ("cp", 300, 1028, 1, -1, 23, 0, 0, "bf16"),        # db: 300 > 256 terms; D: a second trip of the column loop, 4 columns long
    ("cp", 300, 1024, 0, 24, 23, 1, 0, "f16"),
    ("cir", 7, 1028, 0, -1, 23, 0, 1, "bf16"),         # as the step calls it: w is dX
    ("cir", 300, 4, 1, 24, 23, 0, 0, "f16"),
    ("cir", 1, 1024, 0, -1, -1, 0, 0, "bf16"),
]


def head_h(B):
    """db: ceil(B / 256) terms per thread, then the 8 levels of the 256-wide tree"""
    return -(-B // 256) + 8


@functools.lru_cache(maxsize=None)
def head_inputs(i):
    mode, B, D, cu, hs, bs, acc, alias, dt = HEAD_CASES[i]
    g = np.random.default_rng(3000 + i)
    dl = unit_mag(g, (B,)) if mode == "cp" else None
    w = unit_mag(g, (D,) if mode == "cp" else (B, D))
    cu_a = (np.cumsum(g.integers(2, 5, B)) - 1).astype(np.int32) if cu else None    # row of outfit b: 1 .. 3 at b = 0, then steps of 2 .. 4: never b
    rows = int(cu_a[-1]) + 3 if cu else B
    return dict(dlogits=dl, w=w, cu=cu_a, rows=rows, prefill=np.float32(-11.5))
