"""Float64 references of the towers' LayerNorm-fold chain (the producer and consumer epilogues of the GEMMs, stats_finalize_kernel,
row_stats_cast_kernel, vit_embed_ln_kernel, fold_pack_kernel, gather_hilo_kernel, layernorm_kernel) - TEST INFRASTRUCTURE ONLY.
Plain numpy; tests/test_cpu_fold_ops_ref.py pins every function to torch float64 and asserts that the cases below are SHARP (a
planted mistake exceeds the bound on the case's own inputs); tests/test_gpu_fold_ops.py compares the kernels with them.

    producer_ref      v = A W^T + bias + (h0 + l0): the value the (hi, lo) pair must hold; its magnitude sum for the bound
    seg_sums          per row and 64-column segment (sum, sum of squares)
    finalize_ref      (mean, rstd) from partials, float64;  finalize_emul: the kernel's one-pass formula step by step in np.float32
    consumer_ref      act((A Wf^T - col_sum mean) rstd + bias_f)
    ln_ref / ln_emul  LayerNorm rows, float64 / np.float32 two-pass (the yardstick of a correct fp32 row kernel)
    row_stats_ref / row_stats_emul, embed_rows (the rows vit_embed_ln normalises), fold_pack_ref

Bounds and their chain lengths h, each DERIVED from the code it stands next to (see the helpers).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle.bwd_ops import U32, round_op, sum_bound  # noqa: F401  (re-exported: one definition of each)

EPS = 1e-5
SEG = 64


# ---------------------------------------------------------------------------------------------------- number formats
def split_op(v, dt):
    """fp32 values -> the (hi, lo) pair as the kernels form it: hi = cast(v), lo = cast(fp32(v - hi)); both float32 arrays"""
    v = np.asarray(v, np.float32)
    hi = round_op(v, dt)
    return hi, round_op((v - hi).astype(np.float32), dt)


def ulp_op(hi, dt):
    """spacing of the operand type at |hi| (float64), subnormal spacing below the smallest normal"""
    p, emin = (8, -126) if dt == "bf16" else (11, -14)
    a = np.abs(np.asarray(hi, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 2.0 ** (np.maximum(e, emin) - (p - 1))


def pair_res(v, dt):
    """What a (hi, lo) pair cannot resolve of v: lo = cast(v - hi) carries a second rounding of a value that is at most half an ulp of
    hi.  f16: 2^-11 x 2^-11 |v| = 2^-22 |v|, and below f16's normal range (|lo| < 2^-14) half the subnormal spacing, 2^-25.
    bf16: 2^-8 x 2^-8 |v| = 2^-16 |v| (its exponent range is fp32's: no floor that these tests reach)."""
    a = np.abs(np.asarray(v, np.float64))
    return np.maximum(a * 2.0 ** -22, 2.0 ** -25) if dt == "f16" else a * 2.0 ** -16


# ---------------------------------------------------------------------------------------------------- references
def quick_gelu(z):
    return z / (1.0 + np.exp(-1.702 * z))


def producer_ref(a, w, bias, h0, l0, a_lo=None, w_lo=None):
    """-> (v, mag) float64 [M, N]: v = a w^T (+ a_lo w_lo^T: the correction product of split weights, a_lo = a unless the kernel sees
    another image of it) + bias + h0 + l0, mag = the sum of the magnitudes of all terms."""
    a, w, h0, l0 = (np.asarray(t, np.float64) for t in (a, w, h0, l0))
    b = np.zeros(w.shape[0]) if bias is None else np.asarray(bias, np.float64)
    v, mag = a @ w.T, np.abs(a) @ np.abs(w).T
    if w_lo is not None:
        al = a if a_lo is None else np.asarray(a_lo, np.float64)
        wl = np.asarray(w_lo, np.float64)
        v, mag = v + al @ wl.T, mag + np.abs(al) @ np.abs(wl).T
    return v + b[None, :] + h0 + l0, mag + np.abs(b)[None, :] + np.abs(h0) + np.abs(l0)


def value_bound(mag, K, v, dt):
    """|float(hi) + float(lo) - v| <= (K + 3) 2^-24 mag + pair_res(v): K fp32 accumulations in any order and the three additions of the
    epilogue (bias, h0 + l0, onto the accumulator), each relative 2^-24 of a partial sum that is at most mag; then the pair's own
    resolution.  K counts every product of the term (2K for split weights)."""
    return (K + 3) * U32 * np.asarray(mag, np.float64) + pair_res(v, dt)


def seg_sums(v):
    """[M, N] -> [M, N / 64, 2] float64 (sum, sum of squares) per 64-column segment"""
    v = np.asarray(v, np.float64)
    t = v.reshape(v.shape[0], -1, SEG)
    return np.stack([t.sum(-1), (t * t).sum(-1)], -1)


# chain of the producers' segment sums, both DPP trees (gemm_common.h):
#   epilogue (128- and 64-row tiles):  4 values per lane as (v0 + v1) + (v2 + v3): 2 dependent additions, then row16_sum_to_lane15:
#                                      row_shr 1, 2, 4, 8: 4                                                             -> 6
#   epilogue2<FOLD 3> (big tiles):     8 values per lane as ((..) + (..)) + ((..) + (..)): 3, then row8_sum: quad_perm, quad_perm,
#                                      row_half_mirror: 3                                                                -> 6
# the squares carry one more rounding each (the product; an fma leaves it out, which only helps)
H_SEG = 6


def part_bound(t, dt):
    """t = float(hi) + float(lo) as returned [M, N] -> bound [M, N / 64, 2] on |stat_part - seg_sums(t)|.  The kernel sums the fp32 v
    BEFORE the split, t is v to pair_res: (h + 3) 2^-24 sum |t| + sum pair_res(t) for the sums, and for the squares one more rounding
    and d(t^2) = 2 |t| pair_res(t)."""
    t = np.asarray(t, np.float64)
    a = np.abs(t).reshape(t.shape[0], -1, SEG)
    r = pair_res(t, dt).reshape(a.shape)
    return np.stack([(H_SEG + 3) * U32 * a.sum(-1) + r.sum(-1), (H_SEG + 4) * U32 * (a * a).sum(-1) + (2 * a * r + r * r).sum(-1)], -1)


def finalize_ref(part, W, eps=EPS):
    """float64 (mean, rstd) [rows, 2] from partials [rows, slots, 2]"""
    p = np.asarray(part, np.float64)
    mu = p[..., 0].sum(-1) / W
    var = np.maximum(p[..., 1].sum(-1) / W - mu * mu, 0.0)
    return np.stack([mu, 1.0 / np.sqrt(var + np.float64(np.float32(eps)))], -1)


def finalize_emul(part, W, eps=EPS):
    """stats_finalize_kernel step by step in np.float32: the sequential slot loop, s / W, q / W - mu mu, the clamp, rsqrt"""
    f = np.float32
    p = np.asarray(part, f)
    s, q = np.zeros(p.shape[0], f), np.zeros(p.shape[0], f)
    for k in range(p.shape[1]):
        s, q = s + p[:, k, 0], q + p[:, k, 1]
    mu = s / f(W)
    var = np.maximum(q / f(W) - mu * mu, f(0))
    return np.stack([mu, (f(1) / np.sqrt((var + f(eps)).astype(np.float64))).astype(f)], -1)


def finalize_c(slots):
    """The constant of the one-pass bound  |rstd - ref| / ref <= c 2^-24 E[x^2] / (Var + eps) + 3 2^-24,  from the chain of
    stats_finalize_kernel (norm_act.hip), u = 2^-24, E2 = q / W, first order:
      q = sum of `slots` partials, sequentially: slots - 1 additions, |dq| <= (slots - 1) u q;  q / W: one more -> slots u E2
      s likewise, mu = s / W: relative slots u;  mu mu: 2 slots u + u relative of mu^2 <= E2
      var = E2' - mu^2': |dvar| <= slots u E2 + (2 slots + 1) u mu^2 + u var <= (3 slots + 1) u E2 + u var
      rstd = rsqrt(var + eps): half the relative error of its argument, + u for the addition of eps (halved), + 2 u for rsqrt's own
      1-ulp result:  (3 slots + 1) / 2 . u . E2 / (var + eps)  +  (u / 2 + u / 2 + 2 u = 3 u).
    c = (3 slots + 1) / 2: 12.5, 18.5, 24.5 for 8, 12, 16 slots (<= 32)."""
    return (3 * slots + 1) / 2.0


def finalize_bound(cond, slots):
    return finalize_c(slots) * U32 * np.asarray(cond, np.float64) + 3 * U32


def partials_share(cond, dt):
    """What the producer's partials add to the relative error of rstd when it is judged against float64 statistics of the returned hi + lo
    (part_bound, relative): the sums are off by (H_SEG + 3) u, so mu^2 by twice that of at most E2; the sums of squares by (H_SEG + 4) u
    of E2; rstd takes half the relative error of var: ((H_SEG + 3) + (H_SEG + 4) / 2) u cond.  And hi + lo is the summed fp32 v only to
    the pair's relative resolution r (2^-22 f16, 2^-16 bf16): r from mu^2, r from the squares (2 r, halved): 2 r cond."""
    r = 2.0 ** -22 if dt == "f16" else 2.0 ** -16
    return ((H_SEG + 3) + (H_SEG + 4) / 2.0) * U32 * np.asarray(cond, np.float64) + 2 * r * np.asarray(cond, np.float64)


def cond_of(x, eps=EPS):
    """E[x^2] / (Var + eps) per row, float64"""
    x = np.asarray(x, np.float64)
    return (x * x).mean(-1) / (x.var(-1) + eps)


def consumer_ref(a, wf, col_sum, mean, rstd, bias, act=0, w_lo=None):
    a, wf = np.asarray(a, np.float64), np.asarray(wf, np.float64)
    z = a @ wf.T
    if w_lo is not None:
        z = z + a @ np.asarray(w_lo, np.float64).T
    z = (z - np.asarray(col_sum, np.float64)[None, :] * np.asarray(mean, np.float64)[:, None]) * np.asarray(rstd, np.float64)[:, None]
    z = z + np.asarray(bias, np.float64)[None, :]
    return quick_gelu(z) if act else z


CONSUMER_BOUND = 1e-3      # max |got - ref| / max |ref|, as tests/test_gpu_gemm_epilogue_consts.py: output rounding (2^-9 bf16 is judged
#                            per element on top, see the GPU test) + fp32 accumulation; a wrong constant is off by O(1)


def ln_ref(x, gamma=None, beta=None, eps=EPS):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(x.var(-1, keepdims=True) + np.float64(np.float32(eps)))
    return y if gamma is None else y * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def wave_tree(s):
    """wave_sum (ofx_common.h) on np.float32 [..., 64]: v += v[lane ^ o] for o = 32 .. 1; every lane ends with the same total"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lanes ^ o]
    return s[..., 0]


def _lanes(x):
    """[rows, W] -> [rows, W / 256, 64, 4]: chunk c of lane l holds columns 256 c + 4 l .. + 3, as the one-wave-per-row kernels read a row
    (W a multiple of 256: 512, 768, 1024)"""
    return x.reshape(x.shape[0], -1, 64, 4)


def _row_mean(x, paired, recip):
    """the kernels' row mean in np.float32, in their order: per lane the chunks in turn, a chunk's four values as ((a + b) + c) + d
    (layernorm_kernel, vit_embed_ln_kernel's first pass) or (a + b) + (c + d) (row_stats_cast_kernel, vit_embed_ln_kernel's statistics),
    then wave_tree, then x (1 / W) rounded or / W.  A row's mean of |mu| / sigma = k carries k times its half-ulp into every output, so the
    yardstick has to round where the kernel rounds: with np.sum's pairwise order instead, its error on such a row is another draw."""
    f = np.float32
    v = _lanes(x)
    s = np.zeros(v.shape[:1] + (64,), f)
    for c in range(v.shape[1]):
        s = s + (((v[:, c, :, 0] + v[:, c, :, 1]) + (v[:, c, :, 2] + v[:, c, :, 3])) if paired else (((v[:, c, :, 0] + v[:, c, :, 1]) + v[:, c, :, 2]) + v[:, c, :, 3]))
    t = wave_tree(s)
    W = f(x.shape[1])
    return (t * (f(1.0) / W) if recip else t / W).astype(f)


def _row_sumsq(d):
    """per lane the squares in column order, one after the other, then wave_tree"""
    f = np.float32
    v = _lanes(d)
    q = np.zeros(v.shape[:1] + (64,), f)
    for c in range(v.shape[1]):
        for e in range(4):
            q = q + v[:, c, :, e] * v[:, c, :, e]
    return wave_tree(q)


def ln_emul(x, gamma, beta, eps=EPS):
    """layernorm_kernel / vit_embed_ln_kernel step by step in np.float32, in the kernels' order of summation -> float32"""
    f = np.float32
    x = np.ascontiguousarray(x, f)
    D = x.shape[-1]
    d = x - _row_mean(x, False, True)[:, None]
    rstd = (f(1) / np.sqrt((_row_sumsq(d) * (f(1.0) / f(D)) + f(eps)).astype(np.float64))).astype(f)
    o = d * rstd[:, None] * np.asarray(gamma, f) + np.asarray(beta, f)
    assert o.dtype == f
    return o


def row_stats_ref(x, eps=EPS):
    x = np.asarray(x, np.float64)
    return np.stack([x.mean(-1), 1.0 / np.sqrt(x.var(-1) + np.float64(np.float32(eps)))], -1)


def row_stats_emul(x, eps=EPS, recip=False):
    """row_stats_cast_kernel (recip False: sum / W) or the statistics pass of vit_embed_ln_kernel (recip True: sum x fp32(1 / W)) in np.float32"""
    f = np.float32
    x = np.ascontiguousarray(x, f)
    W = f(x.shape[-1])
    mu = _row_mean(x, True, recip)
    q = _row_sumsq(x - mu[:, None])
    var = q * (f(1.0) / W) if recip else q / W
    return np.stack([mu, (f(1) / np.sqrt((var + f(eps)).astype(np.float64))).astype(f)], -1).astype(f)


def embed_rows(patch_out, cls, pos, N, S):
    """[N S, D]: row n S + t = (t == 0 ? cls : patch_out[n (S - 1) + t - 1]) + pos[t], in the dtype of the inputs (fp32: one addition)"""
    D = cls.shape[0]
    x = np.concatenate([np.broadcast_to(cls, (N, 1, D)), patch_out.reshape(N, S - 1, D)], 1) + pos[None]
    return x.reshape(N * S, D)


def fold_pack_ref(w, gamma, beta, bias, dt, split):
    """-> dict(hi, lo (or None): float32 bit-exact expectations; cs_terms [K or 2K, N], bias_terms [K + 1, N]: float64 terms of the sums"""
    f = np.float32
    w, gamma, beta, bias = (np.asarray(t, f) for t in (w, gamma, beta, bias))
    wg = (w * gamma[None, :]).astype(f)
    hi = round_op(wg, dt)
    lo = round_op((wg - hi).astype(f), dt) if split else None
    bt = np.concatenate([(beta[None, :].astype(np.float64) * w.astype(np.float64)).T, bias[None, :].astype(np.float64)], 0)
    return dict(hi=hi, lo=lo, bias_terms=bt)


def fold_pack_h(K, split):
    """fold_pack_kernel: a lane adds its K / 64 columns in turn (hi then lo of each under split: doubled), then wave_sum: 6 xor steps"""
    return -(-K // 64) * (2 if split else 1) + 6


def rel_rows(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(got - ref, axis=-1) / np.maximum(np.linalg.norm(ref, axis=-1), 1e-300)


# ---------------------------------------------------------------------------------------------------- cases and inputs
# ofx_tune(2, v) -> (name, kind in the profile record, weight form, rows per tile)
ROUTES = {"128": (1, 1, 0), "64": (5, 5, 0), "256x256": (2, 2, 0), "256x128": (3, 3, 0), "pingpong": (4, 4, 0), "w2": (6, 6, 1), "w2f8": (6, 8, 2)}
M_ALL = (1, 8, 9, 16, 17, 255, 257, 600)
M_SMALL_TILES = (63, 65, 129)
# (M, N, K) of one route: N = 256 / K = 128 over every M, N = 768 at two M, and the bench's K once
def producer_shapes(route):
    ms = M_ALL + (M_SMALL_TILES if route in ("128", "64") else ())
    return [(m, 256, 128) for m in ms] + [(17, 768, 128), (257, 768, 128), (600, 768, 768)]


CONSUMER_SHAPES = [(1, 256, 128), (255, 512, 128), (600, 768, 768)]
STRIDED = dict(nseq=7, S=50, N=256, K=128)
FINALIZE_ROWS, FINALIZE_SLOTS, FINALIZE_RATIOS = (1, 255, 256, 257), (8, 12, 16), (0, 1, 16, 256)


def _seed(*k):
    return abs(hash(tuple(int(x) if not isinstance(x, str) else sum(map(ord, x)) for x in k))) % (2 ** 31)


def offsets(M, N):
    """every row and every 64-column segment its own offset: neighbours differ by >= 0.75 (rows) / 1.1 (segments), never 0"""
    r = ((np.arange(M) * 7) % 13 - 6) * 0.75 + 0.3
    s = ((np.arange(N // SEG) * 5) % 7 - 3) * 1.1 + 0.2
    return r[:, None] + np.repeat(s, SEG)[None, :]


@functools.lru_cache(maxsize=8)
def producer_random(M, N, K, dt, form):
    """Random producer case: operands already in the operand type (float32 arrays), real lo halves of the stream and of split weights."""
    g = np.random.default_rng(_seed(M, N, K, dt, form, 1))
    a = round_op(g.standard_normal((M, K)) * 0.5, dt)
    w32 = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    w, wl = split_op(w32, dt)
    bias = g.standard_normal(N).astype(np.float32)
    x0 = (offsets(M, N) + g.standard_normal((M, N))).astype(np.float32)
    h0, l0 = split_op(x0, dt)
    return dict(a=a, w=w, w_lo=wl if form else None, bias=bias, h0=h0, l0=l0)


@functools.lru_cache(maxsize=8)
def producer_lattice(M, N, K, dt, form):
    """Exact case: a, w in {-1, 0, 1}, bias and h0 small integers, l0 and the weights' lo halves multiples of 1/4: every accumulation,
    every v and every 64-term sum of v and v^2 is an exact fp32 (and operand-type pair) value - lattice_is_exact checks it."""
    g = np.random.default_rng(_seed(M, N, K, dt, form, 2))
    a = g.choice([-1.0, 0.0, 0.0, 1.0], (M, K)).astype(np.float32)
    w = g.choice([-1.0, 0.0, 0.0, 1.0], (N, K)).astype(np.float32)
    wl = None
    if form:
        wl = np.zeros((N, K), np.float32)
        cols = g.integers(0, K, (N, 2))
        wl[np.arange(N)[:, None], cols] = g.choice([-0.25, 0.25], (N, 2))      # every row has a non-zero lo: the fp8 copy scales each row by its max |lo|
    bias = g.integers(-8, 9, N).astype(np.float32)
    h0 = (g.integers(-12, 13, (M, N)) + np.rint(offsets(M, N))).astype(np.float32)
    l0 = (g.integers(-2, 3, (M, N)) * 0.25).astype(np.float32)
    return dict(a=a, w=w, w_lo=wl, bias=bias, h0=h0, l0=l0)


def lattice_is_exact(c, dt):
    """Sufficient conditions, checked on the float64 result: v a multiple of 1/4 with |v| < 128 (so a 9-bit integer part + 2 fraction
    bits: hi and lo both exact in bf16 (8 + 8 bits) and f16); every partial sum of a subset of a segment's v is a multiple of 1/4 below
    2^22, of its v^2 a multiple of 1/16 below 2^20: 24 bits in any order of summation; the accumulator likewise (|acc| <= sum |a w| < 2^22)."""
    v, mag = producer_ref(c["a"], c["w"], c["bias"], c["h0"], c["l0"], w_lo=c["w_lo"])
    hi, lo = split_op(v.astype(np.float32), dt)
    ok = np.array_equal(v * 4, np.rint(v * 4)) and float(np.abs(v).max()) < 128 and float(mag.max()) < 2 ** 22
    ok = ok and np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), v) and bool((np.abs(lo) <= ulp_op(hi, dt) / 2).all())
    s = seg_sums(np.abs(v))
    return bool(ok and s[..., 0].max() < 2 ** 22 and s[..., 1].max() < 2 ** 20)


@functools.lru_cache(maxsize=8)
def consumer_case(M, N, K, dt, form, act):
    """every row its own (mean, rstd) - mean / std up to 16 so that a col_sum error shows -, every column its own bias and col_sum"""
    g = np.random.default_rng(_seed(M, N, K, dt, form, act, 3))
    a = round_op(g.standard_normal((M, K)), dt)
    w, wl = split_op((g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), dt)
    mean = (g.standard_normal(M) * 0.25 + ((np.arange(M) * 5) % 11 - 5)).astype(np.float32)        # neighbours differ by 5 or 6, +- 1
    rstd = g.uniform(0.5, 2.0, M).astype(np.float32)
    return dict(a=a, w=w, w_lo=wl if form else None, mean=mean, rstd=rstd, bias=g.standard_normal(N).astype(np.float32),
                col_sum=g.standard_normal(N).astype(np.float32))


CHAIN = dict(M=130, N=256, K=256)


@functools.lru_cache(maxsize=4)
def chain_case(dt, split):
    """fp32 rows with mean / std cycling through 0, 1, 4, 16 and a per-row scale, an fp32 weight matrix and LayerNorm parameters"""
    M, N, K = CHAIN["M"], CHAIN["N"], CHAIN["K"]
    g = np.random.default_rng(_seed(dt, split, 6))
    sd = g.uniform(0.5, 2.0, (M, 1))
    ratio = np.array([0.0, 1.0, 4.0, 16.0])[np.arange(M) % 4][:, None] * g.choice([-1.0, 1.0], (M, 1))
    x = (g.standard_normal((M, K)) * sd + ratio * sd).astype(np.float32)
    return dict(x=x, w=(g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), gamma=g.uniform(0.5, 2.0, K).astype(np.float32),
                beta=(g.standard_normal(K) * 0.5).astype(np.float32), bias=g.standard_normal(N).astype(np.float32))


def finalize_rows(rows, slots, ratio, seed=0):
    """float64 row data [rows, 64 slots] with mean / std = ratio (ratio 0: mean 0), std between 0.5 and 2 per row"""
    g = np.random.default_rng(_seed(rows, slots, ratio, seed, 4))
    W = slots * SEG
    z = g.standard_normal((rows, W))
    z = (z - z.mean(-1, keepdims=True)) / z.std(-1, keepdims=True)
    sd = g.uniform(0.5, 2.0, (rows, 1))
    sign = g.choice([-1.0, 1.0], (rows, 1))
    return z * sd + sign * ratio * sd


def stream_rows(rows, W, seed):
    """fp32 rows shaped like a residual stream: per-row offset and scale"""
    g = np.random.default_rng(_seed(rows, W, seed, 5))
    x = g.standard_normal((rows, W)) * g.uniform(0.3, 3.0, (rows, 1)) + g.standard_normal((rows, 1)) * 2
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the fixtures' one-pass envelope
def vit_stream_cond(pixels, W, n_layers=12, n_head=12, prefix="vision_model."):
    """oracle.np_oracle's ViT forward (float64 here) with a tap on the residual stream after every out-proj and fc2 - the rows
    stats_finalize sees -> (max E[x^2] / (Var + eps) over all taps, image embeddings for the pin against vit_forward)."""
    from oracle import np_oracle as O
    dt = np.float64
    g = lambda k: W[k].astype(dt)
    pw = g(prefix + "embeddings.patch_embedding.weight")
    width = pw.shape[0]
    pe = O.patchify(pixels.astype(dt), pw.shape[-1]) @ pw.reshape(width, -1).T
    N = pe.shape[0]
    x = np.concatenate([np.broadcast_to(g(prefix + "embeddings.class_embedding"), (N, 1, width)), pe], 1) + g(prefix + "embeddings.position_embedding.weight")[None]
    x = O.layer_norm(x, g(prefix + "pre_layrnorm.weight"), g(prefix + "pre_layrnorm.bias"))
    dead = np.zeros(x.shape[:2], bool)
    worst = 0.0
    for i in range(n_layers):
        p = f"{prefix}encoder.layers.{i}."
        q = lambda k: W[p + k].astype(dt)
        h = O.layer_norm(x, q("layer_norm1.weight"), q("layer_norm1.bias"))
        x = x + O._mha(h, dead, q("self_attn.q_proj.weight"), q("self_attn.q_proj.bias"), q("self_attn.k_proj.weight"), q("self_attn.k_proj.bias"),
                       q("self_attn.v_proj.weight"), q("self_attn.v_proj.bias"), q("self_attn.out_proj.weight"), q("self_attn.out_proj.bias"), n_head)
        worst = max(worst, float(cond_of(x).max()))
        h = O.layer_norm(x, q("layer_norm2.weight"), q("layer_norm2.bias"))
        x = x + O.quick_gelu(h @ q("mlp.fc1.weight").T + q("mlp.fc1.bias")) @ q("mlp.fc2.weight").T + q("mlp.fc2.bias")
        worst = max(worst, float(cond_of(x).max()))
    pooled = O.layer_norm(x[:, 0], g(prefix + "post_layernorm.weight"), g(prefix + "post_layernorm.bias"))
    return worst, pooled @ g("visual_projection.weight").T
