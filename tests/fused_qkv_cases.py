"""The case table, the inputs and the float64 model of the exact-arithmetic tests of fused_qkv_attn_kernel (csrc/fused_qkv_attn.hip):
tests/test_cpu_fused_qkv_exact.py checks on the CPU what every case claims, tests/test_gpu_fused_qkv_exact.py runs the same arrays
through ofx_fused_qkv_attention / ofx_fused_qkv_attention_w2 and through the unfused pair GEMM -> ofx_attention.  Nothing here touches
HIP at import.

THE EXACTNESS CONDITION.  X = integers in [-7, 7] x q_a; every stored weight block (W, or hi and lo independently) = integers in
[-7, 7] x q_w; q_a and q_w powers of two, q = q_a q_w; bias = integers in [-64, 64] x q; with the LayerNorm fold mean[m] = integers in
[-3, 3] x q_a, col_sum[n] = integers in [-64, 64] x q_w and rstd[m] in {1/2, 1, 2}.  Every product x w and col_sum mean is then a multiple
of q, and every term of

    (acc - col_sum mean) rstd + bias,      acc = sum over the products (hi; lo) and over k of x w,

and every partial sum of such terms taken in ANY order and in any algebraic arrangement of the epilogue (acc rstd - col_sum (mean rstd)
+ bias, ...) is a multiple of q / 2.  Such a number is exact in float32 while its magnitude stays below 2^24 q / 2, and no partial sum
exceeds

    bound = max over (m, n) of  (sum over the products of sum_k |x| |w|  +  |col_sum| |mean|) |rstd|  +  |bias|,

so   bound < 2^24 q / 2   makes the fp32 value independent of the summation order, of fma contraction and of the form of the epilogue:
it EQUALS float64 arithmetic on the same arrays.  The operand-type q | k | v are ONE deterministic round-to-nearest-even of that value:
the same bits in the fused kernel, in the unfused GEMM and in numpy.  `build` computes the bound, the CPU test asserts it for every
case (the `route` family mixes 128 = 128 / q_a units of q_a into X; the bound is computed from the arrays, whatever they hold).

q = 2^-e with e = round(log2(sqrt(K n_products) 18.67)) - 18.67 = (15^2 - 1) / 12 is the variance of a uniform integer in [-7, 7] -
split as q_a = 2^-(e div 2), q_w = q / q_a: q and k then have a standard deviation near 1 before the rstd factor, and the softmax is
neither flat nor one-hot (the CPU test holds the median over the queries of the largest probability inside [1.5 / S, 0.6]).

Families
  ints    as above: a generic softmax on exactly known q | k | v.  The GPU test asserts (A) value equality with the unfused pair - both
          run attn_scores / attn_softmax_p / attn_pv_store of csrc/attn_wave.h at NT = 4 on the same q | k | v bits - and (B) every
          (image, head) block against float64.
  route   an exact check that leans on no other kernel.  Code amplitude a = 128.  Row r of image i has X[row, pi_i(r)] = a and
          X[row, 64 + r] = a, zero in the other columns below 128, integers x q_a from column 128 on (pi_i: a seeded permutation of
          [0, S)).  Head h's q rows are the selection q[., rho_h(c)] = x[., c], c < 64 (rho_h: a per-head permutation of [0, S), the
          identity on [S, 64)); its k rows the selection k[., d] = x[., 64 + d]; for dual weights the selection sits in hi and lo = 0
          on those rows; bias and col_sum are 0 on the q and k columns; the v rows are `ints`.  Then
              q[r, d] = a rstd_r [d = rho_h(pi_i(r))],   k[j, d] = a rstd_j [d = j],   score(r, j) = a^2 rstd_r rstd_j [j = rho_h(pi_i(r))]:
          one key wins with a raw score of at least a^2 / 4 = 4096, every other key scores 0.  The kernel's exponent argument of a
          loser is (0 - s_win) scale log2 e <= -4096 x 0.125 x 1.4427 = -738 (the CPU test asserts a margin >= 160 from the rounded
          q and k), and exp2 of anything below -149 is exactly 0 in float32: the sum is the winner's e alone, e / sum = 1 up to one
          rounding of the reciprocal, and P rounds to exactly 1.0 in the operand type (11 or 8 significand bits).  O = 1.0 v_win +
          zeros is v_win itself, already an operand-type value.  ASSERTION: out[i, r, head h] == v[i, rho_h(pi_i(r)), h] of the float64
          model, bit for bit as values.  This pins image -> wave, head -> weight rows, head -> output columns, group -> block, the
          key >= S mask (an unmasked key of the next image would tie or win) and the V projection with fold and lo.

MUTANTS of `model`, each one plausible slip in this kernel (`applies` says where a mutant can show):
   1  the lo product dropped (dual-weight kernel)                  7  col_sum of the q block used for k and v too (fold)
   2  the last k-step dropped (64 columns single, 32 dual)         8  bias added before the rstd multiply (fold)
   3  the first k-step applied twice                               9  keys S .. 63 not masked: the tile's next rows leak in (S < 64; rows
   4  heads 0 and 1 exchange their k weight rows (ints: route's       past the tile's 256 stay dead, rows past M are the clamped row M - 1)
      k rows are the same selection in every head)                10  output columns of head h written at head heads - 1 - h
   5  in a ragged last group wave w takes image w + 1's rows      11  the row clamp M - 1 missing: rows past M read as NaN, and 0 x NaN
   6  row_stat indexed without the group's row offset m0 (fold,       reaches the last image's output through its keys S .. 63 (S < 64)
      more than one group)
"""
import collections
import functools
import zlib

import numpy as np

from oracle import attn_fwd as A

DTYPES = ("bf16", "f16")
KERNELS = ("single", "dual")
SCALE = 0.125
AMP = 128.0
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
OLD_REL_ERR = {"bf16": 8e-3, "f16": 1e-3}          # tests/test_gpu_ops.py: max|a - b| / max|b| over the whole tensor
F_OP = 1.6                                         # tests/test_gpu_attention_fwd.py F_OP: the same wave core
MUTANTS = tuple(range(1, 12))
OFX_OK, OFX_EINVAL, OFX_ESHAPE = 0, -1, -2
TILE_M, PAD_ROWS = 256, 16                         # FQ_TM, the zeroed V rows behind the tile
EXTRA_ROWS = 3                                     # NaN rows behind X and row_stat in the `strides` sweep

# name    free-form, unique            sweep   seq | images | heads | nofold | strides | route
# family  ints | route                 kernel  single (ofx_fused_qkv_attention) | dual (ofx_fused_qkv_attention_w2)
# pad     0, or 8: ldx = ldo = width + 8, X's pad columns NaN, EXTRA_ROWS NaN rows behind X and row_stat
# claims  what the case is in the table for: "unit-row-2" (a live block in the block order's second row of units), "odd-heads"
Case = collections.namedtuple("Case", "name sweep family kernel dt S heads n_img fold pad claims")


def group_size(S):
    return TILE_M // S


def _case(sweep, family, kernel, dt, S, heads, n_img, fold=1, pad=0):
    G = group_size(S)
    claims = (("unit-row-2",) if (n_img + G - 1) // G > 6 else ()) + (("odd-heads",) if heads % 2 else ())
    return Case(f"{sweep}-{kernel}-{dt}-S{S}-h{heads}-n{n_img}{'' if fold else '-nofold'}{'-pad' if pad else ''}", sweep, family, kernel, dt, S, heads,
                n_img, fold, pad, claims)


SEQ_S = (33, 34, 37, 41, 43, 50, 51, 52, 63, 64)    # every G = 7, 6, 5, 4; key-row overshoot past row 255: 6, 12, < 0, 13, < 0, 8, 12, < 0, < 0, 0
IMAGES_N = (1, 4, 5, 6, 10, 30, 31)                 # S = 50 (G = 5): 30 = exactly six groups, 31 = a seventh group: the second unit row
HEADS_H = (2, 3, 4, 5, 12)                          # k-steps 2, 3, 4, 5, 12 single and 4, 6, 8, 10, 24 dual: every residue mod 2 and mod 3
REFUSED_S = (32, 35, 36, 42, 65)


def _sweeps(kernel, dt):
    c = lambda *a, **kw: _case(a[0], "ints", kernel, dt, *a[1:], **kw)
    r = lambda *a: _case("route", "route", kernel, dt, *a)
    return {
        "seq": [c("seq", S, 2, group_size(S) + 1) for S in SEQ_S],
        "images": [c("images", 50, 2, n) for n in IMAGES_N] + [c("images", 64, 2, 25)],
        "heads": [c("heads", 50, h, 6) for h in HEADS_H] + [c("heads", 50, 3, 31)],
        "nofold": [c("nofold", 50, h, 6, fold=0) for h in (2, 3)],
        "strides": [c("strides", 41, 3, 7, pad=8)],
        "route": [r(S, h, group_size(S) + 1) for S in (33, 50, 64) for h in (2, 3)] + [r(50, h, 31) for h in (2, 3)],
    }


GROUPS = {f"{sweep}-{kernel}-{dt}": cases for kernel in KERNELS for dt in DTYPES for sweep, cases in _sweeps(kernel, dt).items()}
CASES = [c for cs in GROUPS.values() for c in cs]
assert len({c.name for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------ the launcher and the block order, restated
def xcd_remap(bid, nwg):
    """csrc/gemm_walk.h."""
    nx = 8
    q, r, x, i = nwg // nx, nwg % nx, bid % nx, bid // nx
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + i


def geometry(S, heads, n_img):
    """ofx_launch_fused_qkv_attn -> (G, groups, nwg)."""
    G = group_size(S)
    groups = (n_img + G - 1) // G
    return G, groups, ((groups + 5) // 6) * 6 * heads


def block_of(block_idx, heads, nwg):
    """fused_qkv_attn_kernel: blockIdx.x -> (group, head, unit row)."""
    bid = xcd_remap(block_idx, nwg)
    hh = heads // 2 if heads % 2 == 0 else heads
    halves, per_unit = heads // hh, 6 * hh
    unit, in_unit = bid // per_unit, bid % per_unit
    return (unit // halves) * 6 + in_unit // hh, (unit % halves) * hh + in_unit % hh, unit // halves


def admission(S, width, heads, ldx, ldo, n_img=1, X=True, row_stat=False, col_sum=False):
    """The return code ofx_launch_fused_qkv_attn states for these arguments (its OFX_REQUIRE lines, in their order)."""
    if not X or n_img <= 0:
        return OFX_EINVAL
    if not (33 <= S <= 64 and width == heads * 64 and width % 64 == 0 and width // 64 >= 2):
        return OFX_ESHAPE
    if (TILE_M // S - 1) * S + 64 - TILE_M > PAD_ROWS:
        return OFX_ESHAPE
    if not (ldx >= width and ldx % 8 == 0 and ldo >= width and ldo % 8 == 0):
        return OFX_ESHAPE
    if row_stat and not col_sum:
        return OFX_EINVAL
    return OFX_OK


# ------------------------------------------------------------------------------------------------ the inputs
def _ints(g, shape, lim):
    return g.integers(-lim, lim + 1, size=shape).astype(np.float64)


def quanta(K, n_products):
    e = int(round(np.log2(np.sqrt(K * n_products) * 18.67)))
    qa = 2.0 ** -(e // 2)
    return qa, 2.0 ** -e / qa


@functools.lru_cache(maxsize=6)
def _arrays(family, kernel, S, heads, n_img, fold, pad):
    """The arrays of a case (float64 holding values exact in bf16 and f16; they do not depend on the operand type).  READ-ONLY."""
    g = np.random.default_rng(zlib.crc32(repr((family, kernel, S, heads, n_img, fold, pad)).encode()))
    W, M = heads * 64, n_img * S
    nprod = 2 if kernel == "dual" else 1
    qa, qw = quanta(W, nprod)
    q = qa * qw
    x = _ints(g, (M, W), 7) * qa
    blocks = [_ints(g, (3 * W, W), 7) * qw for _ in range(nprod)]
    bias = _ints(g, (3 * W,), 64) * q
    mean = _ints(g, (M,), 3) * qa if fold else np.zeros(M)
    rstd = np.array([0.5, 1.0, 2.0])[g.integers(0, 3, M)] if fold else np.ones(M)
    col_sum = _ints(g, (3 * W,), 64) * qw if fold else np.zeros(3 * W)
    pi = rho = None
    if family == "route":
        pi = np.stack([g.permutation(S) for _ in range(n_img)])
        rho = np.stack([g.permutation(S) for _ in range(heads)])
        r = np.arange(S)
        x[:, :128] = 0.0
        for i in range(n_img):
            x[i * S + r, pi[i]] = AMP
            x[i * S + r, 64 + r] = AMP
        d = np.arange(64)
        for b, blk in enumerate(blocks):
            blk[:2 * W] = 0.0
            if b == 0:
                for h in range(heads):
                    full = np.concatenate([rho[h], np.arange(S, 64)])
                    blk[h * 64 + full, d] = 1.0                 # q[., rho_h(c)] = x[., c]
                    blk[W + h * 64 + d, 64 + d] = 1.0           # k[., d] = x[., 64 + d]
        bias[:2 * W] = 0.0
        col_sum[:2 * W] = 0.0
    ldx = W + pad
    rows = M + (EXTRA_ROWS if pad else 0)
    X = np.full((rows, ldx), np.nan)
    X[:M, :W] = x
    stat = np.full((rows, 2), np.nan)
    stat[:M, 0], stat[:M, 1] = mean, rstd
    mag = sum(np.abs(x) @ np.abs(b).T for b in blocks)
    bound = float(((mag + np.abs(col_sum)[None] * np.abs(mean)[:, None]) * np.abs(rstd)[:, None] + np.abs(bias)[None]).max())
    dd = dict(X=X, x=x, blocks=blocks, Wmat=np.concatenate(blocks, 1), bias=bias, mean=mean, rstd=rstd, stat=stat, col_sum=col_sum, qa=qa, qw=qw, q=q,
              bound=bound, ldx=ldx, ldo=W + pad, W=W, M=M, pi=pi, rho=rho)
    for v in dd.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    for b in blocks:
        b.setflags(write=False)
    return dd


def build(case):
    """-> dict: X [M (+ EXTRA_ROWS), ldx] (pad columns and extra rows NaN), x = its live part, blocks = [W] or [hi, lo] ([3 W, W] each),
    Wmat = [W] or [hi | lo], bias, col_sum [3 W], mean, rstd [M], stat [M (+ EXTRA_ROWS), 2], qa, qw, q, bound, ldx, ldo, W, M, and for
    `route` pi [n_img, S], rho [heads, S].  All float64, every value exact in both operand types."""
    return _arrays(case.family, case.kernel, case.S, case.heads, case.n_img, case.fold, case.pad)


# ------------------------------------------------------------------------------------------------ the float64 model
def applies(case, mutant):
    G, groups, _ = geometry(case.S, case.heads, case.n_img)
    return {1: case.kernel == "dual", 2: True, 3: True, 4: case.family == "ints", 5: case.n_img % G != 0, 6: bool(case.fold) and groups > 1,
            7: bool(case.fold), 8: bool(case.fold), 9: case.S < 64, 10: True, 11: case.S < 64}[mutant]


def qkv64(case, mutant=None):
    """q | k | v [M, 3 W] in float64, before the rounding to the operand type."""
    d = build(case)
    W, M, S = d["W"], d["M"], case.S
    bk = 64 if case.kernel == "single" else 32
    x = d["x"]
    blocks = list(d["blocks"][:1] if mutant == 1 else d["blocks"])
    if mutant == 4:
        swap = np.arange(3 * W)
        swap[W:W + 64], swap[W + 64:W + 128] = np.arange(W + 64, W + 128), np.arange(W, W + 64)
        blocks = [b[swap] for b in blocks]
    kk = slice(0, W - bk) if mutant == 2 else slice(0, W)
    acc = sum(x[:, kk] @ b[:, kk].T for b in blocks)
    if mutant == 3:
        acc = acc + sum(x[:, :bk] @ b[:, :bk].T for b in blocks)
    bias = d["bias"][None]
    if not case.fold:
        return acc + bias
    mean, rstd, cs = d["mean"], d["rstd"], d["col_sum"]
    if mutant == 6:
        in_tile = np.arange(M) % (group_size(S) * S)
        mean, rstd = mean[in_tile], rstd[in_tile]
    if mutant == 7:
        cs = np.tile(cs[:W], 3)
    centred = acc - cs[None] * mean[:, None]
    return (centred + bias) * rstd[:, None] if mutant == 8 else centred * rstd[:, None] + bias


def to_heads(a, case):
    """[n_img * S, W] -> [n_img, heads, S, 64]."""
    return a.reshape(case.n_img, case.S, case.heads, 64).transpose(0, 2, 1, 3)


def from_heads(a, case):
    return a.transpose(0, 2, 1, 3).reshape(case.n_img * case.S, case.heads * 64)


Model = collections.namedtuple("Model", "qkv q k v ref emul out")


@functools.lru_cache(maxsize=4)
def model(case, mutant=None):
    """-> Model: qkv [M, 3 W] = the operand-rounded q | k | v (float64 values), q, k, v [n_img, heads, S, 64], ref / emul [n_img, heads, S,
    64] = oracle.attn_fwd.attn_fwd_ref / attn_fwd_emul on them, out [M, W] = the expected output rows: emul for `ints`, the routed v
    rows for `route` (the CPU test shows emul equal to them).  With a mutant everything is what the slipped kernel would hold."""
    assert mutant is None or applies(case, mutant), (case.name, mutant)
    d = build(case)
    W, M, S, n = d["W"], d["M"], case.S, case.n_img
    G = group_size(S)
    qkv = A.round_to(qkv64(case, mutant), case.dt)
    if mutant == 5:
        first = (n // G) * G                                              # the ragged last group's first image
        src = np.arange(M)
        src[first * S:] = np.minimum(src[first * S:] + S, M - 1)
        qkv = qkv[src]
    q, k, v = (to_heads(qkv[:, i * W:(i + 1) * W], case) for i in range(3))
    if mutant == 9:
        ref, emul = np.empty_like(q), np.empty_like(q)
        for i in range(n):
            w, m0 = i % G, (i // G) * G * S
            rows = np.minimum(m0 + w * S + np.arange(min(64, TILE_M - w * S)), M - 1)
            ke, ve = (qkv[rows, o * W:(o + 1) * W].reshape(len(rows), case.heads, 64).transpose(1, 0, 2) for o in (1, 2))
            ref[i], emul[i] = A.attn_fwd_ref(q[i], ke, ve, None, SCALE), A.attn_fwd_emul(q[i], ke, ve, None, SCALE, case.dt)
    else:
        ref, emul = A.attn_fwd_ref(q, k, v, None, SCALE), A.attn_fwd_emul(q, k, v, None, SCALE, case.dt)
    if case.family == "route" and mutant is None:
        win = d["rho"][:, d["pi"]].transpose(1, 0, 2)                      # [n_img, heads, S]: rho_h(pi_i(r))
        out = np.take_along_axis(v, win[..., None], axis=2)
    else:
        out = emul
    if mutant == 10:
        ref, emul, out = ref[:, ::-1], emul[:, ::-1], out[:, ::-1]
    if mutant == 11:
        ref, emul, out = ref.copy(), emul.copy(), out.copy()
        ref[-1] = emul[-1] = out[-1] = np.nan
    return Model(qkv, q, k, v, ref, emul, from_heads(np.ascontiguousarray(out), case))


def rel_err(a, b):
    """The whole-tensor metric of tests/test_gpu_ops.py."""
    return float(np.abs(a - b).max() / np.abs(b).max())


def block_ratio(got, ref, emul, dt):
    """Section B's rule per (image, head) block: ||got - ref|| / max(||emul - ref||, 1e-2 u ||ref||) -> [n_img, heads]; the kernel is held to
    F_OP.  (block_err is relative to ||ref||, so the floor is 1e-2 u.)"""
    ek = A.block_err(got, ref)
    yard = np.maximum(A.block_err(emul, ref), 1e-2 * U[dt])
    return ek / yard
