"""The case table, the inputs and a float64 model of the exact, per-route tests of the FORWARD GEMM epilogues
(tests/test_cpu_gemm_epilogue_exact.py checks on the CPU what every case claims and that the suite is sharp - the mutants below -,
tests/test_gpu_gemm_epilogue_exact.py runs the same arrays through the kernels).  Nothing here touches HIP at import.

The operands come from tests/gemm_exact_cases.py (`ints`, `ints-fp8`: integers in [-7, 7], lo in [-15, 15]), built once for the largest
row count of a shape and cut to the case's M, so that every route of one operand set sees THE SAME accumulator on the rows it has: the
accumulator is exact (that file's condition) whatever the kernel's summation order.  Row ZERO_ROW of A is zero: an all-zero accumulator
row, on which the pre-activation IS the bias.  Operand sets: g = one product (ofx_gemm, ofx_gemm_splitk, ofx_gemm_fold w_form 0),
w = split weights whose lo block is exact in e4m3 (ofx_gemm_w2, ofx_gemm_w2f8 and the fold entries on them: hi + lo in f16 and
hi + fp8(lo) give the same integers), x = three products (ofx_gemm_x3).

Parts (the `part` of a case)
  A1  out_kind 1, act none, integer bias of a wide range (+ integer residual): every output bit is torch's cast of the float64 value
  A2  planted elements: resid = target - z - bias, target walking TARGETS over every (row mod 16, column mod 64) position
  A3  out_kind 2: [hi | lo | hi]
  A4  fp32 output, separate residual of its own stride, no bias (RAMP 1 of epilogue2); A4b: fp32, bias, no residual (RAMP 0)
  A5  LayerNorm-fold consumer on the lattice: integer col_sum, integer mean, rstd a power of two, integer bias
  B   the same chains on real-valued constants: bias, residual, mean, rstd, col_sum arbitrary fp32 numbers, the accumulator still exact
  C   activations: operands in quanta of 2^-3, A dense in its first 3 columns only (so the accumulator spreads by about one unit
      around the column's bias), bias a multiple of 2^-6 placed per column (sweep_bias)

THE EXACTNESS CONDITION of the lattice parts.  z, bias, resid are integers, so is every partial sum, bound < 2^24.  Fold: col_sum mean
is an integer, (z - col_sum mean) rstd a multiple of 1/4 and so is the sum with the bias: exact, contracted into FMAs or not, while
(|z| + |col_sum mean|) max(rstd, 1) + |bias| < 2^22 = 2^24 / 4.  Part C: u = z + bias is a multiple of 2^-6 below 2^18 2^-6.

-0.0 is NOT among the pre-activations or the planted targets, although the issue names it: the accumulator of a zero row is +0 (the
MFMA starts from +0), x + (-x) = +0 under round-to-nearest and +0 + -0 = +0, so no input of an op-level entry produces a -0 there.
-0 OUTPUTS are covered: QuickGELU and Mish return -0 in the far negative tail, and the casts must keep the sign."""
import collections
import functools
import zlib

import numpy as np

import gemm_exact_cases as X

N0, K0 = 256, 128
ZERO_ROW = 2
F_ACT = 4.0                                   # the issue's factor on the emulation's own error
FLT_MIN = float(np.finfo(np.float32).tiny)    # the floor: flushed results in the far tails
POISON32, POISON16 = 0x7FC0BEEF, 0x7FE5       # payload NaNs (0x7fe5 is a NaN in f16 and in bf16)

# name     unique
# api      gemm | splitk | w2 | w2f8 | x3: the ofx_gemm* entry (fold cases go through ofx_gemm_fold / ofx_gemm_w2f8_fold on the same route)
# knobs    ofx_tune pairs that force the kernel
# kind     GemmKind the launch must record; tm, tn its tile; direct: ofx_tune(18, 1) on kind 8
# oset     the operand set (module text); w_form: what ofx_gemm_fold is given on this route (None: no fold entry reaches it)
Route = collections.namedtuple("Route", "name api knobs kind tm tn direct dts oset w_form")
BOTH = ("bf16", "f16")
ROUTES = collections.OrderedDict((r.name, r) for r in [
    Route("k1", "gemm", ((2, 1),), 1, 128, 128, 0, BOTH, "g", 0),                # R1: `epilogue`, 128-row tiles
    Route("k5", "gemm", ((2, 5),), 5, 64, 128, 0, BOTH, "g", 0),                 # R1: 64-row tiles (nrows = 32 per wave)
    Route("wrap", "w2", ((5, 2),), 1, 128, 128, 0, BOTH, "w", 1),                # R1: split weights left on the 128 x 128 kernel
    Route("k2", "gemm", ((2, 2),), 2, 256, 256, 0, BOTH, "g", 0),                # R2 / R3: epilogue2, NP 8 / JW 4
    Route("k3", "gemm", ((2, 3),), 3, 256, 128, 0, BOTH, "g", 0),
    Route("k4", "gemm", ((2, 4),), 4, 256, 256, 0, BOTH, "g", 0),
    Route("k6", "w2", ((2, 6),), 6, 256, 256, 0, BOTH, "w", 1),
    Route("k9", "x3", ((15, 2),), 9, 256, 128, 0, BOTH, "x", None),              # NP 4 / JW 4
    Route("k8", "w2f8", ((2, 6), (18, 0)), 8, 256, 256, 0, ("f16",), "w", 2),    # NP 4 / JW 8, J0 0 and 4, constants from the cst slot
    Route("k8d", "w2f8", ((2, 6), (18, 1)), 8, 256, 256, 1, ("f16",), "w", 2),   # R4 where the call admits it, else epilogue2 again
    Route("splitk", "splitk", ((2, 1), (5, 2)), 1, 128, 128, 0, BOTH, "g", None),  # R5: two slices, splitk_reduce_kernel
])
KNOB_DEFAULTS = dict(X.KNOB_DEFAULTS)

# part, route, dt, M, N, K; mode int | real | act (operand scaling and the kind of constants); out_kind, act (ofx_act);
# resid none | separate (its own buffer, ldr = N + 4); ldc = width + 8 always (width = N, 3 N for out_kind 2);
# bias none | wide | real | sweep; fold 0 | 1; stat_ld 1 | 3 (3: rows of the statistics 3 pairs apart and A rows 3 K wide);
# grid: None or the value of ofx_tune(11, v) (the persistent grid whose blocks change tile)
Case = collections.namedtuple("Case", "name part route dt M N K mode out_kind act resid ldc ldr bias fold stat_ld grid")


def _case(part, route, dt, M, mode, out_kind, act, resid, bias, fold=0, stat_ld=1, grid=None, N=N0, K=K0):
    width = 3 * N if out_kind == 2 else N
    name = f"{part}-{route}-{dt}-{M}x{N}x{K}-o{out_kind}-a{act}-r{resid[0]}-b{bias}" + (f"-fold{stat_ld}" if fold else "") + (f"-g{grid}" if grid is not None else "")
    return Case(name, part, route, dt, M, N, K, mode, out_kind, act, resid, width + 8, N + 4 if resid != "none" else 0, bias, fold, stat_ld, grid)


def row_counts(r):
    """One row, a ragged tile, one live row in the second panel (256-row kernels); 1, 65, 129 for the 64- and 128-row tiles."""
    return (1, 255, 257) if r.tm == 256 else (1, 65, 129)


def fold_row_counts(r):
    """+ an even M whose last (ra, rb) pair of the statistics load clamps BOTH rows (254: rows 254, 255 -> 253), beside the odd
    ones where only rb clamps (255) and where the pair is whole (257 = 256 + 1: the second panel's pair (256, 257 -> 256))."""
    return (1, 254, 255, 257) if r.tm == 256 else (1, 64, 65, 129)


def takes_direct(c):
    """Whether the launch leaves through epilogue_direct (epilogue_direct_dispatch, gemm_common.h)."""
    return bool(ROUTES[c.route].direct and c.out_kind == 1 and c.resid == "none" and c.act in (0, 1, 2))


def _cases():
    out = []
    for r in ROUTES.values():
        big = row_counts(r)[-1]
        for dt in r.dts:
            res_ok = ("none", "separate")
            for M in row_counts(r):
                for resid in res_ok:
                    out.append(_case("A1", r.name, dt, M, "int", 1, 0, resid, "wide"))
            for M in (1, big):
                out.append(_case("A2", r.name, dt, M, "int", 1, 0, "separate", "wide"))
            for resid in res_ok:
                out.append(_case("A3", r.name, dt, big, "int", 2, 0, resid, "wide"))
            for M in (1, big):
                out.append(_case("A4", r.name, dt, M, "int", 0, 0, "separate", "none"))
            out.append(_case("A4b", r.name, dt, big, "int", 0, 0, "none", "wide"))
            if r.w_form is not None:
                for M in fold_row_counts(r):
                    out.append(_case("A5", r.name, dt, M, "int", 1, 0, "none", "wide", fold=1))
                if r.w_form != 2:                                  # ofx_gemm_w2f8_fold has no stat_ld argument
                    out.append(_case("A5", r.name, dt, big, "int", 1, 0, "none", "wide", fold=1, stat_ld=3))
                for M in fold_row_counts(r)[1::2]:
                    out.append(_case("B", r.name, dt, M, "real", 1, 0, "none", "real", fold=1))
            for ok in (0, 1, 2):
                for resid in res_ok:
                    out.append(_case("B", r.name, dt, big, "real", ok, 0, resid, "real"))
            for act in (1, 2, 3):
                for ok in (0, 1):
                    for resid in res_ok:
                        out.append(_case("C", r.name, dt, big, "act", ok, act, resid, "sweep"))
    # the persistent grid whose blocks change tile: 4 x 2 tiles on 3 blocks (tests/gemm_exact_cases.py W2_GRIDS), N = 512 so that a
    # block's consecutive tiles differ in their per-tile constants
    M, N = X.W2_SHAPE
    for rn in ("k6", "k8", "k8d"):
        for dt in ROUTES[rn].dts:
            out.append(_case("A1", rn, dt, M, "int", 1, 0, "none", "wide", grid=3, N=N))
            out.append(_case("A5", rn, dt, M, "int", 1, 0, "none", "wide", fold=1, grid=3, N=N))
            out.append(_case("B", rn, dt, M, "real", 1, 0, "none", "real", fold=1, grid=3, N=N))
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def groups():
    """One GPU test per (part, operand set, type): cases that share operands run on one set of device tensors."""
    g = collections.OrderedDict()
    for c in CASES:
        g.setdefault(f"{c.part}-{ROUTES[c.route].oset}-{c.dt}", []).append(c)
    return g


GROUPS = groups()


def knobs(c):
    return ROUTES[c.route].knobs + (((11, c.grid),) if c.grid is not None else ())


def plan(c):
    """(kind, tile_m, tile_n, splits, grid_x) the case is meant for."""
    r = ROUTES[c.route]
    tiles = ((c.M + r.tm - 1) // r.tm) * (c.N // r.tn)
    return (r.kind, r.tm, r.tn, 2 if r.api == "splitk" else 1, c.grid if c.grid is not None else tiles)


def plan_inputs(c):
    """-> (GemmShape dict, knob dict) of tests/gemm_plan_ref.py for the launch the entry point makes of the case."""
    r = ROUTES[c.route]
    mult = {"gemm": 1, "splitk": 1, "w2": 2, "w2f8": 2, "x3": 3}[r.api]
    sh = dict(M=c.M, N=c.N, K=mult * c.K, lda=lda(c), f16=int(c.dt == "f16"), resid=int(c.resid != "none"), out_kind=c.out_kind)
    if r.api in ("w2", "w2f8"):
        sh["a_wrap"] = c.K
    if r.api == "w2f8":
        sh["has_w8"] = 1
    if r.api == "x3":
        sh["k_mult"] = 3
    if r.api == "splitk":
        sh["can_split"] = 1
    return sh, {X.KNOB_NAMES[k]: v for k, v in knobs(c)}


def lda(c):
    return 3 * c.K if (ROUTES[c.route].api == "x3" or c.stat_ld == 3) else c.K


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=16)
def operands(oset, M, N, K, mode, a3k):
    """A [M, lda] and W [N, K | 2 K | 3 K] as float32 (exact in f16 and bf16, A and hi in E5M2, lo in e4m3), z = the exact accumulator
    in float64, absz = sum |a| |w|.  READ-ONLY."""
    api = {"g": "gemm", "w": "w2f8", "x": "x3"}[oset]
    Mb = M if M > 257 else 257
    d = X.build(X.Case("", api, "ints-fp8" if oset == "w" else "ints", "f16", Mb, N, K, (), False, 0, 0, "none", 0, False, "", None))
    q = np.float32(0.125 if mode == "act" else 1.0)
    a = [x[:M].copy() for x in d["a"]]
    for x in a:
        if M > ZERO_ROW:
            x[ZERO_ROW] = 0.0
        if mode == "act":
            x[:, 3:] = 0.0
        x *= q
    b = [w * q for w in d["b"]]
    if oset == "g":
        # a3k: A's rows are [a0 | other integers | other integers]; only the first block is read
        A = np.concatenate([a[0], a[1] + q, a[1] - q], 1) if a3k else a[0]
        W, prods = b[0], [(a[0], b[0])]
    elif oset == "w":
        A = np.concatenate([a[0], a[1] + q, a[1] - q], 1) if a3k else a[0]
        W, prods = np.concatenate([b[0], b[1]], 1), [(a[0], b[0]), (a[0], b[1])]
    else:
        A = np.concatenate([a[0], a[1], a[0]], 1)
        W, prods = np.concatenate([b[0], b[0], b[1]], 1), [(a[0], b[0]), (a[1], b[0]), (a[0], b[1])]
    z = sum(x.astype(np.float64) @ w.astype(np.float64).T for x, w in prods)
    absz = sum(np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T for x, w in prods)
    out = dict(A=np.ascontiguousarray(A, np.float32), W=np.ascontiguousarray(W, np.float32), lo=b[1], z=z, absz=absz, q=float(q))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def wide_bias(dt, N):
    """Integers spread over the binades above 2^11 (f16) / 2^8 (bf16) up to 40,000, both signs: most sums round, the odd ones of the
    first binade are exact ties."""
    g = _rng("wide", dt, N)
    lo = 11.2 if dt == "f16" else 8.2
    mag = np.rint(2.0 ** g.uniform(lo, 15.28, N))
    return (mag * np.where(g.integers(0, 2, N) == 1, 1.0, -1.0)).astype(np.float32)


SWEEP_TAILS = (60.0, -60.0, 100.0, -100.0, 60.5, -61.25, 99.0, -99.0)


def sweep_kind(n):
    return (n // 64 + n % 64) % 4


def sweep_bias(N):
    """Per column, a multiple of 2^-6.  kind = (n div 64 + n mod 64) mod 4, so every column position of a wave tile (n mod 64) meets
    every kind among the column blocks: 0 -> around 0 (and +-1: the accumulator spreads about a unit), 1 -> around the softplus
    threshold 20, 2 -> around -5 (1 + erf cancels), 3 -> -24 + 48 (n mod 64) / 63: the whole of [-24, 24].  Within a kind the offsets
    ((37 n) mod 65 - 32) / 64 differ by column.  Column 0 is exactly 0, column 64 exactly 20 (kind 1): on the zero row the
    pre-activation IS these.  Eight columns of kind 3 carry the far tails SWEEP_TAILS."""
    n = np.arange(N)
    c = n % 64
    off = ((37 * n) % 65 - 32) / 64.0
    centre = np.select([sweep_kind(n) == 0, sweep_kind(n) == 1, sweep_kind(n) == 2], [0.0 + off, 20.0 + off, -5.0 + 2 * off],
                       np.rint((-24.0 + 48.0 * c / 63.0) * 64.0) / 64.0)
    centre[0], centre[64] = 0.0, 20.0
    k3 = n[sweep_kind(n) == 3]
    for i, t in enumerate(SWEEP_TAILS):
        centre[k3[5 + 7 * i]] = t
    assert sweep_kind(0) == 0 and sweep_kind(64) == 1
    return centre.astype(np.float32)


# TARGETS: ties to even in both directions (f16: odd integers of [2^11, 2^12), 4 k + 2 of [2^12, 2^13); bf16: the same three binades
# lower, and 65792 / 66304 above 2^16), the integers one below and one above a tie, the largest finite f16 65504, 65519 (-> 65504),
# 65520 (-> inf in f16: the kernel's conversion must overflow as torch's does), 0.  32 entries: TARGET_CLASS walks them all at every
# (row mod 16, column mod 64) position once the case has 128 rows.
TARGETS = np.array([2049, 2051, -2049, -2051, 4098, 4102, -4098, -4102, 4097, 4099, 4101, 4103, -4097, -4103, 65504, 65519, 65520, -65520,
                    -65519, 0, 257, 259, -257, -259, 514, 518, 513, 515, 517, 519, 65792, 66304], np.float64)


def target_class(M, N):
    m, n = np.arange(M)[:, None], np.arange(N)[None, :]
    return ((m // 16) * 4 + n // 64 + m % 16 + n % 64) % len(TARGETS)


@functools.lru_cache(maxsize=32)
def _inputs(oset, part, dt, M, N, K, mode, bias, resid, fold, stat_ld):
    """Every random constant is drawn for the operand set's largest row count and cut to M (the generator's key does not hold M):
    routes of different tile heights see the same numbers on the rows they share."""
    ops = operands(oset, M, N, K, mode, stat_ld == 3)
    Mb = M if M > 257 else 257
    g = _rng("inputs", oset, part, Mb, N, K, bias, resid, fold)
    d = dict(ops)
    d["bias"] = {"none": None, "wide": wide_bias(dt, N), "real": (3.0 * g.standard_normal(N)).astype(np.float32), "sweep": sweep_bias(N)}[bias]
    bz = np.zeros(N, np.float32) if d["bias"] is None else d["bias"]
    if fold:
        if mode == "int":
            m, n = np.arange(M), np.arange(N)
            mean, rstd = ((5 * m) % 7 - 3).astype(np.float32), np.array([0.25, 0.5, 1.0, 2.0], np.float32)[(m + m // 4) % 4]
            csum = ((7 * n) % 17 - 8).astype(np.float32)
        else:
            mean, rstd = g.standard_normal(Mb).astype(np.float32)[:M], g.uniform(0.5, 2.0, Mb).astype(np.float32)[:M]
            csum = (4.0 * g.standard_normal(N)).astype(np.float32)
        stat = (1000.0 + np.arange(2 * M * stat_ld, dtype=np.float32)).reshape(M * stat_ld, 2)      # decoys between the rows of a strided stream
        stat[::stat_ld, 0], stat[::stat_ld, 1] = mean, rstd
        d.update(mean=mean, rstd=rstd, csum=csum, stat=stat)
    if resid != "none":
        ldr = N + 4
        res = np.full((M, ldr), np.nan, np.float32)
        if part == "A2":
            res[:, :N] = (TARGETS[target_class(M, N)] - ops["z"] - bz.astype(np.float64)).astype(np.float32)
        elif mode == "int":
            res[:, :N] = g.integers(-64, 65, (Mb, N)).astype(np.float32)[:M]
            if M > ZERO_ROW:
                res[ZERO_ROW, :N:3] = 0.0            # zero accumulator + zero residual (+ no bias in A4): the result is 0
        else:
            res[:, :N] = ((5.0 if mode == "real" else 1.0) * g.standard_normal((Mb, N))).astype(np.float32)[:M]
        d["resid"] = res
    else:
        d["resid"] = None
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def inputs(c):
    return _inputs(ROUTES[c.route].oset, c.part, c.dt if c.bias == "wide" else "", c.M, c.N, c.K, c.mode, c.bias, c.resid, c.fold, c.stat_ld)


# ------------------------------------------------------------------------------------------------ number formats
FMT = {"f16": (11, -14, 65504.0), "bf16": (8, -126, float(np.float32(3.3895313892515355e38)))}      # significand bits, emin, largest finite


def _quantum(v, dt):
    p, emin, _ = FMT[dt]
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return 2.0 ** (np.maximum(e, emin) - (p - 1))


def half_ulp(v, dt):
    """Half a unit in the last place of the operand type at |v| (float32: dt = 'f32')."""
    if dt == "f32":
        return 0.5 * np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)
    return 0.5 * _quantum(v, dt)


def rnd(v, dt, how="rne"):
    """float64 -> the operand type's value (as float64): rne round to nearest even | trunc | away (round half away from zero).
    Overflow as IEEE: past the largest finite + half a unit -> inf (rne, away), trunc saturates."""
    v = np.asarray(v, np.float64)
    q = _quantum(np.where(np.isfinite(v), v, 1.0), dt)
    big = FMT[dt][2]
    with np.errstate(invalid="ignore"):
        r = v / q
        if how == "rne":
            r = np.rint(r)
        elif how == "trunc":
            r = np.trunc(r)
        else:
            r = np.sign(r) * np.floor(np.abs(r) + 0.5)
        out = r * q
        if how == "trunc":
            return np.clip(out, -big, big)
        return np.where(np.abs(out) > big, np.copysign(np.inf, v), out)


def torch_cast(v, dt):
    """torch's cast of a float64 / float32 array to the operand type -> int16 bit patterns."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v)).to(torch.float16 if dt == "f16" else torch.bfloat16)
    return t.view(torch.int16).numpy()


def decode(bits, dt):
    """int16 bit patterns of the operand type -> float64."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits)).view(torch.float16 if dt == "f16" else torch.bfloat16).double().numpy()


# ------------------------------------------------------------------------------------------------ activations
def _erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def act_ref(u, act):
    """float64 of the reference's definitions (oracle/np_oracle.py: quick_gelu, gelu, mish with torch's softplus threshold 20)."""
    u = np.asarray(u, np.float64)
    with np.errstate(over="ignore"):
        if act == 1:
            return u / (1.0 + np.exp(-1.702 * u))
        if act == 2:
            return 0.5 * u * (1.0 + _erf(u / np.sqrt(2.0)))
        if act == 3:
            return u * np.tanh(np.where(u > 20, u, np.log1p(np.exp(np.minimum(u, 20)))))
    return u


def act_emul(u, act, variant=""):
    """np.float32 step by step: the formulas of ofx_common.h (act_quick_gelu, act_gelu, act_mish), the same operations in the same
    order, with numpy's exp / exp2, a float64 erf rounded once, and a correctly rounded division where the kernel takes a reciprocal.
    variant: libexp (Mish with a correctly rounded exp: a yardstick the GPU test reports beside the real one), or a defect - qg17 (constant 1.7), tanh (tanh-form GELU), nothr (Mish without the threshold), thr15 (threshold at 15)."""
    f = np.float32
    u = np.asarray(u, f)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if act == 1:
            k = f(-2.4554669595930157) if variant != "qg17" else f(-1.7 * 1.4426950408889634)
            e = np.exp2((k * u).astype(np.float64)).astype(f)
            return (u * (f(1.0) / (f(1.0) + e))).astype(f)
        if act == 2:
            if variant == "tanh":
                t = np.tanh(np.sqrt(2.0 / np.pi) * (u.astype(np.float64) + 0.044715 * u.astype(np.float64) ** 3)).astype(f)
                return ((f(0.5) * u) * (f(1.0) + t)).astype(f)
            er = _erf((u * f(0.70710678118654752)).astype(np.float64)).astype(f)
            return ((f(0.5) * u) * (f(1.0) + er)).astype(f)
        if act == 3:
            thr = {"nothr": np.inf, "thr15": 15.0}.get(variant, 20.0)
            # __expf(u) IS two operations: the fp32 product u log2(e), then the hardware's 2^x (the form act_quick_gelu writes out)
            e = np.exp2((u * f(1.4426950408889634)).astype(np.float64)).astype(f)
            if variant == "libexp":                  # a correctly rounded exp instead: what the bound would be without the product's rounding
                e = np.exp(u.astype(np.float64)).astype(f)
            n = (e * (e + f(2.0))).astype(f)
            y = (u * (n * (f(1.0) / (n + f(2.0))))).astype(f)
            return np.where(u > f(thr), u, y).astype(f)
    return u


def act_bound(u, act, variant=""):
    """Per element: F_ACT x E_act(u) + FLT_MIN, E_act = |emulation - float64| taken as the maximum over the 64 neighbouring sweep points
    (the DISTINCT values of u in order: 32 on each side), never below half an fp32 ulp of the reference value.  -> (ref64, bound),
    shaped like u."""
    u = np.asarray(u, np.float64)
    pts, inv = np.unique(u.ravel(), return_inverse=True)
    ref = act_ref(pts, act)
    err = np.abs(act_emul(pts, act, variant).astype(np.float64) - ref)
    win = np.lib.stride_tricks.sliding_window_view(np.pad(err, 32, mode="edge"), 65).max(axis=1)
    e = np.maximum(win, half_ulp(ref, "f32"))
    return ref[inv].reshape(u.shape), (F_ACT * e + FLT_MIN)[inv].reshape(u.shape)


# ------------------------------------------------------------------------------------------------ the model
VALUE_MUTANTS = ("bias_after_act", "bias_n^4", "bias_n+64", "stat_m^1", "stat_m+1", "rstd_first", "csum_n+16", "resid_ldc", "resid_before_act")
ROUND_MUTANTS = ("trunc", "half_away", "double_round")
SPLIT3_MUTANTS = ("lo_other_element", "third_is_lo", "split3_stride")
STORE_MUTANTS = ("swap8", "soffset_rows")
ACT_MUTANTS = ("qg17", "gelu_tanh", "mish_nothr", "mish_thr15")
MUTANTS = VALUE_MUTANTS + ROUND_MUTANTS + SPLIT3_MUTANTS + STORE_MUTANTS + ACT_MUTANTS


def value(c, d, mut="", FT=np.float64, emul=False):
    """The epilogue's value chain before the store, [M, N] in FT (float64: the reference; float32: every operation rounds, nothing is
    contracted).  emul: the activation is act_emul (float32), else act_ref.  mut: one of VALUE_MUTANTS / ACT_MUTANTS."""
    M, N = c.M, c.N
    m, n = np.arange(M), np.arange(N)
    acc = d["z"].astype(FT)
    bn = {"bias_n^4": n ^ 4, "bias_n+64": (n + 64) % N}.get(mut, n)
    bias = (np.zeros(N, FT) if d["bias"] is None else d["bias"].astype(FT)[bn])[None, :]
    res = None
    if d["resid"] is not None:
        if mut == "resid_ldc":                       # row m read at m ldc instead of m ldr (the pad columns are NaN: read as 0 here)
            flat = np.nan_to_num(d["resid"], nan=0.0).ravel()
            res = flat[np.minimum(m[:, None] * c.ldc + n[None, :], flat.size - 1)].astype(FT)
        else:
            res = d["resid"][:, :N].astype(FT)
    with np.errstate(over="ignore", invalid="ignore"):
        if c.fold:
            sm = {"stat_m^1": np.minimum(m ^ 1, M - 1), "stat_m+1": np.minimum(m + 1, M - 1)}.get(mut, m)
            cn = n ^ 16 if mut == "csum_n+16" else n
            mu, rs, cs = d["mean"].astype(FT)[sm][:, None], d["rstd"].astype(FT)[sm][:, None], d["csum"].astype(FT)[cn][None, :]
            v = (acc * rs - cs * mu) if mut == "rstd_first" else (acc - cs * mu) * rs
            v = v if mut == "bias_after_act" else v + bias
        else:
            v = acc if mut == "bias_after_act" else acc + bias
        if mut == "resid_before_act" and res is not None:
            v = v + res
        if c.act:
            variant = {"qg17": "qg17", "gelu_tanh": "tanh", "mish_nothr": "nothr", "mish_thr15": "thr15"}.get(mut, "")
            ok = (variant == "") or (variant == "qg17" and c.act == 1) or (variant == "tanh" and c.act == 2) or (variant in ("nothr", "thr15") and c.act == 3)
            v = act_emul(v, c.act, variant if ok else "").astype(FT) if emul else act_ref(v, c.act).astype(FT)
        if mut == "bias_after_act":
            v = v + bias
        if mut != "resid_before_act" and res is not None:
            v = v + res
    return v.astype(FT)


def _store_mutant(bits, mut):
    """Defects of epilogue_direct's store on the [M, N] block of 16-bit patterns."""
    M, N = bits.shape
    m, n = np.arange(M)[:, None], np.arange(N)[None, :]
    if mut == "swap8":               # the permlane trade gone wrong: the middle two 8-column groups of every 32 columns change places
        g = (n // 8) % 4
        src = np.where((g == 1) | (g == 2), n ^ 24, n)
        return bits[m, src]
    if mut == "soffset_rows":        # rows 12-15 of every pass but a wave's first take dwords 1 and 3 (columns 2, 3, 6, 7 of 8) from the pass before
        hit = (m % 16 >= 12) & ((m % 64) // 16 >= 1) & np.isin(n % 8, (2, 3, 6, 7))
        return np.where(hit, bits[np.maximum(m - 16, 0), n], bits)
    return bits


def expected(c, d, mut=""):
    """Lattice parts (A*): the output [M, width] the kernel must return - float32 values for out_kind 0, int16 bit patterns of the
    operand type else.  mut: any of MUTANTS (a defect the CPU test must see change this array)."""
    N = c.N
    v = value(c, d, mut if mut in VALUE_MUTANTS else "")
    if c.out_kind == 0:
        return v.astype(np.float32)
    if mut == "trunc":
        hi = rnd(v, c.dt, "trunc")
    elif mut == "half_away":
        hi = rnd(v, c.dt, "away")
    elif mut == "double_round":
        hi = rnd(rnd(v, "bf16" if c.dt == "f16" else "f16"), c.dt)
    else:
        hi = decode(torch_cast(v, c.dt), c.dt)
    hb = _store_mutant(torch_cast(hi, c.dt), mut)
    if c.out_kind == 1:
        return hb
    with np.errstate(invalid="ignore"):
        rem = (v - hi).astype(np.float32)                  # fp32(v - hi): exact here, v and hi are integers below 2^24
    if mut == "lo_other_element":
        rem = (np.roll(v, 1, axis=1) - hi).astype(np.float32)
    lb = torch_cast(rem, c.dt)
    out = np.full((c.M, c.ldc), POISON16, np.uint16).view(np.int16)
    stride = (c.ldc // 3) if mut == "split3_stride" else N
    out[:, :N] = hb
    out[:, stride:stride + N] = lb
    out[:, 2 * stride:2 * stride + N] = lb if mut == "third_is_lo" else hb
    return out[:, :3 * N]


def lattice_bound(c, d):
    """The module text's bound: the largest magnitude any partial sum of the chain can take, in units of the quantum."""
    b = d["absz"].copy()
    if c.fold:
        b = (b + np.abs(d["csum"]).astype(np.float64)[None, :] * np.abs(d["mean"]).astype(np.float64)[:, None]) * np.maximum(d["rstd"].astype(np.float64), 1.0)[:, None]
    if d["bias"] is not None:
        b = b + np.abs(d["bias"]).astype(np.float64)[None, :]
    if d["resid"] is not None:
        b = b + np.abs(d["resid"][:, :c.N]).astype(np.float64)
    return float(b.max()) / (d["q"] ** 2) * (4.0 if c.fold else 1.0)        # fold: the sums are multiples of 1/4


def real_bound(c, d):
    """Part B.  -> (ref64, bound) per element for the fp32 value: one half-ulp per fp32 operation of epi_value / epi_residual, taken at
    the magnitude that operation's result can have (the float64 value plus the error so far), an earlier error scaled by what multiplies
    it.  Plain: s1 = acc + bias, s2 = s1 + resid.  Fold: t1 = cs mu, t2 = acc - t1, t3 = t2 rs, t4 = t3 + bias (a contracted
    evaluation rounds less often).  The operand-type outputs add half an ulp of T at |ref| + bound (out_bound)."""
    acc = d["z"]
    bias = (np.zeros(c.N) if d["bias"] is None else d["bias"].astype(np.float64))[None, :]
    hu = lambda x, e: half_ulp(np.abs(x) + e, "f32")
    if c.fold:
        mu, rs, cs = d["mean"].astype(np.float64)[:, None], d["rstd"].astype(np.float64)[:, None], d["csum"].astype(np.float64)[None, :]
        t1 = cs * mu; e = hu(t1, 0.0)
        t2 = acc - t1; e = e + hu(t2, e)
        t3 = t2 * rs; e = e * np.abs(rs); e = e + hu(t3, e)
        v = t3 + bias; e = e + hu(v, e)
    else:
        v = acc + bias; e = hu(v, 0.0)
    if d["resid"] is not None:
        v = v + d["resid"][:, :c.N].astype(np.float64); e = e + hu(v, e)
    return v, e


def out_bound(ref, e, dt):
    return e + half_ulp(np.abs(ref) + e, dt)
