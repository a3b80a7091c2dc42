"""The case table and the inputs of the exact-arithmetic tests of the NT GEMM main loops (tests/test_cpu_gemm_exact.py checks on the
CPU what every case claims, tests/test_gpu_gemm_exact.py runs the same arrays through the kernels), and the split-weight helpers the
tolerance tests of tests/test_gpu_ops.py share with them.  Nothing here touches HIP at import; the three helpers at the bottom take
the loaded library's module as an argument.

THE EXACTNESS CONDITION.  Every operand is q_a x integer and q_w x integer with power-of-two quanta (q = q_a q_w: 1, or 2^-24 for the
`subnormal-lo` family), exactly representable in the operand type (and, for the fp8 correction product, in the kernel's E5M2 image of
A and the packed e4m3 image of lo).  Then every product is q x integer, and so is every partial sum of them taken in ANY order; such a
number is exact in float32 as long as its magnitude stays below 2^24 q.  The magnitude of any partial sum - over any subset of the
terms, of any of the case's products, with the bias and the residual added at any point - is at most

    bound = max over (m, n) of  sum over the case's products of sum_k |a| |w|  +  |bias| + |resid|,

so   bound < 2^24 q   makes the float32 result independent of the summation order, of split-K slabs, of the persistent walk and of the
instruction that forms a product: it EQUALS the float64 `@` of the same arrays, bit for bit.  Any dropped, doubled or misplaced
k-step, row, column or lo product changes an integer.  `build` computes the bound; the CPU test asserts it for every case.

Families
  ints          A, every stored weight block (W; hi and lo independently; w0 and w2 of three products) uniform integers in [-7, 7];
                bias and fp32 residual integers in [-64, 64].  Independent hi and lo: hi used twice, or lo taken at a wrong k, shows.
  ints-fp8      (kind 8, f16) A and hi in [-7, 7] (3 significant bits: exact in E5M2); lo integers in [-15, 15] with every row's
                max |lo| in [8, 15], so ofx_pack_lo8's scale is 2^4 and lo 16 <= 240 has 4 significant bits: exact in e4m3.  Row 3 of
                lo is all zero (scale byte 127).
  subnormal-lo  (f16) weights = integers in [-15, 15] x 2^-24: f16 SUBNORMALS, what the lo halves of real weights are.  Variant "lo":
                hi = 0 (w0 = 0), only the lo block (w2) subnormal; "both": every weight block subnormal.  A in [-7, 7]; bias and
                residual are integers in [-64, 64] x 2^-24 (whole numbers would push the sum past 24 bits of 2^-24).
  census        diagnostic: A = 1, ONE weight block holds W[n, k] = 2^(k div 32), the others 0, no bias, no residual: C / unit has one
                binary digit per 32-column step (unit = 32 x the number of A blocks that meet the block), so a missing or doubled
                step is named by the digit string in the assertion message.

Guards, all in in-bounds memory: A's columns between the last operand block and lda are NaN; a single-product GEMM reading the hi
block of 3 K-wide rows finds OTHER INTEGERS in the two blocks behind it; C is NaN before the launch, and its columns between N and ldc
must still be NaN after it.  A has exactly M rows (the kernels clamp rows past M onto row M - 1)."""
import collections
import functools
import zlib

import numpy as np

Q_SUB = 2.0 ** -24
DTYPES = ("bf16", "f16")
KNOB_NAMES = {2: "kernel", 5: "splitk", 11: "w2_persist", 15: "x3_kernel", 16: "x3_persist", 18: "epi_direct"}      # ofx_tune knob -> tests/gemm_plan_ref.py KNOBS key
KNOB_DEFAULTS = {2: 0, 5: 1, 11: -1, 15: 1, 16: 1, 18: 1}

# name      free-form, unique
# api       gemm | splitk | w2 | w2f8 | x3 (the ofx_gemm* entry point); K is the LOGICAL depth (W rows are K, 2 K, 3 K wide)
# a3k       gemm / splitk only: A's rows are 3 K wide blocks [A | other integers | other integers]
# lda, ldc  0 = the natural stride (K or 3 K; N)
# resid     none | inplace (C holds the residual, ldr = ldc) | separate (its own buffer of row stride ldr)
# variant   subnormal-lo: lo | both; census: the block that carries the powers of two (w | hi | lo | w0 | w2)
# knobs     ((knob, value), ...) of ofx_tune, everything else at its default
# plan      the launch the case is MEANT for: (kind, tile_m, tile_n, splits, grid_x), stated here from the kernels' documentation -
#           tests/test_cpu_gemm_exact.py holds tests/gemm_plan_ref.py's gemm_plan to it
Case = collections.namedtuple("Case", "name api family dt M N K knobs a3k lda ldc resid ldr bias variant plan")


def _case(name, api, family, dt, M, N, K, knobs, plan, a3k=False, lda=0, ldc=0, resid="inplace", ldr=0, bias=True, variant=""):
    if family == "census":
        resid, bias = "none", False
    return Case(f"{name}-{family}{'-' + variant if variant else ''}-{dt}-{M}x{N}x{K}", api, family, dt, M, N, K, tuple(knobs), a3k, lda, ldc,
                resid, ldr, bias, variant, plan)


# ofx_tune(2, v) -> the single-product kernel's tile (csrc/gemm_plan.h: GemmKind)
TILE = {1: (128, 128), 5: (64, 128), 2: (256, 256), 3: (256, 128), 4: (256, 256)}
# (k-tiles, forced slices) -> slices after "every slice owns at least one k-tile": (5, 2) -> 3 + 2, (7, 3) -> 3 + 3 + 1,
# (17, 16) -> 9 slices of 2 with a last one of 1, (48, 5) -> 4 x 10 + 8
SPLITK = {(2, 2): 2, (5, 2): 2, (7, 3): 3, (16, 16): 16, (17, 16): 9, (48, 5): 5}
W2_SHAPE, X3_SHAPE = (769, 512), (769, 384)        # 4 x 2 tiles of 256 x 256, 4 x 3 tiles of 256 x 128; the last row panel has ONE live row
W2_GRIDS = {0: 8, 3: 3, 5: 5, -1: 8}               # ofx_tune(11, g) -> blocks: 3 walk 3 / 3 / 2 tiles, 5 walk 2 / 2 / 2 / 1 / 1
X3_GRIDS = {0: 12, 5: 5, 7: 7, -1: 12}
W2_DEPTHS = (64, 128, 192, 256, 320, 768)          # 2, 4, 6, 8, 10, 24 steps of 32: every residue mod 3 (the stage count) twice
W2F8_DEPTHS = (128, 256, 384, 512, 640)            # 1 .. 5 super-steps of 128
X3_DEPTHS = (64, 128, 192, 256, 320)
SMALL_M = (1, 255, 256, 257)
CENSUS_K = 512                                     # 16 steps of 32: 2^15 is exact in f16 and bf16, the sum 32 (2^16 - 1) < 2^24


def _tiles(M, N, tm, tn):
    return ((M + tm - 1) // tm) * (N // tn)


def _single(v, dt):
    """Single-product kernels forced with ofx_tune(2, v) -> {sweep: [cases]}."""
    tm, tn = TILE[v]
    kn = ((2, v),)
    def c(name, M, N, K, **kw):
        return _case(f"k{v}-{name}", "gemm", kw.pop("family", "ints"), dt, M, N, K, kn, (v, tm, tn, 1, _tiles(M, N, tm, tn)), **kw)
    edge = [c("edge", M, N, 192) for M in (1, tm - 1, tm, tm + 1, 2 * tm + 1) for N in (tn, 3 * tn)]
    M, N = tm + 1, 2 * tn
    # 1 k-tile: the prologue alone (the second stage's fill clamped onto tile 0); 2: each stage once; 3 - 5: the stage parity wraps and
    # the tail prefetch is clamped to the last k-tile; 8, 24: the steady state
    depth = [c("depth", M, N, 64 * d) for d in (1, 2, 3, 4, 5, 8, 24)]
    strides = [c("lda+8", M, N, 192, lda=192 + 8), c("lda3k", M, N, 192, a3k=True), c("ldc+4", M, N, 192, ldc=N + 4),
               c("ldr+4", M, N, 192, resid="separate", ldr=N + 4), c("plain", M, N, 192, resid="none", bias=False),
               c("census", M, N, CENSUS_K, family="census", variant="w")]
    return {"edge": edge, "depth": depth, "strides": strides}


def _splitk(tile_m, dt):
    """ofx_gemm_splitk with a forced plan.  128-row tiles: ofx_tune(2, 1) and ofx_tune(5, s).  64-row tiles: bit 8 of knob 5 is honoured
    only where the planner may choose the tile height - the automatic kernel choice (which is kind 1 at these shapes) and M > 64 - so
    M = 65, 129 leave knob 2 alone, and M = 1 forces the 64-row kernel itself (ofx_tune(2, 5))."""
    out = []
    for (nkt, s), sp in SPLITK.items():
        for M in (1, 65, 129):
            if tile_m == 128:
                kn, kind = ((2, 1), (5, s)), 1
            elif M > 64:
                kn, kind = ((5, s | 256),), 1
            else:
                kn, kind = ((2, 5), (5, s | 256)), 5
            out.append(_case(f"splitk{tile_m}-{nkt}by{s}", "splitk", "ints", dt, M, 256, 64 * nkt, kn, (kind, tile_m, 128, sp, _tiles(M, 256, tile_m, 128))))
    return out


def _wrap(dt):
    """Split weights on the 128 x 128 kernel with a wrapping A index (ofx_gemm_w2, no kernel forced: fewer than 256 big tiles).  Left to
    itself the planner takes 64-row tiles on these grids from M = 65 on, so both heights are forced through knob 5 (no slab is given: the
    slice count of the forced plan collapses to 1): ofx_tune(5, 2) = 128 rows, ofx_tune(5, 257) = 64 rows - which the planner honours
    for M > 64 only, M = 1 stays a 128-row launch."""
    out = []
    for k5 in (2, 257):
        for K in (64, 128, 192):
            for M in (1, 65, 129):
                tm = 64 if (k5 == 257 and M > 64) else 128
                out.append(_case(f"wrap{'64' if k5 == 257 else '128'}", "w2", "ints", dt, M, 256, K, ((5, k5),), (1, tm, 128, 1, _tiles(M, 256, tm, 128))))
    M, N = 129, 256
    kn, pl = ((5, 2),), (1, 128, 128, 1, _tiles(M, N, 128, 128))
    out.append(_case("wrap128-plain", "w2", "ints", dt, M, N, 128, kn, pl, resid="none", bias=False))
    out.append(_case("wrap-planned", "w2", "ints", dt, M, N, 128, (), (1, 64, 128, 1, _tiles(M, N, 64, 128))))       # every knob at its default
    out += [_case("wrap128", "w2", "census", dt, M, N, CENSUS_K, kn, pl, variant=b) for b in ("hi", "lo")]
    if dt == "f16":
        out += [_case("wrap128", "w2", "subnormal-lo", dt, M, N, 128, kn, pl, variant=v) for v in ("lo", "both")]
        out += [_case("wrap64", "w2", "subnormal-lo", dt, M, N, 128, ((5, 257),), (1, 64, 128, 1, _tiles(M, N, 64, 128)), variant=v) for v in ("lo", "both")]
    return out


def _w2(dt, K):
    """The dual-weight 256 x 256 kernel (kind 6, ofx_tune(2, 6)), three stages of 32-deep steps, persistent grids."""
    M, N = W2_SHAPE
    out = [_case(f"w2-g{g}", "w2", "ints", dt, M, N, K, ((2, 6), (11, g)), (6, 256, 256, 1, grid)) for g, grid in W2_GRIDS.items()]
    if K == 128:
        out += [_case("w2-smallM", "w2", "ints", dt, m, 256, K, ((2, 6),), (6, 256, 256, 1, _tiles(m, 256, 256, 256))) for m in SMALL_M]
        out.append(_case("w2-plain", "w2", "ints", dt, M, N, K, ((2, 6), (11, 3)), (6, 256, 256, 1, 3), resid="none", bias=False))
    if K == 192 and dt == "f16":
        out += [_case("w2-g3", "w2", "subnormal-lo", dt, M, N, K, ((2, 6), (11, 3)), (6, 256, 256, 1, 3), variant=v) for v in ("lo", "both")]
    if K == 768:
        out += [_case("w2", "w2", "census", dt, 257, 256, CENSUS_K, ((2, 6),), (6, 256, 256, 1, 2), variant=b) for b in ("hi", "lo")]
    return out


def _w2f8(K, family, variant=""):
    """The fp8-correction kernel (kind 8: kind 6 given the fp8 copy of lo; f16 only), four stages, 128-deep super-steps; both settings
    of ofx_tune(18, v) (which epilogue an operand-type output takes: an fp32 output must not care)."""
    M, N = W2_SHAPE
    out = [_case(f"w2f8-g{g}-e{e}", "w2f8", family, "f16", M, N, K, ((2, 6), (11, g), (18, e)), (8, 256, 256, 1, grid), variant=variant)
           for g, grid in W2_GRIDS.items() for e in (1, 0)]
    if K == 128:
        out += [_case("w2f8-smallM", "w2f8", family, "f16", m, 256, K, ((2, 6),), (8, 256, 256, 1, _tiles(m, 256, 256, 256)), variant=variant) for m in SMALL_M]
    if K == 256 and family == "ints-fp8":
        out.append(_case("w2f8-plain", "w2f8", family, "f16", M, N, K, ((2, 6), (11, 3)), (8, 256, 256, 1, 3), resid="none", bias=False))
    if K == 512 and family == "ints-fp8":
        out += [_case("w2f8", "w2f8", "census", "f16", 257, 256, CENSUS_K, ((2, 6),), (8, 256, 256, 1, 2), variant=b) for b in ("hi", "lo")]
    return out


def _x3(dt, K):
    """Three products (A rows [a0 | a1 | a0], W rows [w0 | w0 | w2], the duplicated blocks really equal): gemm_x3_kernel (kind 9,
    ofx_tune(15, 2)) over its grids, and the K-concatenated path (ofx_tune(15, 0): here the 128 x 128 kernel, whose planner takes
    64-row tiles on this 21-tile grid) on the same buffers."""
    M, N = X3_SHAPE
    out = [_case(f"x3-g{g}", "x3", "ints", dt, M, N, K, ((15, 2), (11, g)), (9, 256, 128, 1, grid)) for g, grid in X3_GRIDS.items()]
    out.append(_case("x3-blockpertile", "x3", "ints", dt, M, N, K, ((15, 2), (16, 0)), (9, 256, 128, 1, 12)))
    out.append(_case("x3-concat", "x3", "ints", dt, M, N, K, ((15, 0),), (1, 64, 128, 1, _tiles(M, N, 64, 128))))
    if K == 128:
        out.append(_case("x3-plain", "x3", "ints", dt, M, N, K, ((15, 2), (11, 5)), (9, 256, 128, 1, 5), resid="none", bias=False))
        # the single-product big kernels at depth 3 K with lda = 3 K
        out += [_case(f"x3-concat-k{v}", "x3", "ints", dt, 257, 512, K, ((15, 0), (2, v)), (v, 256, TILE[v][1], 1, _tiles(257, 512, 256, TILE[v][1]))) for v in (2, 3, 4)]
    if K == 192 and dt == "f16":
        out += [_case("x3-g5", "x3", "subnormal-lo", dt, M, N, K, ((15, 2), (11, 5)), (9, 256, 128, 1, 5), variant=v) for v in ("lo", "both")]
    if K == 320:
        out += [_case("x3", "x3", "census", dt, 257, N, CENSUS_K, ((15, 2),), (9, 256, 128, 1, 6), variant=b) for b in ("w0", "w2")]
    return out


def _groups():
    g = {}
    for dt in DTYPES:
        for v in (1, 2, 3, 4, 5):
            for sweep, cases in _single(v, dt).items():
                g[f"k{v}-{sweep}-{dt}"] = cases
        for tm in (128, 64):
            g[f"splitk{tm}-{dt}"] = _splitk(tm, dt)
        g[f"wrap-{dt}"] = _wrap(dt)
        for K in W2_DEPTHS:
            g[f"w2-K{K}-{dt}"] = _w2(dt, K)
        for K in X3_DEPTHS:
            g[f"x3-K{K}-{dt}"] = _x3(dt, K)
    for K in W2F8_DEPTHS:
        g[f"w2f8-K{K}-ints"] = _w2f8(K, "ints-fp8")
        g[f"w2f8-K{K}-subnormal"] = _w2f8(K, "subnormal-lo", "lo") + _w2f8(K, "subnormal-lo", "both")
    return g


GROUPS = _groups()       # one GPU test per group: a handful of launches on buffers of at most a few MB
CASES = [c for cs in GROUPS.values() for c in cs]
assert len({c.name + repr(c.knobs) for c in CASES}) == len(CASES)


def census_unit(case):
    """What one 32-column step contributes to C per unit of its power of two: 32 ones of A, from each A block that meets the block."""
    return 64.0 if case.variant == "w0" else 32.0


def census_digits(value, case):
    """C / unit as a binary digit string, step 0 first; anything that is no whole number of units is shown as it is."""
    u = value / census_unit(case)
    if not np.isfinite(u) or u != np.floor(u) or u < 0 or u >= 2.0 ** 40:
        return repr(float(value))
    return format(int(u), f"0{case.K // 32}b")[::-1]


def _ints(g, shape, lim):
    return g.integers(-lim, lim + 1, size=shape).astype(np.float32)


@functools.lru_cache(maxsize=4)
def _arrays(api, family, M, N, K, a3k, lda, ldc, resid, ldr, bias, variant):
    """The arrays of a case; they do not depend on the operand type, the knobs or the name, so the grids of one shape share them.
    READ-ONLY for the callers."""
    g = np.random.default_rng(zlib.crc32(repr((api, family, M, N, K, a3k, variant)).encode()))
    na = 3 if (api == "x3" or a3k) else 1
    nw = {"gemm": 1, "splitk": 1, "w2": 2, "w2f8": 2, "x3": 3}[api]
    lda = lda or na * K
    ldc = ldc or N
    qw = Q_SUB if family == "subnormal-lo" else 1.0
    q = qw
    A = np.full((M, lda), np.nan, np.float32)
    if family == "census":
        a = [np.ones((M, K), np.float32)] * 2
    else:
        a = [_ints(g, (M, K), 7), _ints(g, (M, K), 7)]
    other = _ints(g, (M, K), 7)
    # weight blocks b[0], b[1]: W | hi, lo | w0, w2
    if family == "census":
        pw = np.broadcast_to(np.float32(2.0) ** (np.arange(K) // 32).astype(np.float32), (N, K)).copy()
        first = variant in ("w", "hi", "w0")
        b = [pw if first else np.zeros((N, K), np.float32), np.zeros((N, K), np.float32) if first else pw]
    elif family == "subnormal-lo":
        b = [_ints(g, (N, K), 15) * np.float32(Q_SUB), _ints(g, (N, K), 15) * np.float32(Q_SUB)]
        if variant == "lo":
            b[0] = np.zeros((N, K), np.float32)
    elif family == "ints-fp8":
        lo = _ints(g, (N, K), 15)
        n = np.arange(N)
        lo[n, (5 * n) % K] = (8 + n % 8) * np.where(n % 3 == 0, -1.0, 1.0)          # every row's max |lo| in [8, 15]
        lo[3] = 0.0                                                                  # an all-zero row: scale byte 127
        b = [_ints(g, (N, K), 7), lo]
    else:
        b = [_ints(g, (N, K), 7), _ints(g, (N, K), 7)]
    if api in ("gemm", "splitk"):
        A[:, :K] = a[0]
        if a3k:
            A[:, K:2 * K] = a[1]; A[:, 2 * K:3 * K] = other
        W = b[0]
        prods = [(a[0], b[0])]
    elif api in ("w2", "w2f8"):
        A[:, :K] = a[0]
        W = np.concatenate([b[0], b[1]], 1)
        prods = [(a[0], b[0]), (a[0], b[1])]
    else:
        A[:, :K] = a[0]; A[:, K:2 * K] = a[1]; A[:, 2 * K:3 * K] = a[0]
        W = np.concatenate([b[0], b[0], b[1]], 1)
        prods = [(a[0], b[0]), (a[1], b[0]), (a[0], b[1])]
    assert W.shape == (N, nw * K)
    want = np.zeros((M, N), np.float64)
    bound = np.zeros((M, N), np.float64)
    for x, w in prods:
        want += x.astype(np.float64) @ w.astype(np.float64).T
        bound += np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T
    bias_v = (_ints(g, (N,), 64) * np.float32(q)) if bias else None
    res = None
    if resid != "none":
        res = np.full((M, ldc if resid == "inplace" else ldr), np.nan, np.float32)
        res[:, :N] = _ints(g, (M, N), 64) * np.float32(q)
    if bias_v is not None:
        want += bias_v.astype(np.float64); bound += np.abs(bias_v).astype(np.float64)
    if res is not None:
        want += res[:, :N].astype(np.float64); bound += np.abs(res[:, :N]).astype(np.float64)
    d = dict(A=A, W=W, a=a, b=b, bias=bias_v, resid=res, want=want, bound=float(bound.max()), q=q, lda=lda, ldc=ldc, ldr=(ldc if resid == "inplace" else ldr))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def build(case):
    """-> dict: A [M, lda] and W [N, K | 2 K | 3 K] as float32 (exact in the operand type), a / b the operand blocks, bias [N] or None,
    resid [M, ldr] or None (columns past N NaN), want [M, N] float64 from a plain `@`, bound (see the module text), q, lda, ldc, ldr."""
    return _arrays(case.api, case.family, case.M, case.N, case.K, case.a3k, case.lda, case.ldc, case.resid, case.ldr, case.bias, case.variant)


def plan_inputs(case):
    """-> (GemmShape dict, knob dict) of tests/gemm_plan_ref.py for the launch ofx_gemm* makes of the case."""
    d = build(case)
    mult = {"gemm": 1, "splitk": 1, "w2": 2, "w2f8": 2, "x3": 3}[case.api]
    sh = dict(M=case.M, N=case.N, K=mult * case.K, lda=d["lda"], f16=int(case.dt == "f16"), resid=int(case.resid != "none"))
    if case.api in ("w2", "w2f8"):
        sh["a_wrap"] = case.K
    if case.api == "w2f8":
        sh["has_w8"] = 1
    if case.api == "x3":
        sh["k_mult"] = 3
    if case.api == "splitk":
        sh["can_split"] = 1
    return sh, {KNOB_NAMES[k]: v for k, v in case.knobs}


# ---- split-weight helpers on the device, shared with tests/test_gpu_ops.py.  L = the outfitx_amd._lib module (library loaded).
OP_DTYPE = {"bf16": 1, "f16": 2}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _split_w(L, Wf, dt):
    """fp32 [N, K] -> ([N, 2K] operand-type [hi | lo] via ofx_convert mode 3, float64 value hi + lo)."""
    import torch
    N, K = Wf.shape
    src = torch.from_numpy(np.ascontiguousarray(Wf)).cuda()
    td = torch.bfloat16 if dt == "bf16" else torch.float16
    W2 = torch.empty(N, 2 * K, dtype=td, device="cuda")
    L.check(L.load().ofx_convert(src.data_ptr(), W2.data_ptr(), N, K, 3, OP_DTYPE[dt], _stream()))
    hi = src.to(td)
    lo = (src - hi.float()).to(td)
    assert torch.equal(W2[:, :K], hi) and torch.equal(W2[:, K:], lo)
    return W2, (hi.double() + lo.double()).cpu().numpy()


def _e4m3_decode(b):
    """uint8 ndarray (OCP e4m3fn bit patterns) -> float64 values."""
    b = b.astype(np.int64)
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    return np.where(s == 1, -v, v)


def _pack_lo8(L, W2, N, K):
    """ofx_pack_lo8 on the device; returns (W8 bytes tensor, scale bytes tensor, lo values as the kernel will see them [N, K] float64
    in natural k order = e4m3(byte) 2^-sw, per-row sw)."""
    import torch
    W8 = torch.zeros(N, K, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(N, dtype=torch.uint8, device="cuda")
    L.check(L.load().ofx_pack_lo8(W2.data_ptr(), W8.data_ptr(), sc.data_ptr(), N, K, _stream()))
    torch.cuda.synchronize()
    b = W8.cpu().numpy().reshape(N, K // 128, 4, 4, 8)                 # [n][block][g][s][j] <- k = 32 s + 8 g + j
    nat = _e4m3_decode(b).transpose(0, 1, 3, 2, 4).reshape(N, K)       # [n][block][s][g][j] -> natural k
    scb = sc.cpu().numpy().reshape(N // 128, 16, 8)                    # [(n >> 7)][n & 15][(n >> 4) & 7]
    n = np.arange(N)
    sw = 127 - scb[n >> 7, n & 15, (n >> 4) & 7].astype(np.int64)
    return W8, sc, nat * 2.0 ** (-sw[:, None].astype(np.float64)), sw
