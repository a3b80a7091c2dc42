"""The case table and the inputs of the exact-arithmetic tests of the weight-gradient (TN) GEMM, gemm_tn_kernel with its launcher
ofx_launch_gemm_tn (csrc/gemm_tn.hip), reached through ofx_gemm_tn and ofx_gemm_tn_into: C[m, n] = sum_k A[k, m] B[k, n], both operands
row-major with the contraction index as their ROW.  tests/test_cpu_gemm_tn_exact.py checks on the CPU what every case claims,
tests/test_gpu_gemm_tn_exact.py runs the same arrays through the kernel.  Nothing here touches HIP at import.

THE EXACTNESS CONDITION.  Operands are integers in [-7, 7], exact in bf16 and f16; the values C holds before an `accumulate` launch
(the prefill) are integers in [-64, 64].  Every product is an integer, and so is every partial sum of products taken in ANY order,
within one accumulator or across split-K planes, with the prefill added at any point.  The magnitude of any such sum is at most

    bound = max over (m, n) of  sum_k |a[k, m]| |b[k, n]|  +  |prefill[m, n]|,

and an integer below 2^24 is exact in float32.  So   bound < 2^24   makes the float32 result independent of the summation order, of the
split count and of the k-partition: it EQUALS `a64.T @ b64 (+ prefill)` of the live rows, bit for bit.  A dropped, doubled or misplaced
k-row, k-tile, tile row, column or plane changes an integer.  `build` computes the bound; the CPU test asserts it for every case.

Families
  ints     the integer operands above.
  census   diagnostic: A = 1, B[k, n] = 2^(k div 32), K = 512, no accumulate: C / 32 has one binary digit per 32-deep k-step (the unit
           of one MFMA pass; a 64-deep k-tile is two digits), so a missing or doubled half-tile is named by the digit string in the
           assertion message.

Guards, all in in-bounds memory.  Both operand buffers have exactly round_up(K, 64) rows (the contract of include/ofx.h).  Rows at or
past the live count - min(k_dev, K) where a device-side count is given, else K - hold NaN (even rows) and +Inf / -Inf (odd rows,
alternating), inside the last live k-tile and in the tiles wholly past it: the kernel zero-fills the former in LDS and never reads the
latter.  Columns of A between M and lda, and of B between N and ldb, hold NaN.  C is NaN before a plain launch and holds the prefill
before an `accumulate` one; it is m_valid rows of ldc floats followed by guard rows, and everything outside C[:m_valid, :n_valid] must
come back bit-unchanged.  The split-K slab is NaN and one plane (M N floats) longer than ofx_gemm_tn_ws says: the first `splits` planes
must come back finite (every split writes its whole plane; an empty split writes zeros), the last one still NaN."""
import collections
import functools
import zlib

import numpy as np

from gemm_exact_cases import CENSUS_K, DTYPES, OP_DTYPE, census_digits      # noqa: F401  (re-exported to the two test files)

# name       free-form, unique
# entry      tn (ofx_gemm_tn) | into (ofx_gemm_tn_into)
# K          the static depth handed to the launcher; kdev: None, or the value of the device-side live row count
# lda, ldb   0 = M, N;   ldc: 0 = N
# slab       a split-K slab is passed (the launcher then splits as gemm_tn_splits says), else NULL = one split
# m_valid, n_valid, accumulate    ofx_gemm_tn_into's arguments (0 = all)
# What the case is MEANT to reach, stated here from the kernel's documentation and held to it by the CPU test:
# splits     the launcher's split count;   blocks = tile rows x tile columns x splits
# parts      k-tiles owned by each split under the kernel's device-side partition of the LIVE rows
# tail       None, or (split, rows): the split that owns the partial last k-tile and how many live rows that tile has
# variant    unused but for census_digits of tests/gemm_exact_cases.py ("b": one unit is 32 ones of A)
Case = collections.namedtuple("Case", "name entry family dt M N K kdev lda ldb ldc slab m_valid n_valid accumulate splits blocks parts tail variant")


def round_up(x, m):
    return (x + m - 1) // m * m


def live_rows(c):
    return c.K if c.kdev is None else min(c.kdev, c.K)


def tn_partition(live, splits):
    """The kernel's documented k-partition: nkt = ceil(live / 64) k-tiles, per = ceil(nkt / splits), split s owns the k-tiles
    [s per, min(nkt, (s + 1) per)).  -> (k-tiles per split, None or (the split that owns the partial last tile, its live rows))."""
    nkt = (live + 63) // 64
    per = (nkt + splits - 1) // splits
    parts = tuple(max(0, min(nkt, (s + 1) * per) - s * per) for s in range(splits))
    tail = ((nkt - 1) // per, live % 64) if live % 64 else None
    return parts, tail


def _case(name, dt, M, N, K, parts, tail=None, slab=False, kdev=None, lda=0, ldb=0, ldc=0, entry="tn", m_valid=0, n_valid=0, accumulate=0,
          family="ints"):
    if m_valid or n_valid or accumulate:
        entry = "into"
    splits = len(parts)
    assert slab or splits == 1
    tag = f"{'slab' if slab else 'direct'}{'' if kdev is None else f'-kdev{kdev}'}{'-acc' if accumulate else ''}"
    ext = f"-lda{lda}-ldb{ldb}" if lda else ""
    ext += f"-mv{m_valid}-nv{n_valid}" if m_valid else ""
    ext += f"-ldc{ldc}" if ldc else ""
    return Case(f"{name}-{family}-{dt}-{entry}-{M}x{N}x{K}-{tag}{ext}", entry, family, dt, M, N, K, kdev, lda or M, ldb or N, ldc or N, slab,
                m_valid, n_valid, accumulate, splits, (M // 256) * (N // 256) * splits, tuple(parts), tail, "b")


# One 256 x 256 tile, no slab: K -> (k-tiles, live rows of a partial last tile).  1 k-tile: the prologue alone, the second stage's fill
# clamped onto tile 0; 2: each stage once; 3 - 5: the stage parity wraps and the tail refill is clamped; 8: the steady state.  The
# partial tiles are 1, 8 and 63 rows deep (63, 56 and 1 rows zero-filled in LDS).
DEPTHS = {1: (1, 1), 63: (1, 63), 64: (1, 0), 65: (2, 1), 128: (2, 0), 192: (3, 0), 200: (4, 8), 256: (4, 0), 320: (5, 0), 512: (8, 0)}
# Tile grids at K = 192, no slab: the group_m = 4 walk over 5 x 1 (a group of 4 and a group of 1), 2 x 3 (one short group), 6 x 2 (a
# full group and a short one of 2) tiles
WALKS = ((1280, 256), (512, 768), (1536, 512))
# Split-K as the launcher plans it: (M, N, K) -> (k-tiles per split, tail)
PLANNED = {(256, 256, 200): ((1, 1, 1, 1), (3, 8)),                    # the shape of test_gpu_bwd_ops.py::test_gemm_tn_into
           (256, 256, 1088): ((2,) * 8 + (1,), None),                  # 17 k-tiles over 9 splits
           (1280, 768, 576): ((3, 3, 3), None),                        # 45 blocks: no multiple of the 8 XCDs
           (1280, 768, 1024): ((4, 4, 4, 4), None),
           (1280, 768, 1100): ((6, 6, 6), (2, 12)),                    # 18 k-tiles, the last 12 rows deep
           (1536, 1536, 1024): ((8, 8), None)}                         # 72 blocks
# The device-side live row count on 1280 x 768 with static K = 1088 (3 splits with the slab): k_dev -> (k-tiles per split, tail)
LIVE_SHAPE = (1280, 768, 1088)
LIVE = {0: ((0, 0, 0), None), 1: ((1, 0, 0), (0, 1)), 63: ((1, 0, 0), (0, 63)), 64: ((1, 0, 0), None),
        65: ((1, 1, 0), (1, 1)),                                       # split 1's only tile is 1 row deep, split 2 is empty
        129: ((1, 1, 1), (2, 1)),
        300: ((2, 2, 1), (2, 44)),                                     # per = 2, the last split owns one 44-row tile
        576: ((3, 3, 3), None), 1087: ((6, 6, 5), (2, 63)), 1088: ((6, 6, 5), None),
        5000: ((6, 6, 5), None)}                                       # clamps to K
LIVE_DIRECT = {0: ((0,), None), 65: ((2,), (0, 1)), 300: ((5,), (0, 44))}
# A split that starts at an ODD k-tile, owns an EVEN number of them and ends in a partial one: on the 4-split plan of K = 1024, 650 live
# rows are 11 k-tiles, per = 3, and split 3 owns tiles 9 and 10, the last 10 rows deep.  A stage parity taken from the absolute k-tile
# index visits every tile of such a split once all the same, in swapped pairs - only the zero-fill then lands on the stage that holds
# tile 9 and the NaN rows of tile 10 are read.  (An odd start with an odd count, as split 1 of the 3 x 3 plan, ends on the right tile.)
LIVE_ODD = ((1280, 768, 1024), 650, (3, 3, 3, 2), (3, 10))
# Valid extent: the cut at row 1100 is in tile row 4 (of 5), the one at column 700 in tile column 2 (of 3)
INTO_SHAPE = (1280, 768)
INTO_VALID = (1100, 700)


def _groups():
    g = {}
    for dt in DTYPES:
        g[f"depth-{dt}"] = [_case("depth", dt, 256, 256, K, (nkt,), (0, rem) if rem else None) for K, (nkt, rem) in DEPTHS.items()]
        M, N = WALKS[0]
        g[f"walk-{dt}"] = ([_case("walk", dt, M, N, 192, (3,)) for M, N in WALKS]
                           + [_case("walk", dt, M, N, 192, (3,), lda=M + 8, ldb=N + 16, ldc=N + 4)])      # A's rows 16-byte, not 32-byte aligned
        # every planned split next to the unsplit launch of the same arrays
        g[f"planned-{dt}"] = [c for (M, N, K), (parts, tail) in PLANNED.items()
                              for c in (_case("planned", dt, M, N, K, parts, tail, slab=True),
                                        _case("planned", dt, M, N, K, (sum(parts),), (0, tail[1]) if tail else None))]
        M, N, K = LIVE_SHAPE
        g[f"live-{dt}"] = ([_case("live", dt, M, N, K, parts, tail, slab=True, kdev=kd) for kd, (parts, tail) in LIVE.items()]
                           + [_case("live", dt, M, N, K, parts, tail, kdev=kd) for kd, (parts, tail) in LIVE_DIRECT.items()])
        (M, N, K), kd, parts, tail = LIVE_ODD
        g[f"live-{dt}"].append(_case("live-odd", dt, M, N, K, parts, tail, slab=True, kdev=kd))
        M, N = INTO_SHAPE
        mv, nv = INTO_VALID
        into = []
        for ldc in (nv, N + 4):                                       # ldc = n_valid < N;  ldc > N
            for K, slab, parts in ((192, False, (3,)), (576, True, (3, 3, 3))):
                into += [_case("into", dt, M, N, K, parts, slab=slab, m_valid=mv, n_valid=nv, ldc=ldc, accumulate=acc) for acc in (0, 1)]
        into.append(_case("into", dt, M, N, 576, (2, 2, 1), (2, 44), slab=True, kdev=300, m_valid=mv, n_valid=nv, ldc=nv, accumulate=1))
        into.append(_case("into", dt, M, N, 576, (0, 0, 0), slab=True, kdev=0, m_valid=mv, n_valid=nv, ldc=nv, accumulate=1))    # C stays the prefill
        into.append(_case("into", dt, M, N, 192, (0,), kdev=0, m_valid=mv, n_valid=nv, ldc=nv, accumulate=1))
        g[f"into-{dt}"] = into
        # the two entry points on the same arrays, direct and through the slab
        g[f"entry-{dt}"] = [_case("entry", dt, M, N, 576, parts, slab=slab, entry=e)
                            for slab, parts in ((False, (9,)), (True, (3, 3, 3))) for e in ("tn", "into")]
        g[f"census-{dt}"] = [_case("census", dt, 256, 256, CENSUS_K, (8,), family="census"),
                             _case("census", dt, 256, 256, CENSUS_K, (1,) * 8, slab=True, family="census"),
                             _case("census", dt, 1280, 768, CENSUS_K, (8,), family="census")]
    return g


GROUPS = _groups()       # one GPU test per group: a few launches on operands of at most a few MB
CASES = [c for cs in GROUPS.values() for c in cs]
assert len({c.name for c in CASES}) == len(CASES)


def _ints(g, shape, lim):
    return g.integers(-lim, lim + 1, size=shape).astype(np.float32)


def _poison_rows(buf, live):
    """Rows at or past the live count: NaN on even rows, +Inf / -Inf alternating on the odd ones."""
    r = np.arange(live, buf.shape[0])
    buf[r[r % 2 == 0]] = np.nan
    buf[r[r % 4 == 1]] = np.inf
    buf[r[r % 4 == 3]] = -np.inf


@functools.lru_cache(maxsize=4)
def _arrays(family, M, N, K, live, lda, ldb, ldc, m_valid, n_valid, accumulate):
    """The arrays of a case; they depend neither on the operand type nor on the entry point nor on the slab, so those launches share
    them.  READ-ONLY for the callers."""
    g = np.random.default_rng(zlib.crc32(repr((family, M, N, K)).encode()))         # the same integers under every live count
    Kp = round_up(K, 64)
    if family == "census":
        a = np.ones((K, M), np.float32)
        b = np.broadcast_to((np.float32(2.0) ** (np.arange(K) // 32).astype(np.float32))[:, None], (K, N)).copy()
    else:
        a, b = _ints(g, (K, M), 7), _ints(g, (K, N), 7)
    a, b = a[:live], b[:live]
    A = np.full((Kp, lda), np.nan, np.float32)
    B = np.full((Kp, ldb), np.nan, np.float32)
    A[:live, :M] = a
    B[:live, :N] = b
    _poison_rows(A[:, :M], live)
    _poison_rows(B[:, :N], live)
    mv, nv = m_valid or M, n_valid or N
    want = (a.astype(np.float64).T @ b.astype(np.float64))[:mv, :nv]
    bound = (np.abs(a).astype(np.float64).T @ np.abs(b).astype(np.float64))[:mv, :nv]
    prefill = None
    if accumulate:
        prefill = _ints(np.random.default_rng(zlib.crc32(repr((M, N, ldc)).encode())), (mv, ldc), 64)
        want = want + prefill[:, :nv]
        bound = bound + np.abs(prefill[:, :nv])
    d = dict(A=A, B=B, a=a, b=b, prefill=prefill, want=want, full=None, bound=float(bound.max()) if bound.size else 0.0, live=live)
    if m_valid or n_valid or accumulate:
        d["full"] = a.astype(np.float64).T @ b.astype(np.float64)                   # what the slab planes sum to: the whole M x N product
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def plane_wants(case, d):
    """What each split-K plane must hold: the float64 product over the rows of the k-tiles `tn_partition` gives that split (zeros for an
    empty one), the whole M x N of it whatever the valid extent.  -> [splits, M, N] float64."""
    parts, _ = tn_partition(d["live"], case.splits)
    out = np.zeros((case.splits, case.M, case.N), np.float64)
    k0 = 0
    for s, nkt in enumerate(parts):
        k1 = min(d["live"], k0 + 64 * nkt)
        if k1 > k0:
            out[s] = d["a"][k0:k1].astype(np.float64).T @ d["b"][k0:k1].astype(np.float64)
        k0 = k1
    return out


def build(case):
    """-> dict: A [round_up(K, 64), lda] and B [.., ldb] as float32 (the live integers exact in the operand type, the rest guards), a / b
    the live blocks [live, M] / [live, N], prefill [m_valid, ldc] or None, want [m_valid, n_valid] float64 from a plain `@` (+ prefill),
    full [M, N] (the product without the valid extent; None where want is that already), bound (see the module text), live."""
    c = case
    return _arrays(c.family, c.M, c.N, c.K, live_rows(c), c.lda, c.ldb, c.ldc, c.m_valid, c.n_valid, c.accumulate)
