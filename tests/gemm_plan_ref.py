"""The GEMM launch decision as the launch code made it before it moved into outfitx_amd/csrc/gemm_plan.h, written out in Python from
that code: the dispatcher's kernel choice, its small-problem planner (`plan_small`: tile height x split-K, cost model in float64), the
L2 group size, the 64-row rule, the second-pass route and the profile record's label, as ofx_launch_gemm had them; the tile counts and
grids as each of the five big-tile launchers computed them; the persistent-grid rule that stood in api.hip; and the TN kernel's split
planner.  C integer division of non-negative ints is floor division, and every float expression keeps the C expression's order of
operations, so tests/test_gemm_plan.py asks for EQUALITY with the header on every point, and tests/test_gpu_gemm_plan.py with the
records of real launches."""
from functools import lru_cache

AUTO, K128, K256, K256x128, PP, K64, W2, W2F8, X3 = 0, 1, 2, 3, 4, 5, 6, 8, 9
PASS_NONE, PASS_DEFERRED, PASS_REDUCE_LN, PASS_REDUCE = 0, 1, 2, 3
BM = BN = 128
BK = 64

# ofx_tune knob number -> name, with the defaults
KNOBS = {"kernel": 0, "splitk": 1, "x3_kernel": 1, "x3_persist": 1, "w2_persist": -1, "epi_direct": 1}
# what the decision reads of the problem (GemmShape), with a plain bf16 GEMM's values for all but M, N, K
SHAPE = {"M": 0, "N": 0, "K": 0, "lda": 0, "a_wrap": 0, "k_mult": 1, "f16": 0, "has_w8": 0, "has_m_dev": 0, "can_split": 0, "defer": 0,
         "ln_fusable": 0, "out_kind": 0, "resid": 0, "aux": 0, "xlo": 0}
# the plan, in the order the test program prints it
FIELDS = ("kind", "tile_m", "tile_n", "tiles_m", "tiles_n", "nwg", "group_m", "splits", "kt_per_split", "grid_x", "grid_y", "second_pass",
          "reduce_grid", "epi_direct", "kmul", "k_logical", "flops", "bytes")


def persistent_grid(nwg, persist, has_m_dev, cu_count):
    if persist < 0:
        persist = cu_count
    return persist if (persist and not has_m_dev and nwg > persist) else nwg


@lru_cache(maxsize=None)
def plan_small(M, N, K, allow_split, allow64, splitk):
    """-> (tile64, splits)"""
    nk = K // BK
    if splitk >= 2:
        tile64, splits = (splitk >> 8) & 1, min(splitk & 0xff, 16)
        if tile64 and not allow64:
            tile64 = 0
        if not allow_split or splits > nk:
            splits = 1
        kps = (nk + splits - 1) // splits
        return tile64, (nk + kps - 1) // kps
    best = (0, 1)
    best_cost = 1e30
    for t64 in ((0, 1) if allow64 else (0,)):
        blocks = ((M + (63 if t64 else 127)) // (64 if t64 else 128)) * (N // 128)
        slots = 768 if t64 else 512
        per = 0.65 if t64 else 1.06
        for sp in range(1, 17):
            if sp > 1 and not (allow_split and splitk != 0 and blocks < 256 and nk >= 16 and sp <= nk // 4):
                break
            kps = (nk + sp - 1) // sp
            if (nk + kps - 1) // kps != sp:
                continue
            t = float((blocks * sp + slots - 1) // slots) * kps * per + (1.0 if t64 else 0.0)
            if sp > 1:
                t += 2.0 * sp * M * N * 4.0 / 5.0e6 + 3.0
            if t < best_cost:
                best, best_cost = (t64, sp), t
    return best


def splitk_bytes(M, N, K, splitk=1):
    sp = max(plan_small(M, N, K, True, True, splitk)[1], plan_small(M, N, K, True, False, splitk)[1])
    return sp * M * N * 4 if sp > 1 else 0


def gemm_plan(shape, knobs=None, cu_count=256):
    """shape: the SHAPE keys (missing ones take SHAPE's values, lda = the depth of A's rows), knobs: the KNOBS keys -> dict of FIELDS."""
    g = dict(SHAPE, **shape)
    kn = dict(KNOBS, **(knobs or {}))
    M, N, K, a_wrap = g["M"], g["N"], g["K"], g["a_wrap"]
    if "lda" not in shape:
        g["lda"] = a_wrap if a_wrap else K
    forced = kn["kernel"]
    # ---- the kernel (ofx_launch_gemm)
    kind = AUTO if forced == W2 else forced
    if a_wrap:
        t2 = ((M + 255) // 256) * (N // 256)
        ok = K == 2 * a_wrap and a_wrap % 32 == 0 and a_wrap >= 64 and N % 256 == 0 and (t2 >= 256 or forced == W2) and forced != K128
        kind = W2 if ok else K128
        if kind == W2 and g["has_w8"] and g["f16"] and a_wrap % 128 == 0:
            kind = W2F8
    elif kind == AUTO:
        t2, t3 = ((M + 255) // 256) * (N // 256), ((M + 255) // 256) * (N // 128)
        if N % 256 == 0 and t2 >= 1024:
            kind = PP if K <= 1024 else K256
        elif N % 128 == 0 and t3 >= 512:
            kind = K256x128
        else:
            kind = K128
    if (g["k_mult"] == 3 and not a_wrap and kn["x3_kernel"] and forced in (AUTO, W2) and K % 96 == 0 and N % 128 == 0 and g["lda"] >= K
            and (kn["x3_kernel"] >= 2 or ((M + 255) // 256) * (N // 128) >= 192)):
        kind = X3
    if kind in (K256, PP) and N % 256:
        kind = K128
    if kind == K64 and N % 128:
        kind = K128
    p = dict.fromkeys(FIELDS, 0)
    p["kind"] = kind
    # ---- the profile record
    km = K // a_wrap if a_wrap else (g["k_mult"] if g["k_mult"] > 0 else 1)
    ab = 2.0 * M * (K // 3) * 2 if kind == X3 else 2.0 * M * (a_wrap if a_wrap else K)
    wb = 3.0 * N * a_wrap if kind == W2F8 else (2.0 * N * (K // 3) * 2 if kind == X3 else 2.0 * N * K)
    ob = 4.0 if g["out_kind"] == 0 else (6.0 if g["out_kind"] == 2 else 2.0)
    if g["xlo"]:
        ob = 8.0
    elif g["resid"]:
        ob += 4.0
    if g["aux"]:
        ob += 4.0
    p["kmul"], p["k_logical"], p["bytes"] = km, K // km, ab + wb + ob * M * N
    p["flops"] = 2.0 * M * N * K * (0.75 if kind == W2F8 else 1.0)
    p["splits"], p["grid_y"] = 1, 1
    # ---- the big-tile launchers: launch_big<WR, WC> (256x256: 2, 4; 256x128: 2, 2), launch_pp, launch_w2, ofx_gemm_launch_w2f8, launch_x3
    if kind in (K256, K256x128, PP, W2, W2F8, X3):
        p["group_m"] = 4 if kind == K256x128 else 8
        p["tile_m"], p["tile_n"] = 256, (128 if kind in (K256x128, X3) else 256)
        p["tiles_n"], p["tiles_m"] = N // p["tile_n"], (M + 255) // 256
        p["nwg"] = p["tiles_m"] * p["tiles_n"]
        if kind in (W2, W2F8):
            p["grid_x"] = persistent_grid(p["nwg"], kn["w2_persist"], g["has_m_dev"], cu_count)
        elif kind == X3:
            p["grid_x"] = persistent_grid(p["nwg"], kn["w2_persist"] if kn["x3_persist"] == 1 else 0, g["has_m_dev"], cu_count)
        else:
            p["grid_x"] = p["nwg"]
        if kind == W2F8:
            p["epi_direct"] = kn["epi_direct"]
        return p
    # ---- the 128x128 / 64x128 kernel
    tiles_n, tiles_m = N // BN, (M + BM - 1) // BM
    gm = min(max((3 << 20) // (BM * K * 2) // 2, 1), 8)
    can64 = kind == K64 or (kind == K128 and forced == AUTO and M > 64 and tiles_m * tiles_n <= 384)
    tile64, splits = plan_small(M, N, K, bool(g["can_split"]), bool(can64), kn["splitk"])
    if kind == K64:
        tile64 = 1
    if tile64:
        tiles_m, gm = (M + 63) // 64, 2 * gm
    p.update(tile_m=64 if tile64 else 128, tile_n=128, tiles_m=tiles_m, tiles_n=tiles_n, nwg=tiles_m * tiles_n, group_m=gm, splits=splits,
             kt_per_split=(K // BK + splits - 1) // splits if splits > 1 else 0, grid_x=tiles_m * tiles_n, grid_y=splits if splits > 1 else 1)
    if splits > 1:
        if g["defer"]:
            p["second_pass"] = PASS_DEFERRED
        elif g["ln_fusable"] and N in (512, 768, 1024, 1536):
            p["second_pass"] = PASS_REDUCE_LN
        else:
            p["second_pass"] = PASS_REDUCE
            p["reduce_grid"] = min((M * (N // 4) + 255) // 256, 2048)
    return p


def tn_splits(M, N, K):
    tiles = ((M + 255) // 256) * (N // 256)
    nkt = (K + 63) // 64
    best, best_t = 1, 1e30
    for s in range(1, min(16, nkt) + 1):
        waves = float((tiles * s + 255) // 256)
        t = waves * ((nkt + s - 1) // s) * 1.6 + 4.0 + ((2.0 * s * M * N * 4.0 / 4.0e6 + 3.0) if s > 1 else 0.0)
        if t < best_t:
            best_t, best = t, s
    return best
