"""The GEMM launch decision (outfitx_amd/csrc/gemm_plan.h: gemm_plan, gemm_splitk_slab_bytes, gemm_tn_splits), compiled alone by the
Makefile's compiler in host-only mode.  A small program reads (shape, knobs, CU count) records and prints every field of the plan; the
lattice below puts points on both sides of every comparison of the rule, and on each of them the plan EQUALS the transcription of the
launch code as it stood before the header (tests/gemm_plan_ref.py) - integers and the float64 FLOP / byte counts alike.  Further
properties hold whatever the transcription says.  CPU only: the header is plain integer and double arithmetic."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import gemm_plan_ref as R
from conftest import ROOT

SHAPE_KEYS = tuple(R.SHAPE)
KNOB_KEYS = tuple(R.KNOBS)
NIN = len(SHAPE_KEYS) + len(KNOB_KEYS) + 1          # + the CU count

# in: int32 records [shape..., knobs..., cu]; out: float64 rows [FIELDS..., slab bytes of the shape under the knobs] (every integer
# here is exact in a double).  `tn`: int32 (M, N, K) -> float64 (splits, slab bytes).
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "gemm_plan.h"
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<int> in;
    int buf[4096];
    for (size_t n; (n = fread(buf, sizeof(int), 4096, f)) > 0;) in.insert(in.end(), buf, buf + n);
    fclose(f);
    std::vector<double> out;
    if (!strcmp(argv[1], "tn")) {
        for (size_t i = 0; i + 3 <= in.size(); i += 3) {
            out.push_back(gemm_tn_splits(in[i], in[i + 1], in[i + 2]));
            out.push_back((double)gemm_tn_slab_bytes(in[i], in[i + 1], in[i + 2]));
        }
    } else {
        for (size_t i = 0; i + %(NIN)d <= in.size(); i += %(NIN)d) {
            const int* r = &in[i];
            GemmShape s;
            s.M = r[0]; s.N = r[1]; s.K = r[2]; s.lda = r[3]; s.a_wrap = r[4]; s.k_mult = r[5]; s.f16 = r[6]; s.has_w8 = r[7]; s.has_m_dev = r[8];
            s.can_split = r[9]; s.defer = r[10]; s.ln_fusable = r[11]; s.out_kind = r[12]; s.resid = r[13]; s.aux = r[14]; s.xlo = r[15];
            GemmKnobs k;
            k.kernel = r[16]; k.splitk = r[17]; k.x3_kernel = r[18]; k.x3_persist = r[19]; k.w2_persist = r[20]; k.epi_direct = r[21];
            const GemmPlan p = gemm_plan(s, k, r[22]);
            const double row[] = {(double)p.kind, (double)p.tile_m, (double)p.tile_n, (double)p.tiles_m, (double)p.tiles_n, (double)p.nwg, (double)p.group_m,
                                  (double)p.splits, (double)p.kt_per_split, (double)p.grid_x, (double)p.grid_y, (double)p.second_pass, (double)p.reduce_grid,
                                  (double)p.epi_direct, (double)p.kmul, (double)p.k_logical, p.flops, p.bytes,
                                  (double)gemm_splitk_slab_bytes(s.M, s.N, s.K, k)};
            out.insert(out.end(), row, row + sizeof(row) / sizeof(double));
        }
    }
    return fwrite(out.data(), sizeof(double), out.size(), stdout) == out.size() ? 0 : 1;
}
"""
assert SHAPE_KEYS == ("M", "N", "K", "lda", "a_wrap", "k_mult", "f16", "has_w8", "has_m_dev", "can_split", "defer", "ln_fusable", "out_kind", "resid", "aux", "xlo")
assert KNOB_KEYS == ("kernel", "splitk", "x3_kernel", "x3_persist", "w2_persist", "epi_direct")

CUS = (256, 80)
# the widths the models use (512 .. 6144) and widths that are no multiple of 256
WIDTHS = (128, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4608, 6144)
# depths: nk = 1, 2, 15 | 16 (the split threshold), K <= 1024 | above, sp <= nk / 4 at many nk
DEPTHS = (64, 128, 512, 960, 1024, 1088, 1536, 3072, 4096, 4608, 6144)
# rows: 1, around the 64- and 128-row tiles, the planner's blocks < 256 (N = 1024: 3968 | 4096) and tiles <= 384 (N = 1536: 4096 | 4097),
# t3 >= 512 (N = 1536: 10752 | 10753), t2 >= 1024 (N = 4608: 14336 | 14337; N = 1024: 65280 | 65536)
ROWS = (1, 63, 64, 65, 128, 129, 256, 257, 288, 300, 512, 1000, 2304, 3840, 3968, 3969, 4096, 4097, 4224, 10752, 10753, 14336, 14337, 65280, 65281, 65536, 65537)
# knob 5: never, planned, forced (2, 4, 16, 40 -> 16, 255 -> 16 slices; + bit 8: 64-row tiles, 1 slice and 4 and 40 -> 16)
SPLITK = (0, 1, 2, 4, 16, 17, 40, 255, 0x101, 0x104, 0x128)


def points():
    """Every lattice point as a dict of the keys that differ from the defaults."""
    out = []
    # the automatic choice and every forced kernel over the whole shape lattice, with and without a slab
    for kernel, M, N, K, can_split in itertools.product(range(7), ROWS, WIDTHS, DEPTHS, (0, 1)):
        if kernel in (0, 5) or (M, K) in {(r, k) for r in ROWS[::3] for k in DEPTHS[::2]}:
            out.append(dict(M=M, N=N, K=K, can_split=can_split, kernel=kernel))
    # knob 5 on the small plans
    for splitk, kernel, M, N, K, can_split in itertools.product(SPLITK, (0, 1, 5), (1, 64, 65, 300, 2304, 4224), (512, 1024, 1536, 4608), (64, 512, 1024, 4096), (0, 1)):
        out.append(dict(M=M, N=N, K=K, can_split=can_split, kernel=kernel, splitk=splitk))
    # split weights: a_wrap % 32 (48, 80), >= 64 (32), % 128 (64, 192), K == 2 a_wrap or not, t2 >= 256 (N = 512: 32512 | 32768 is 254 | 256 tiles,
    # N = 1536: 10752 | 10753, N = 4608: 3584 | 3585)
    for (a_wrap, K), M, N, has_w8, f16, kernel, w2_persist, has_m_dev, cu in itertools.product(
            ((32, 64), (48, 96), (64, 128), (80, 160), (128, 256), (128, 512), (192, 384), (768, 1536), (1536, 3072)), (1, 300, 3584, 3585, 10752, 10753, 32512, 32768),
            (384, 512, 1536, 4608), (0, 1), (0, 1), (0, 1, 2, 6), (-1, 0, 5, 300), (0, 1), CUS):
        out.append(dict(M=M, N=N, K=K, a_wrap=a_wrap, has_w8=has_w8, f16=f16, kernel=kernel, w2_persist=w2_persist, has_m_dev=has_m_dev, cu=cu, can_split=1))
    # three products: K % 96 (192, 576, 960, 4608 | 256, 320), lda >= K or not, 192 tiles (N = 1536: 3840 | 4096), knobs 15, 16, 11
    for K, short_lda, M, N, x3_kernel, x3_persist, w2_persist, kernel, has_m_dev, cu in itertools.product(
            (192, 256, 320, 576, 960, 4608), (0, 1), (1, 256, 3840, 4096, 4097, 70000), (128, 1536, 4608), (0, 1, 2), (0, 1), (-1, 0, 7), (0, 1, 3, 6), (0, 1), CUS):
        out.append(dict(M=M, N=N, K=K, lda=K - 8 * short_lda, k_mult=3, x3_kernel=x3_kernel, x3_persist=x3_persist, w2_persist=w2_persist, kernel=kernel,
                        has_m_dev=has_m_dev, cu=cu, f16=has_m_dev))
    # the second pass and the record's byte count: a shape that splits at every width, one that does not, the fp8 kernel, the three-product kernel
    for base in ([dict(M=64, N=N, K=4096, can_split=1) for N in (512, 768, 1024, 1536, 2048, 4608)] + [dict(M=64, N=1536, K=4096, can_split=0), dict(M=3000, N=1536, K=1536, can_split=1),
                 dict(M=300, N=512, K=256, a_wrap=128, has_w8=1, f16=1, kernel=6), dict(M=300, N=512, K=576, k_mult=3, x3_kernel=2), dict(M=300, N=512, K=576, k_mult=2)]):
        for defer, ln_fusable, out_kind, resid, aux, xlo, epi_direct in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1)):
            out.append(dict(base, defer=defer, ln_fusable=ln_fusable, out_kind=out_kind, resid=resid, aux=aux, xlo=xlo, epi_direct=epi_direct))
    return out


def record(pt):
    shape = dict(R.SHAPE, **{k: v for k, v in pt.items() if k in R.SHAPE})
    if "lda" not in pt:
        shape["lda"] = shape["a_wrap"] or shape["K"]
    knobs = dict(R.KNOBS, **{k: v for k, v in pt.items() if k in R.KNOBS})
    return shape, knobs, pt.get("cu", 256)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_plan")
    src = d / "plan.cpp"
    src.write_text(PROGRAM % {"NIN": NIN})
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = os.path.join(ROOT, "outfitx_amd", "csrc")
    subprocess.run([hipcc, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(d / "plan")], check=True)

    def run(mode, records, width):
        path = d / f"{mode}.in"
        np.ascontiguousarray(records, dtype=np.int32).tofile(path)
        raw = subprocess.run([str(d / "plan"), mode, str(path)], check=True, capture_output=True).stdout
        return np.frombuffer(raw, dtype=np.float64).reshape(len(records), width)
    return run


@pytest.fixture(scope="module")
def lattice(program):
    recs = [record(pt) for pt in points()]
    rows = np.array([[s[k] for k in SHAPE_KEYS] + [kn[k] for k in KNOB_KEYS] + [cu] for s, kn, cu in recs], dtype=np.int64)
    got = program("plan", rows, len(R.FIELDS) + 1)
    want = [R.gemm_plan(s, kn, cu) for s, kn, cu in recs]
    return recs, {f: got[:, i] for i, f in enumerate(R.FIELDS + ("slab",))}, {f: np.array([w[f] for w in want], dtype=np.float64) for f in R.FIELDS}


def test_plan_equals_the_launch_code_it_replaces(lattice):
    recs, got, want = lattice
    for f in R.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (f, len(bad), recs[bad[0]], got[f][bad[0]], want[f][bad[0]])
    slab = np.array([R.splitk_bytes(s["M"], s["N"], s["K"], kn["splitk"]) for s, kn, _ in recs], dtype=np.float64)
    assert (got["slab"] == slab).all()


def test_lattice_meets_both_sides_of_every_comparison(lattice):
    """The lattice is worth what it reaches: every kernel kind, both tile heights with and without a split, all four second-pass routes,
    persistent and one-block-per-tile grids, and each threshold of the rule from both sides (by the rule's own inputs, not its result)."""
    recs, got, _ = lattice
    S = {k: np.array([s[k] for s, _, _ in recs]) for k in SHAPE_KEYS}
    KN = {k: np.array([kn[k] for _, kn, _ in recs]) for k in KNOB_KEYS}
    cu = np.array([c for _, _, c in recs])
    M, N, K, aw = S["M"], S["N"], S["K"], S["a_wrap"]
    t2, t3 = (M + 255) // 256 * (N // 256), (M + 255) // 256 * (N // 128)
    auto = (KN["kernel"] == 0) & (aw == 0) & (S["k_mult"] == 1)
    sides = {
        "t2 >= 1024": (t2 >= 1024)[auto & (N % 256 == 0)],
        "K <= 1024": (K <= 1024)[auto & (N % 256 == 0) & (t2 >= 1024)],
        "t3 >= 512": (t3 >= 512)[auto & ~((N % 256 == 0) & (t2 >= 1024))],
        "w2: t2 >= 256": (t2 >= 256)[(aw >= 64) & (K == 2 * aw) & (N % 256 == 0) & (KN["kernel"] == 0)],
        "w2: a_wrap % 32": (aw % 32 == 0)[aw > 0], "w2: a_wrap >= 64": (aw >= 64)[aw > 0], "w2: K == 2 a_wrap": (K == 2 * aw)[aw > 0],
        "w2: N % 256": (N % 256 == 0)[aw > 0], "w2: a_wrap % 128": (aw % 128 == 0)[np.isin(got["kind"], (6, 8))],
        "w2: W8": S["has_w8"][aw > 0] == 1, "w2: f16": S["f16"][(aw > 0) & (S["has_w8"] == 1)] == 1,
        "x3: K % 96": (K % 96 == 0)[S["k_mult"] == 3], "x3: lda >= K": (S["lda"] >= K)[S["k_mult"] == 3],
        "x3: 192 tiles": (t3 >= 192)[(S["k_mult"] == 3) & (KN["x3_kernel"] == 1) & (K % 96 == 0) & (S["lda"] >= K) & (KN["kernel"] == 0)],
        "small: M > 64": (M > 64)[got["kind"] == 1], "small: tiles <= 384": (((M + 127) // 128) * (N // 128) <= 384)[(got["kind"] == 1) & (KN["kernel"] == 0)],
        "small: blocks < 256": (((M + 127) // 128) * (N // 128) < 256)[(got["kind"] == 1) & (S["can_split"] == 1) & (KN["splitk"] == 1) & (K >= 1024)],
        "small: nk >= 16": (K // 64 >= 16)[(got["kind"] == 1) & (S["can_split"] == 1) & (KN["splitk"] == 1)],
        "has_m_dev": S["has_m_dev"][np.isin(got["kind"], (6, 8, 9))] == 1,
        "persistent grid": (got["grid_x"] < got["nwg"])[np.isin(got["kind"], (6, 8, 9))],
        "CU count": (cu == 256)[got["grid_x"] < got["nwg"]],
    }
    for name, v in sides.items():
        assert v.any() and not v.all(), name
    assert set(got["kind"]) == {1, 2, 3, 4, 5, 6, 8, 9}
    assert set(KN["kernel"]) == set(range(7)) and set(KN["splitk"]) == set(SPLITK)
    assert set(KN["x3_kernel"]) == {0, 1, 2} and set(KN["x3_persist"]) == {0, 1} and {-1, 0} < set(KN["w2_persist"])
    assert set(got["second_pass"]) == {0, 1, 2, 3}
    planned = KN["splitk"] == 1
    for t in (64, 128):              # both tile heights, planned, with and without a split; the planner's sp <= nk / 4 bound is reached
        assert set((got["splits"] > 1)[planned & (got["tile_m"] == t)]) == {False, True}
    assert (got["splits"] == (K // 64) // 4)[planned & (got["splits"] > 1)].any() and got["splits"].max() == 16
    assert {512, 768, 1024, 1536} <= set(N[got["second_pass"] == 2]) and {2048, 4608} <= set(N[(got["second_pass"] == 3) & (S["ln_fusable"] == 1)])
    assert {1536, 4608, 6144} <= set(N)


def test_plan_properties(lattice):
    recs, got, _ = lattice
    M = np.array([s["M"] for s, _, _ in recs])
    N = np.array([s["N"] for s, _, _ in recs])
    nk = np.array([s["K"] for s, _, _ in recs]) // 64
    sp, kps = got["splits"], got["kt_per_split"]
    split = sp > 1
    assert ((sp >= 1) & (sp <= 16) & (got["grid_y"] == sp)).all()
    assert (((sp - 1) * kps < nk) & (nk <= sp * kps))[split].all()                  # every k-tile belongs to exactly one split, no split is empty
    assert (kps[~split] == 0).all() and ((got["second_pass"] > 0) == split).all()
    assert ((got["grid_x"] >= 1) & (got["grid_x"] <= got["nwg"])).all()
    assert (got["nwg"] == got["tiles_m"] * got["tiles_n"]).all()
    assert (got["tiles_m"] * got["tile_m"] >= M).all() and ((got["tiles_m"] - 1) * got["tile_m"] < M).all()
    assert (got["tiles_n"] * got["tile_n"] == N).all()
    assert (got["group_m"] >= 1).all()


def test_slab_covers_the_plan_under_either_tile_height(program):
    """ofx_gemm_splitk_bytes sizes the slab before the launcher knows whether it may use 64-row tiles: whatever the forced kernel (0:
    the grid decides, 1: never, 5: always) the plan's slices fit, under every value of knob 5."""
    pts = [dict(M=M, N=N, K=K, can_split=1, kernel=kernel, splitk=splitk) for splitk, kernel, M, N, K in
           itertools.product(SPLITK, (0, 1, 5), ROWS[:20], (512, 1024, 1536, 4608), (512, 1024, 1536, 4096, 6144))]
    recs = [record(pt) for pt in pts]
    rows = np.array([[s[k] for k in SHAPE_KEYS] + [kn[k] for k in KNOB_KEYS] + [cu] for s, kn, cu in recs], dtype=np.int64)
    got = program("plan", rows, len(R.FIELDS) + 1)
    splits, tile_m, slab = got[:, R.FIELDS.index("splits")], got[:, R.FIELDS.index("tile_m")], got[:, -1]
    need = np.where(splits > 1, splits * rows[:, 0] * rows[:, 1] * 4, 0)
    assert (slab >= need).all()
    assert (splits > 1)[tile_m == 64].any() and (splits > 1)[tile_m == 128].any()


def test_tn_splits(program):
    """gemm_tn_splits over the weight-gradient shapes (M, N multiples of 256; K = the row count, any value): equal to the planner that
    stood in gemm_tn.hip, at most 16 slices, none of them empty, and the slab is the slices' size."""
    rows = np.array(list(itertools.product((256, 512, 1024, 1536, 3072, 4608, 6144), (256, 512, 1536, 4608, 6144),
                                           (1, 63, 64, 65, 128, 200, 512, 1000, 1024, 2304, 4096, 9000, 16384, 65536))), dtype=np.int64)
    got = program("tn", rows, 2)
    s = got[:, 0]
    assert (s == np.array([R.tn_splits(*r) for r in rows.tolist()])).all()
    assert ((s >= 1) & (s <= 16) & (s <= (rows[:, 2] + 63) // 64)).all()
    assert (got[:, 1] == np.where(s > 1, s * rows[:, 0] * rows[:, 1] * 4, 0)).all()
    assert s.min() == 1 and s.max() == 16
