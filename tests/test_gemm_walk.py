"""The GEMM kernels' tile walk (outfitx_amd/csrc/gemm_walk.h: xcd_remap, grouped_tile), compiled alone by the Makefile's compiler
in host-only mode and checked on every point of a lattice of grids: tiles_m 1..40 x tiles_n 1..13 x group_m {1, 2, 3, 4, 8, 16} x
splits {1, 2, 3, 5} (nwg = tiles x splits; splits > 1 is gemm_tn_kernel's use, which peels the split index off the remapped id).
CPU only: the header is plain integer arithmetic."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GROUP_M = (1, 2, 3, 4, 8, 16)
SPLITS = (1, 2, 3, 5)
TILES_M = range(1, 41)
TILES_N = range(1, 14)

# One record of four int16 per block id, in the order of the loops of `lattice()` below: the remapped id, then - as gemm_tn_kernel
# peels them - the split index and the tile of the remaining id.
PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "gemm_walk.h"
int main() {
    const int G[] = {%(G)s}, S[] = {%(S)s};
    std::vector<short> out;
    for (int g : G) for (int sp : S) for (int tiles_m = 1; tiles_m <= %(TM)d; ++tiles_m) for (int tiles_n = 1; tiles_n <= %(TN)d; ++tiles_n) {
        const int tiles = tiles_m * tiles_n, nwg = tiles * sp;
        for (int b = 0; b < nwg; ++b) {
            const int bid = xcd_remap(b, nwg), split = bid / tiles;
            int tm, tn;
            grouped_tile(bid - split * tiles, g, tiles_m, tiles_n, tm, tn);
            out.push_back((short)bid); out.push_back((short)split); out.push_back((short)tm); out.push_back((short)tn);
        }
    }
    return fwrite(out.data(), sizeof(short), out.size(), stdout) == out.size() ? 0 : 1;
}
"""


def lattice():
    """Flat int64 arrays over every (grid, block id) of the domain, in the program's order, plus each grid's first record."""
    cols = {k: [] for k in ("b", "nwg", "g", "tiles_m", "tiles_n")}
    starts, n = [], 0
    for g in GROUP_M:
        for sp in SPLITS:
            for tiles_m in TILES_M:
                for tiles_n in TILES_N:
                    nwg = tiles_m * tiles_n * sp
                    cols["b"].append(np.arange(nwg))
                    for k, v in (("nwg", nwg), ("g", g), ("tiles_m", tiles_m), ("tiles_n", tiles_n)):
                        cols[k].append(np.full(nwg, v))
                    starts.append(np.full(nwg, n))
                    n += nwg
    return {k: np.concatenate(v).astype(np.int64) for k, v in cols.items()}, np.concatenate(starts).astype(np.int64)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_walk")
    src = d / "walk.cpp"
    src.write_text(PROGRAM % {"G": ", ".join(map(str, GROUP_M)), "S": ", ".join(map(str, SPLITS)), "TM": TILES_M[-1], "TN": TILES_N[-1]})
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = os.path.join(ROOT, "outfitx_amd", "csrc")
    subprocess.run([hipcc, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(d / "walk")], check=True)
    raw = subprocess.run([str(d / "walk")], check=True, capture_output=True).stdout
    c, starts = lattice()
    rec = np.frombuffer(raw, dtype=np.int16).reshape(-1, 4).astype(np.int64)
    assert rec.shape[0] == c["b"].size == 820 * 91 * sum(SPLITS) * len(GROUP_M)
    return c, starts, rec


def test_xcd_remap_is_a_permutation(walk):
    c, starts, rec = walk
    bid = rec[:, 0]
    assert ((bid >= 0) & (bid < c["nwg"])).all()
    assert (np.bincount(starts + bid, minlength=bid.size) == 1).all()      # every id of every grid exactly once


def test_every_tile_once_per_split(walk):
    c, starts, rec = walk
    split, tm, tn = rec[:, 1], rec[:, 2], rec[:, 3]
    tiles = c["tiles_m"] * c["tiles_n"]
    assert ((split >= 0) & (split * tiles < c["nwg"])).all()
    assert ((tm >= 0) & (tm < c["tiles_m"]) & (tn >= 0) & (tn < c["tiles_n"])).all()
    assert (np.bincount(starts + split * tiles + tm * c["tiles_n"] + tn, minlength=tm.size) == 1).all()


def test_walk_equals_the_kernels_formulas(walk):
    """The formulas as every kernel wrote them out before they moved into the header (C division of non-negative ints = floor)."""
    c, _, rec = walk
    bid, nwg = c["b"], c["nwg"]
    nx = 8
    q, r, x, i = nwg // nx, nwg % nx, bid % nx, bid // nx
    bid = np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + i
    assert (rec[:, 0] == bid).all()
    tiles = c["tiles_m"] * c["tiles_n"]
    split = bid // tiles
    t = bid - split * tiles
    per_group = c["g"] * c["tiles_n"]
    gidx = t // per_group
    first = gidx * c["g"]
    gm = np.minimum(c["g"], c["tiles_m"] - first)
    r = t - gidx * per_group
    assert (rec[:, 1] == split).all()
    assert (rec[:, 2] == first + r % gm).all()
    assert (rec[:, 3] == r // gm).all()
