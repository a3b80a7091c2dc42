"""The stage arithmetic of the persistent ping-pong GEMM kernels (outfitx_amd/csrc/gemm_pingpong.h: pp_stage, pp_epilogue_stage,
pp_next_base - what PpWalk::stage / epilogue_stage / advance compute), compiled alone by the Makefile's compiler in host-only mode,
and a replay of one block's walk on it: NST in {3, 4} stages, nk = 1..13 k-steps per tile (four stages: the multiples of 4, the
fp8 kernel's super-steps), 1..5 tiles per block, with the fill schedules of the kernels.

Time is counted in barrier slots.  A tile takes slots 0 .. 2 nk + 1 (slot 0: the wait for step 0; group 0 reads step t in slot
2 t + 1, group 1 in slot 2 t + 2; slot 2 nk + 1 is group 1's last MFMA slot), the epilogue follows and the next tile starts at its
own slot 0.  Each group fills ITS half of a stage (its waves' LDS-DMA pieces) and both groups read both halves.  Iteration t of
group g issues its fills at the top of its read slot, 2 t + 1 + g.
  three stages (gemm_w2, gemm_x3, the fused kernel's dual-weight branch): the block's first tile fills steps 0, 1 in slot 0;
    iteration t fills step t + 2;
  four stages (gemm_w2f8, head comment of gemm_w2f8.hip): the first tile fills steps 0, 1 (group 0) / 0, 1, 2 (group 1) in slot 0;
    iteration t = 4 u + r fills   group 0: r = 0: t + 2, t + 3;  1: nothing (the fp8 quarters);  2: t + 2;  3: t + 2
                                  group 1: r = 0: t + 3;          1: nothing;                     2: t + 2;  3: t + 2, t + 3.
A step x >= nk of the walk is step x - nk of the block's next tile (on the block's last tile, and where x - nk is no step of the
next tile, the fill is redundant: it overwrites the stage with data nobody reads).

Three stages with ONE k-step per tile lie outside the schedule: iteration t fills step t + 2, which is then two tiles ahead, so
from the third tile of a block on step 0 was never fetched.  The replay must say so (it does: that case is asserted to fail check
(a)); the dispatcher gives these kernels problems of two k-steps and more (logical depth a multiple of 64; 128 with four stages).
CPU only: plain integers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NK_MAX, X_MAX = 13, 20

# int8 tables: stage[NST][base][x], epilogue[NST][base][nk], next_base[NST][base][nk] for NST = 3, 4 (base < 4, rows base >= NST unused)
PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "gemm_pingpong.h"
template <int NST>
void tabulate(std::vector<signed char>& out) {
    for (int base = 0; base < 4; ++base) for (int x = 0; x < %(X)d; ++x) out.push_back((signed char)(base < NST ? pp_stage<NST>(base, x) : -1));
    for (int base = 0; base < 4; ++base) for (int nk = 0; nk <= %(NK)d; ++nk) out.push_back((signed char)(base < NST && nk ? pp_epilogue_stage<NST>(base, nk) : -1));
    for (int base = 0; base < 4; ++base) for (int nk = 0; nk <= %(NK)d; ++nk) out.push_back((signed char)(base < NST && nk ? pp_next_base<NST>(base, nk) : -1));
}
int main() {
    std::vector<signed char> out;
    tabulate<3>(out);
    tabulate<4>(out);
    return fwrite(out.data(), 1, out.size(), stdout) == out.size() ? 0 : 1;
}
"""


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_pingpong")
    src = d / "pp.cpp"
    src.write_text(PROGRAM % {"X": X_MAX, "NK": NK_MAX})
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    inc = os.path.join(ROOT, "outfitx_amd", "csrc")
    subprocess.run([hipcc, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(d / "pp")], check=True)
    raw = np.frombuffer(subprocess.run([str(d / "pp")], check=True, capture_output=True).stdout, dtype=np.int8).astype(np.int64)
    per = 4 * X_MAX + 2 * 4 * (NK_MAX + 1)
    assert raw.size == 2 * per
    t = {}
    for k, nst in enumerate((3, 4)):
        r = raw[k * per:(k + 1) * per]
        t[nst] = (r[:4 * X_MAX].reshape(4, X_MAX), r[4 * X_MAX:4 * X_MAX + 4 * (NK_MAX + 1)].reshape(4, NK_MAX + 1), r[4 * X_MAX + 4 * (NK_MAX + 1):].reshape(4, NK_MAX + 1))
    return t


def fills(nst, g, t):
    """Steps that iteration t of group g issues."""
    if nst == 3:
        return [t + 2]
    return {0: ([t + 2, t + 3], [t + 3]), 1: ([], []), 2: ([t + 2], [t + 2]), 3: ([t + 2], [t + 2, t + 3])}[t % 4][g]


def first_fills(nst, g):
    return [0, 1] if nst == 3 or g == 0 else [0, 1, 2]


class Violation(AssertionError):
    pass


def replay(tab, nst, nk, tiles):
    """One block's walk over `tiles` tiles; raises Violation(check, ...) at the first broken property."""
    stage, epilogue, next_base = tab[nst]
    read_slot = lambda j, t, g: j * (2 * nk + 2) + 2 * t + 1 + g             # global slot in which group g reads step t of tile j
    held = [[None] * nst, [None] * nst]                                      # per group half and stage: (tile, step, slot of the fill) or None
    base = 0
    for j in range(tiles):
        t0 = j * (2 * nk + 2)
        epi = epilogue[base, nk]
        assert epi == stage[base, nk - 1]

        def fill(g, x, now):
            s = stage[base, x]
            assert 0 <= s < nst
            old = held[g][s]
            if old is not None and old[0] is not None:                       # (b) the step this half holds has been read by BOTH groups
                if not all(read_slot(old[0], old[1], r) < now for r in (0, 1)):
                    raise Violation("b", nst, nk, tiles, j, g, x, old)
            if x >= nk and s == epi:                                         # (c) lands under this tile's epilogue
                raise Violation("c", nst, nk, tiles, j, g, x)
            tile, step = (j, x) if x < nk else (j + 1, x - nk)
            live = tile < tiles and step < nk
            held[g][s] = (tile if live else None, step, now)

        if j == 0:
            for g in (0, 1):
                for x in first_fills(nst, g):
                    fill(g, x, t0)
        for slot in range(1, 2 * nk + 2):
            for g in (0, 1):
                t, odd = divmod(slot - 1 - g, 2)
                if odd or not 0 <= t < nk:
                    continue
                for x in fills(nst, g, t):                                   # ISSUE, then READ (gemm_pingpong.h: pp_slot)
                    fill(g, x, t0 + slot)
                for half in (0, 1):                                          # (a) step t sits, complete, in the stage it is read from
                    h = held[half][stage[base, t]]
                    if h is None or h[:2] != (j, t) or not h[2] < t0 + slot:
                        raise Violation("a", nst, nk, tiles, j, g, t, h)
        nb = next_base[base, nk]
        for x in range(nk, nk + nst - 1):                                    # (d) the prefetched steps are where the next tile looks for them
            if stage[base, x] != stage[nb, x - nk]:
                raise Violation("d", nst, nk, tiles, j, x)
        base = nb


CASES = [(3, nk) for nk in range(1, NK_MAX + 1)] + [(4, nk) for nk in range(4, NK_MAX + 1, 4)]


@pytest.mark.parametrize("nst,nk", CASES)
def test_walk_reads_every_step_where_it_was_filled_and_fills_no_stage_in_use(tables, nst, nk):
    for tiles in range(1, 6):
        if nst == 3 and nk == 1 and tiles >= 3:                              # outside the schedule (module docstring): the replay notices
            with pytest.raises(Violation) as e:
                replay(tables, nst, nk, tiles)
            assert e.value.args[0] == "a" and e.value.args[4] == 2           # step 0 of the block's third tile was never fetched
        else:
            replay(tables, nst, nk, tiles)


def test_stage_arithmetic_is_the_kernels_formulas(tables):
    """(base + x) % NST, the stage of the tile's last step, (base + nk) % NST - as the kernels wrote them out before the header."""
    for nst in (3, 4):
        stage, epilogue, next_base = tables[nst]
        b = np.arange(nst)[:, None]
        assert (stage[:nst] == (b + np.arange(X_MAX)) % nst).all()
        nk = np.arange(1, NK_MAX + 1)
        assert (epilogue[:nst, 1:] == (b + nk - 1) % nst).all() and (next_base[:nst, 1:] == (b + nk) % nst).all()


def test_replay_notices_a_fill_into_a_stage_still_to_be_read(tables):
    """The replay has teeth: two stages under the three-stage schedule overwrite step t + 1 while group 1 has yet to read it."""
    stage, epilogue, next_base = tables[3]
    two = {3: (stage % 2, epilogue % 2, next_base % 2)}
    with pytest.raises(Violation):
        replay(two, 3, 6, 1)
