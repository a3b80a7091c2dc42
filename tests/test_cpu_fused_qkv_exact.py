"""What tests/fused_qkv_cases.py claims of every case, checked without a GPU: the exactness condition (so that bit equality is the right
criterion on the device), that q | k | v survive float32, the softmax band of the `ints` family and the winning margin of the `route`
family, the launcher's admission rule and the kernel's block -> (group, head) map restated in Python (every live (group, head) reached
exactly once; a case that claims the second unit row or the odd-head block order reaches it), and the eleven mutants of the model.

MUTANTS, measured with the model on these inputs.  Every mutant changes the expected bits in every case where it applies, and mutants
2, 4, 5, 6, 7, 9 and 10 break the per-block rule of tests/test_gpu_fused_qkv_exact.py section B in every `ints` case where they apply.
THE OLD METRIC - max|a - b| / max|b| over the whole tensor at 8e-3 (bf16) / 1e-3 (f16), tests/test_gpu_ops.py - lets MUTANT 8 (bias
added before the rstd multiply) through on all sixteen bf16 `route` cases and on six of the eight dual-weight f16 `route` cases (a
wrong bias of at most 64 q on rows with rstd != 1, against v values of up to 128 x 7 q_w: 4.4e-3 - 4.8e-3 in bf16, 6.8e-4 - 8.4e-4 in
f16), and mutant 7 (the q block's col_sum used for v) through on the eight dual-weight bf16 `route` cases, while both change bits
and break the per-block rule there.  On the `ints` cases, whose operands all have one magnitude, no mutant passes the old metric:
test_the_old_metric_lets_mutant_8_through holds both statements."""
import numpy as np
import pytest
import torch

import fused_qkv_cases as F

TD = {"bf16": torch.bfloat16, "f16": torch.float16}
B_BREAKERS = (2, 4, 5, 6, 7, 9, 10)


def _roundtrip(a, td):
    return torch.from_numpy(np.array(a)).to(td).double().numpy()


def _max_prob_median(m):
    s = m.q @ np.swapaxes(m.k, -1, -2) * F.SCALE
    e = np.exp(s - s.max(-1, keepdims=True))
    return float(np.median((e / e.sum(-1, keepdims=True)).max(-1))), s


@pytest.mark.parametrize("group", list(F.GROUPS))
def test_every_case_holds_what_it_claims(group):
    for c in F.GROUPS[group]:
        d = F.build(c)
        W, M, S = d["W"], d["M"], c.S
        # ---- the exactness condition, and the operands are what the operand type holds
        assert d["bound"] < 2.0 ** 24 * d["q"] / 2, (c.name, d["bound"] / d["q"])
        for a in [d["x"], d["Wmat"]] + list(d["blocks"]):
            assert np.array_equal(_roundtrip(a, TD[c.dt]), a), c.name
        for a, lim, quantum in ((d["bias"], 64, d["q"]), (d["col_sum"], 64, d["qw"]), (d["mean"], 3, d["qa"])):
            u = a / quantum
            assert np.array_equal(u, np.round(u)) and np.abs(u).max() <= lim, c.name
        assert set(np.unique(d["rstd"])) <= ({0.5, 1.0, 2.0} if c.fold else {1.0}), c.name
        if c.family == "ints":
            for a, quantum in [(d["x"], d["qa"])] + [(b, d["qw"]) for b in d["blocks"]]:
                u = a / quantum
                assert np.array_equal(u, np.round(u)) and np.abs(u).max() == 7, c.name
        assert len(d["blocks"]) == (2 if c.kernel == "dual" else 1) and d["Wmat"].shape == (3 * W, len(d["blocks"]) * W)
        # ---- q | k | v: on the grid q / 2, exact in float32, one rounding away from the operand type
        v64 = F.qkv64(c)
        assert np.array_equal(v64 / (d["q"] / 2), np.round(v64 / (d["q"] / 2))), c.name
        assert np.array_equal(v64.astype(np.float32).astype(np.float64), v64), c.name
        m = F.model(c)
        assert np.array_equal(m.qkv.astype(np.float32).astype(np.float64), m.qkv) and np.array_equal(_roundtrip(m.qkv, TD[c.dt]), m.qkv), c.name
        assert np.isfinite(m.out).all() and m.out.shape == (M, W)
        # ---- the softmax is generic (ints) / decided with a margin no rounding can touch (route)
        med, s = _max_prob_median(m)
        if c.family == "ints":
            assert 1.5 / S <= med <= 0.6, (c.name, med)
        else:
            srt = np.sort(s, -1)
            margin = float(((srt[..., -1] - srt[..., -2]) * np.log2(np.e)).min())
            assert margin >= 160 and not srt[..., :-1].any(), (c.name, margin)
            win = d["rho"][:, d["pi"]].transpose(1, 0, 2)
            assert np.array_equal(s.argmax(-1), win), c.name
            assert np.array_equal(F.from_heads(np.ascontiguousarray(m.emul), c), m.out), (c.name, "the emulation must route v unchanged")
            assert np.array_equal(_roundtrip(m.out, TD[c.dt]), m.out)
            if W > 128:
                assert d["x"][:, 128:].any()
            assert not d["bias"][:2 * W].any() and not d["col_sum"][:2 * W].any() and all(not b[:2 * W].any() for b in d["blocks"][1:])
        # ---- guards
        assert d["X"].shape == (M + (F.EXTRA_ROWS if c.pad else 0), W + c.pad) and np.isnan(d["X"][:, W:]).all() and np.isnan(d["X"][M:]).all()
        assert np.isnan(d["stat"][M:]).all() and np.isfinite(d["stat"][:M]).all() and d["stat"].shape[0] == d["X"].shape[0]
        # ---- the launcher: admitted, G, groups, grid
        G, groups, nwg = F.geometry(S, c.heads, c.n_img)
        assert F.admission(S, W, c.heads, d["ldx"], d["ldo"], c.n_img, row_stat=bool(c.fold), col_sum=bool(c.fold)) == F.OFX_OK, c.name
        assert G == 256 // S and G * S <= 256 < (G + 1) * S and (G - 1) * S + 64 - 256 <= F.PAD_ROWS
        assert (groups - 1) * G < c.n_img <= groups * G and nwg % (6 * c.heads) == 0 and nwg >= groups * c.heads > nwg - 6 * c.heads
        if c.sweep in ("seq", "route") and c.n_img != 31:
            assert c.n_img == G + 1 and groups == 2                        # one full group and a one-image group
        # ---- the block order: every live (group, head) exactly once
        assert sorted(F.xcd_remap(b, nwg) for b in range(nwg)) == list(range(nwg))
        blocks = [F.block_of(b, c.heads, nwg) for b in range(nwg)]
        assert all(0 <= h < c.heads and g >= 0 for g, h, _ in blocks)
        live = [(g, h) for g, h, _ in blocks if g * G < c.n_img]
        assert sorted(live) == [(g, h) for g in range(groups) for h in range(c.heads)], c.name
        assert ("unit-row-2" in c.claims) == any(row >= 1 for g, _, row in blocks if g * G < c.n_img), c.name
        # odd heads: one unit holds all heads of its six groups; even: the second half of the heads sits one unit (6 x heads / 2 ids) later
        last_head_id = next(F.xcd_remap(b, nwg) for b in range(nwg) if blocks[b][:2] == (0, c.heads - 1))
        odd = c.heads % 2 == 1
        assert ("odd-heads" in c.claims) == odd and last_head_id == (c.heads - 1 if odd else 6 * (c.heads // 2) + c.heads // 2 - 1), c.name


def test_the_table_covers_what_it_is_for():
    for kernel in F.KERNELS:
        for dt in F.DTYPES:
            cs = [c for c in F.CASES if c.kernel == kernel and c.dt == dt]
            ints = [c for c in cs if c.family == "ints"]
            assert {c.S for c in cs if c.sweep == "seq"} == set(F.SEQ_S) and {256 // S for S in F.SEQ_S} == {4, 5, 6, 7}
            assert [(256 // S - 1) * S + 64 - 256 for S in F.SEQ_S] == [6, 12, -7, 13, -20, 8, 12, -36, -3, 0]
            assert {c.n_img for c in cs if c.sweep == "images" and c.S == 50} == set(F.IMAGES_N)
            assert any(c.S == 64 and c.n_img == 25 and "unit-row-2" in c.claims for c in ints)
            bk = 64 if kernel == "single" else 32
            steps = {c.heads * 64 // bk for c in cs if c.sweep == "heads"}
            assert steps == ({2, 3, 4, 5, 12} if kernel == "single" else {4, 6, 8, 10, 24})
            assert {s % 2 for s in steps} == {0, 1} or kernel == "dual"
            assert {s % 3 for s in steps} == {0, 1, 2}
            assert any(set(c.claims) == {"unit-row-2", "odd-heads"} for c in ints)
            assert {c.heads for c in cs if not c.fold} == {2, 3}
            assert any(c.pad == 8 and c.heads == 3 and c.S == 41 and c.n_img == 7 for c in ints)
            route = {(c.S, c.heads, c.n_img) for c in cs if c.family == "route"}
            assert route == {(S, h, 256 // S + 1) for S in (33, 50, 64) for h in (2, 3)} | {(50, 2, 31), (50, 3, 31)}
            for mu in F.MUTANTS:                                           # every mutant has a case of each family it can show in
                assert any(F.applies(c, mu) for c in ints) == (mu != 1 or kernel == "dual"), (kernel, dt, mu)
    for S in F.REFUSED_S:
        assert F.admission(S, 128, 2, 128, 128) == F.OFX_ESHAPE
    assert [S for S in range(33, 65) if F.admission(S, 128, 2, 128, 128) != F.OFX_OK] == [35, 36, 42]
    assert F.admission(50, 64, 1, 64, 64) == F.OFX_ESHAPE and F.admission(50, 128, 2, 132, 128) == F.OFX_ESHAPE
    assert F.admission(50, 128, 2, 128, 120) == F.OFX_ESHAPE and F.admission(50, 128, 2, 128, 128, row_stat=True) == F.OFX_EINVAL
    assert F.admission(50, 128, 2, 128, 128, X=False) == F.OFX_EINVAL


def test_block_map_is_a_bijection_over_heads_and_group_counts():
    """Wider than the table: heads 2 .. 16, 1 .. 39 groups."""
    for heads in range(2, 17):
        for groups in range(1, 40):
            nwg = ((groups + 5) // 6) * 6 * heads
            live = sorted((g, h) for g, h, _ in (F.block_of(b, heads, nwg) for b in range(nwg)) if g < groups)
            assert live == [(g, h) for g in range(groups) for h in range(heads)], (heads, groups)


def test_reassociated_float32_epilogues_equal_the_float64_value():
    """The condition at work: float32 sums of one case's products in random chunk orders, through two algebraic forms of the epilogue, are
    bit-equal to the float64 value."""
    c = next(c for c in F.CASES if c.sweep == "strides" and c.kernel == "dual")
    d = F.build(c)
    g = np.random.default_rng(0)
    rows, cols = slice(200, 264), slice(3 * 64, 4 * 64)                    # 64 rows, the k columns of head 0
    f32 = lambda a: np.asarray(a, np.float32)
    terms = np.concatenate([f32(d["x"])[rows, None, :] * f32(b)[None, cols, :] for b in d["blocks"]], 2)
    mean, rstd, cs, bias = f32(d["mean"])[rows, None], f32(d["rstd"])[rows, None], f32(d["col_sum"])[None, cols], f32(d["bias"])[None, cols]
    want = F.qkv64(c)[rows, cols]
    for _ in range(4):
        acc = np.zeros((64, 64), np.float32)
        for chunk in np.array_split(g.permutation(terms.shape[2]), 7):
            part = np.zeros((64, 64), np.float32)
            for k in chunk:
                part += terms[:, :, k]
            acc += part
        for v in ((acc - cs * mean) * rstd + bias, acc * rstd + (bias - cs * (mean * rstd)), bias - (cs * mean - acc) * rstd):
            assert v.dtype == np.float32 and np.array_equal(v.astype(np.float64), want)


@pytest.mark.parametrize("group", list(F.GROUPS))
def test_every_mutant_changes_the_expected_bits(group):
    for c in F.GROUPS[group]:
        m = F.model(c)
        ref_rows = F.from_heads(np.ascontiguousarray(m.ref), c)
        for mu in F.MUTANTS:
            if not F.applies(c, mu):
                continue
            mm = F.model(c, mu)
            assert not np.array_equal(mm.out, m.out), (c.name, mu, "the mutant leaves the expected bits unchanged")
            ratio = F.block_ratio(mm.emul, m.ref, m.emul, c.dt)
            if c.family == "ints":
                if mu in B_BREAKERS:
                    assert (ratio > F.F_OP).any(), (c.name, mu, "the per-block rule does not see the mutant")
                old = F.rel_err(mm.out, ref_rows)
                assert not old < F.OLD_REL_ERR[c.dt], (c.name, mu, old)     # one magnitude everywhere: the old metric sees it too (NaN: it fails)
        assert not (F.block_ratio(m.emul, m.ref, m.emul, c.dt) > 1.0).any()


def test_the_old_metric_lets_mutant_8_through():
    """The sentence in the module text: the whole-tensor metric of tests/test_gpu_ops.py passes mutant 8 on the `route` cases named there
    (and mutant 7 on the dual-weight bf16 ones) while the bits change and the per-block rule fails."""
    passed = {7: [], 8: []}
    for c in F.CASES:
        if c.family != "route":
            continue
        m = F.model(c)
        ref_rows = F.from_heads(np.ascontiguousarray(m.ref), c)
        for mu in (7, 8):
            mm = F.model(c, mu)
            if F.rel_err(mm.out, ref_rows) < F.OLD_REL_ERR[c.dt]:
                assert not np.array_equal(mm.out, m.out) and (F.block_ratio(mm.emul, m.ref, m.emul, c.dt) > F.F_OP).any(), (c.name, mu)
                passed[mu].append(c)
    count = lambda cs, kernel, dt: sum(c.kernel == kernel and c.dt == dt for c in cs)
    assert [count(passed[8], k, t) for k in F.KERNELS for t in F.DTYPES] == [8, 0, 8, 6], [c.name for c in passed[8]]
    assert [count(passed[7], k, t) for k in F.KERNELS for t in F.DTYPES] == [0, 0, 8, 0], [c.name for c in passed[7]]
