"""What tests/gemm_epilogue_cases.py claims of every case, checked without a GPU: the exactness bound of the lattice parts, that the
operands survive the operand type (and E5M2 / e4m3 on the fp8 route), the rounding / tie counts of the wide bias, the position
coverage of the planted elements and of the activation sweep, that a plain np.float32 evaluation of the real-valued chain stays inside
the bound the GPU test will ask of the kernels, that the launch decision (tests/gemm_plan_ref.py) sends every case to the kernel, tile,
split count, grid and - kind 8 - the epilogue it is meant for, and that the suite is SHARP: each defect of the model (MUTANTS) changes
expected bits or breaks a bound on at least one case, while the unmutated model passes them all."""
import numpy as np
import pytest
import torch

import gemm_epilogue_cases as E
import gemm_plan_ref as R

TD = {"bf16": torch.bfloat16, "f16": torch.float16}
LATTICE = ("A1", "A2", "A3", "A4", "A4b", "A5")


def _roundtrip(a, td):
    return torch.from_numpy(np.array(a)).to(td).float().numpy()


def _is_tie(v, dt):
    r = np.abs(v) / E._quantum(v, dt)
    return (r - np.floor(r)) == 0.5


@pytest.mark.parametrize("group", list(E.GROUPS))
def test_every_case_is_what_it_claims_and_reaches_its_kernel(group):
    for c in E.GROUPS[group]:
        r, d = E.ROUTES[c.route], E.inputs(c)
        # ---- operands are what the operand type holds (the fp8 route: A in E5M2, lo 2^sw in e4m3)
        assert d["A"].shape == (c.M, E.lda(c)) and np.array_equal(_roundtrip(d["A"], TD[c.dt]), d["A"]) and np.array_equal(_roundtrip(d["W"], TD[c.dt]), d["W"]), c.name
        if c.M > E.ZERO_ROW:
            assert not d["A"][E.ZERO_ROW, :c.K].any() and not d["z"][E.ZERO_ROW].any()
        if r.api == "w2f8":
            a, lo = d["A"][:, :c.K], d["lo"]
            assert np.array_equal(_roundtrip(a, torch.float8_e5m2), a), c.name
            mx = np.abs(lo).max(1)
            sw = np.where(mx > 0, 8 - np.frexp(np.where(mx > 0, mx, 1.0))[1], 0)
            scaled = lo.astype(np.float64) * 2.0 ** sw[:, None]
            assert np.abs(scaled).max() <= 448 and np.array_equal(_roundtrip(scaled.astype(np.float32), torch.float8_e4m3fn), scaled), c.name
        # ---- strides and guards
        width = 3 * c.N if c.out_kind == 2 else c.N
        assert c.ldc == width + 8 and c.ldc % 8 == 0
        if d["resid"] is not None:
            assert c.ldr == c.N + 4 != c.ldc and d["resid"].shape == (c.M, c.ldr) and np.isnan(d["resid"][:, c.N:]).all()
        # ---- the launch it is meant for
        sh, kn = E.plan_inputs(c)
        p = R.gemm_plan(sh, kn)
        kind, tm, tn, splits, grid_x = E.plan(c)
        assert (p["kind"], p["tile_m"], p["tile_n"], p["splits"], p["grid_x"], p["grid_y"]) == (kind, tm, tn, splits, grid_x, splits), (c.name, p)
        assert p["epi_direct"] == r.direct and (not E.takes_direct(c) or kind == 8), c.name
        if r.api == "splitk":
            assert R.splitk_bytes(c.M, c.N, c.K, kn["splitk"]) >= splits * c.M * c.N * 4 > 0
        if c.grid is not None:
            assert p["nwg"] > grid_x and p["tiles_n"] == 2                # a block walks several tiles, of both column origins
        # ---- the exactness condition and what it buys: float32, every operation rounding, gives the float64 result
        if c.part in LATTICE:
            assert E.lattice_bound(c, d) < 2.0 ** 24, (c.name, E.lattice_bound(c, d))
            assert np.array_equal(E.value(c, d, FT=np.float32).astype(np.float64), E.value(c, d)), c.name
            if c.fold:                                                    # ... and so does the contracted form: fma(-cs, mu, acc), fma(t, rs, bias) in float64
                assert np.array_equal(E.value(c, d).astype(np.float32).astype(np.float64), E.value(c, d))
                assert len(set(zip(d["mean"].tolist(), d["rstd"].tolist()))) > 1 or c.M == 1
                m, n = np.arange(c.M - 1), np.arange(c.N - 16)
                assert ((d["mean"][m] != d["mean"][m + 1]) & (d["rstd"][m] != d["rstd"][m + 1])).all() and (d["csum"][n] != d["csum"][n + 16]).all()
        if c.part == "C":
            u_bound = (d["absz"] + np.abs(d["bias"]).astype(np.float64)[None, :]).max() * 64
            assert u_bound < 2.0 ** 24 and np.array_equal(np.rint(d["bias"] * 64) / 64, d["bias"]), c.name
        # ---- part A1 / A5: most elements round, and there are exact ties in both directions
        if c.part in ("A1", "A5") and c.M >= 64:
            v = E.value(c, d)
            hi = E.decode(E.torch_cast(v, c.dt), c.dt)
            fin = np.isfinite(hi)
            assert fin.mean() > 0.99 and (hi != v)[fin].mean() >= 0.5, (c.name, (hi != v).mean())
            ties = _is_tie(v, c.dt) & fin
            assert ties.sum() >= 32 and (hi > v)[ties].any() and (hi < v)[ties].any(), (c.name, int(ties.sum()))
        if c.part == "A3":
            v = E.value(c, d)
            hi = E.decode(E.torch_cast(v, c.dt), c.dt)
            lo = E.decode(E.torch_cast((v - hi).astype(np.float32), c.dt), c.dt)
            assert (lo != 0).mean() > 0.5 and len(np.unique(lo)) > 16, c.name             # lo is live
        if c.part == "A4" and c.M > E.ZERO_ROW:
            assert (E.value(c, d)[E.ZERO_ROW] == 0).sum() >= c.N // 3


def test_rnd_is_torchs_cast():
    """The numpy rounding the mutants are written in, against torch: every 16-bit pattern's neighbourhood and the overflow edge."""
    g = np.random.default_rng(0)
    v = np.concatenate([E.TARGETS, g.integers(-70000, 70000, 20000).astype(np.float64), g.standard_normal(20000) * 100, [65519.99, 65520.0, -65520.0, 1e-7, 6e-8, 0.0]])
    for dt in E.BOTH:
        assert np.array_equal(E.torch_cast(E.rnd(v, dt), dt), E.torch_cast(v, dt)), dt
        assert np.array_equal(E.half_ulp(np.array([1.0, 3000.0, 1e-30]), dt), 0.5 * np.array([2.0 ** (1 - E.FMT[dt][0]), 2.0 ** (12 - E.FMT[dt][0]), E._quantum(1e-30, dt)]))
    assert E.decode(E.torch_cast(np.array([65520.0, 65519.0, 65504.0]), "f16"), "f16").tolist() == [np.inf, 65504.0, 65504.0]


def test_planted_targets_reach_every_position_in_every_class():
    for dt in E.BOTH:
        hi = E.decode(E.torch_cast(E.TARGETS, dt), dt)
        tie = _is_tie(E.TARGETS, dt)
        assert (tie & (hi > E.TARGETS)).any() and (tie & (hi < E.TARGETS)).any() and (tie & (E.TARGETS < 0)).any(), dt
        t = set(np.flatnonzero(tie))
        assert any(i - 1 in t or i + 1 in t for i in np.flatnonzero(~tie & (hi != E.TARGETS))), dt      # one off a tie, and inexact
    f16 = E.decode(E.torch_cast(E.TARGETS, "f16"), "f16")
    assert {65504.0, 65519.0, 65520.0, -65520.0, 0.0} <= set(E.TARGETS.tolist()) and np.isinf(f16).sum() >= 4
    for c in (c for c in E.CASES if c.part == "A2"):
        d = E.inputs(c)
        bz = d["bias"].astype(np.float64)[None, :]
        target = d["z"] + bz + d["resid"][:, :c.N]
        cls = E.target_class(c.M, c.N)
        assert np.array_equal(target, E.TARGETS[cls]), c.name                                          # the planted sum IS the target, exactly
        assert np.array_equal(E.expected(c, d), E.torch_cast(E.TARGETS[cls], c.dt)), c.name
        if c.M >= 128:
            pos = (np.arange(c.M)[:, None] % 16) * 64 + np.arange(c.N)[None, :] % 64
            seen = np.zeros((len(E.TARGETS), 1024), bool)
            seen[cls, pos] = True
            assert seen.all(), c.name


WINDOWS = {"zero": (-0.75, 0.75), "plus one": (0.5, 1.5), "minus one": (-1.5, -0.5), "below 20": (19.0, 19.999), "above 20": (20.001, 21.0), "negative tail": (-8.0, -3.0)}

REGIONS = {"around 0 and +-1": (-1.5, 1.5), "around the threshold 20": (18.5, 21.5), "negative tail": (-8.0, -3.0)}


def test_activation_sweep_covers_its_windows_at_every_position():
    seen_sets = set()
    for c in (c for c in E.CASES if c.part == "C" and c.resid == "none" and c.out_kind == 0 and c.act == 1):
        key = (E.ROUTES[c.route].oset, c.M)
        if key in seen_sets:
            continue
        seen_sets.add(key)
        d = E.inputs(c)
        u = d["z"] + d["bias"].astype(np.float64)[None, :]
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
        pos = (np.arange(c.M)[:, None] % 16) * 64 + np.arange(c.N)[None, :] % 64
        for name, (lo, hi) in WINDOWS.items():
            w = (u >= lo) & (u <= hi)
            assert w.sum() >= 1000 and len(np.unique(u[w])) >= 30, (c.name, name, int(w.sum()))      # dense: most multiples of 2^-6 of the window
        for name, (lo, hi) in REGIONS.items():
            w = (u >= lo) & (u <= hi)
            assert len(np.unique(pos[w])) == 1024, (c.name, name, len(np.unique(pos[w])))              # at every (row mod 16, column mod 64)
        sweep = u[(u >= -24) & (u <= 24)]
        assert np.diff(np.unique(sweep)).max() <= 0.25 and sweep.min() <= -23.9 and sweep.max() >= 23.9, c.name
        assert (u[E.ZERO_ROW] == 0.0).any() and (u[E.ZERO_ROW] == 20.0).any() and (u == 20.0).sum() >= 2
        for t in (60.0, -60.0, 100.0, -100.0):
            assert (np.abs(u - t) < 3).sum() >= c.M // 2, (c.name, t)
        # the tails: the emulation (and any correct kernel) returns -0 / 0 / u there, never NaN or inf
        for act in (1, 2, 3):
            y = E.act_emul(u, act)
            assert np.isfinite(y).all()
            # (Mish(-60) = -60 e^-60 = -5e-25 is an ordinary fp32 number; below about -87 it is subnormal: the floor of the bound)
            assert (y[u > 55] == u[u > 55].astype(np.float32)).all() and (np.abs(y[u < -55]) < (1e-20 if act == 3 else 1e-45)).all() and np.signbit(y[u < -55]).all(), (c.name, act)


def test_plain_float32_evaluation_stays_inside_the_bounds():
    """The bounds are no tighter than the reference itself: part B's chain in np.float32 (nothing contracted) against real_bound, part
    C's emulation against act_bound, on every case."""
    for c in E.CASES:
        d = E.inputs(c)
        if c.part == "B":
            ref, e = E.real_bound(c, d)
            v32 = E.value(c, d, FT=np.float32).astype(np.float64)
            assert (np.abs(v32 - ref) <= e).all(), c.name
            assert (e <= 4 * 2.0 ** -24 * (np.abs(ref) + 200)).all()                                  # and no looser than a few ulps of the chain's largest term
            if c.out_kind:
                got = E.decode(E.torch_cast(v32.astype(np.float32), c.dt), c.dt)
                assert (np.abs(got - ref) <= E.out_bound(ref, e, c.dt)).all(), c.name
        if c.part == "C" and c.resid == "none" and c.out_kind == 0:
            u = d["z"] + d["bias"].astype(np.float64)[None, :]
            ref, b = E.act_bound(u, c.act)
            assert (np.abs(E.value(c, d, FT=np.float32, emul=True).astype(np.float64) - ref) <= b).all(), c.name


# ------------------------------------------------------------------------------------------------ the mutants
MUTANT_ROUTES = ("k1", "k8d", "splitk")
# where each defect can show at all: (part, extra condition on the case)
MUTANT_PARTS = {
    "bias_after_act": ("C",), "resid_before_act": ("C",), "qg17": ("C",), "gelu_tanh": ("C",), "mish_nothr": ("C",), "mish_thr15": ("C",),
    "bias_n^4": ("A1", "B"), "bias_n+64": ("A1", "B"), "stat_m^1": ("A5", "B"), "stat_m+1": ("A5", "B"), "rstd_first": ("A5", "B"), "csum_n+16": ("A5", "B"),
    "resid_ldc": ("A1", "A4", "B"), "trunc": ("A1", "A2"), "half_away": ("A1", "A2"), "double_round": ("A1", "A2"),
    "lo_other_element": ("A3",), "third_is_lo": ("A3",), "split3_stride": ("A3",), "swap8": ("A1", "A5"), "soffset_rows": ("A1", "A5"),
}
assert set(MUTANT_PARTS) == set(E.MUTANTS)


def _mutant_cases(mut):
    return [c for c in E.CASES if c.route in MUTANT_ROUTES and c.part in MUTANT_PARTS[mut] and c.M >= 64 and c.grid is None]


def _c_judgement(c, d, mut=""):
    """Part C on the CPU: the (mutated) float32 emulation stands in for a kernel -> (got, ref, bound), fp32 outputs."""
    u = d["z"] + d["bias"].astype(np.float64)[None, :]
    ref, b = E.act_bound(u, c.act)
    if d["resid"] is not None:
        ref = ref + d["resid"][:, :c.N].astype(np.float64)
        b = b + E.half_ulp(np.abs(ref) + b, "f32")
    return E.value(c, d, mut, FT=np.float32, emul=True).astype(np.float64), ref, b


def _detects(c, mut):
    d = E.inputs(c)
    if c.part in LATTICE:
        return not np.array_equal(E.expected(c, d, mut), E.expected(c, d))
    if c.part == "B":
        ref, e = E.real_bound(c, d)
        return not (np.abs(E.value(c, d, mut, FT=np.float32).astype(np.float64) - ref) <= e).all()
    if c.out_kind:
        return False
    got, ref, b = _c_judgement(c, d, mut)
    return not (np.abs(got - ref) <= b).all()


# mish_thr15: for 15 < u <= 20 the defect returns u instead of u tanh(softplus(u)); the two differ by 2 u e^(-2 u) <= 3e-12 there, a
# 10^-5 of half an fp32 ulp of u (4.8e-7).  No fp32 test can tell them apart: an EQUIVALENT mutant, asserted as such below.
EQUIVALENT = ("mish_thr15",)


@pytest.mark.parametrize("mut", E.MUTANTS)
def test_each_defect_is_seen(mut):
    hits = [c.name for c in _mutant_cases(mut) if _detects(c, mut)]
    if mut in EQUIVALENT:
        u = np.linspace(15.0, 20.0, 1001)
        assert not hits and (np.abs(u - E.act_ref(u, 3)) < 1e-5 * E.half_ulp(u, "f32")).all()
        return
    assert hits, mut
    if mut in E.STORE_MUTANTS:                      # epilogue_direct's own defects: seen on the route that takes it
        assert any(E.takes_direct(c) for c in _mutant_cases(mut) if c.name in hits), mut


def test_the_unmutated_model_passes_every_case():
    for c in E.CASES:
        assert not _detects(c, ""), c.name


# ------------------------------------------------------------------------------------------------ what the earlier metrics let through
def _old_metric_passes(c, d, mut):
    """The whole-tensor metrics the suite held this code to before (tests/test_gpu_ops.py, test_gpu_fold_ops.py,
    test_gpu_gemm_epilogue_consts.py), applied to the mutant's output on a new case: max |got - want| / max |want| < 1e-3 for a fold
    consumer, < 2e-5 for an fp32 output (3e-5 for hi + lo of out_kind 2), at most one ulp of T per element for out_kind 1."""
    with np.errstate(invalid="ignore", over="ignore"):
        if c.part == "C":
            got, want, _ = _c_judgement(c, d, mut)
            if c.out_kind:
                got = E.decode(E.torch_cast(got.astype(np.float32), c.dt), c.dt)
        elif c.part == "B":
            want = E.value(c, d)
            got = E.value(c, d, mut, FT=np.float32).astype(np.float64)
            if c.out_kind:
                got = E.decode(E.torch_cast(got.astype(np.float32), c.dt), c.dt)
        else:
            want = E.value(c, d)
            got = E.expected(c, d, mut)
            if c.out_kind == 2:
                got = E.decode(got[:, :c.N], c.dt) + E.decode(got[:, c.N:2 * c.N], c.dt)
            elif c.out_kind == 1:
                got = E.decode(got, c.dt)
            got = got.astype(np.float64)
        fin = np.isfinite(want) & (np.abs(want) < (60000 if c.dt == "f16" and c.out_kind else np.inf))
        err = np.abs(got - want)[fin]
        scale = max(np.abs(want[fin]).max(), 1e-30)
        if not np.isfinite(err).all():
            return False
        if c.fold:
            return err.max() / scale < 1e-3
        if c.out_kind == 1:
            return (err <= 2 * E.half_ulp(want[fin], c.dt)).all()
        return err.max() / scale < (3e-5 if c.out_kind == 2 else 2e-5)


LET_THROUGH = ("trunc", "half_away", "third_is_lo", "qg17", "gelu_tanh")


def test_which_defects_the_whole_tensor_metrics_let_through():
    """The justification of this file: of the defects above, the ones in LET_THROUGH pass the EARLIER metrics on every one of the new
    cases they apply to - a neighbour's (mean, rstd), a rounding mode, a swapped pair of column groups, a wrong activation constant are
    all within 1e-3 (fold consumer), 2e-5 (fp32) or one ulp (operand type) of the right tensor as a whole."""
    passed = []
    for mut in E.MUTANTS:
        cases = [c for c in _mutant_cases(mut) if mut in EQUIVALENT or _detects(c, mut)]
        if cases and all(_old_metric_passes(c, E.inputs(c), mut) for c in cases):
            passed.append(mut)
    assert tuple(passed) == LET_THROUGH, passed
