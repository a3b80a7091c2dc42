"""What tests/gemm_exact_cases.py claims of every case, checked without a GPU: the exactness condition (so that bit equality with the
float64 product is the right criterion on the device), that the operands survive the operand type (and E5M2 / e4m3 where the fp8
correction product reads them), that the guards are where the module says, and that the launch decision (tests/gemm_plan_ref.py, which
tests/test_gemm_plan.py pins to csrc/gemm_plan.h) sends the case to the kernel, tile height, split count and grid it is meant for."""
import numpy as np
import pytest
import torch

import gemm_exact_cases as X
import gemm_plan_ref as R

TD = {"bf16": torch.bfloat16, "f16": torch.float16}


def _roundtrip(a, td):
    return torch.from_numpy(np.array(a)).to(td).float().numpy()


@pytest.mark.parametrize("group", list(X.GROUPS))
def test_every_case_is_exact_representable_and_reaches_its_kernel(group):
    for c in X.GROUPS[group]:
        d = X.build(c)
        # ---- the exactness condition
        assert d["bound"] < 2.0 ** 24 * d["q"], (c.name, d["bound"])
        # ---- operands are what the operand type holds
        td = TD[c.dt]
        for blk in d["a"] + d["b"]:
            assert np.array_equal(_roundtrip(blk, td), blk), c.name
        op = np.where(np.isnan(d["A"]), np.float32(0), d["A"])
        assert np.array_equal(_roundtrip(op, td), op) and np.array_equal(_roundtrip(d["W"], td), d["W"]), c.name
        if c.family == "subnormal-lo":
            live = np.concatenate([b[b != 0] for b in d["b"]])
            assert c.dt == "f16" and live.size and np.abs(live).max() < 2.0 ** -14, c.name        # below f16's smallest normal
        if c.api == "w2f8":
            assert c.dt == "f16" and c.K % 128 == 0
            a, lo = d["a"][0], d["b"][1]
            assert np.array_equal(_roundtrip(a, torch.float8_e5m2), a), c.name                     # the kernel's image of A
            mx = np.abs(lo).max(1)
            sw = np.where(mx > 0, 8 - np.frexp(np.where(mx > 0, mx, 1.0))[1], 0)                    # ofx_pack_lo8: max |lo| 2^sw in [128, 256)
            scaled = lo.astype(np.float64) * 2.0 ** sw[:, None]
            assert np.abs(scaled).max() <= 448 and np.array_equal(_roundtrip(scaled.astype(np.float32), torch.float8_e4m3fn), scaled), c.name
            if c.family == "ints-fp8":
                assert (mx[np.arange(c.N) != 3] >= 8).all() and mx.max() <= 15 and mx[3] == 0 and (sw[mx > 0] == 4).all(), c.name
        # ---- guards
        kw = {"gemm": 1, "splitk": 1, "w2": 2, "w2f8": 2, "x3": 3}[c.api] * c.K
        ka = 3 * c.K if (c.api == "x3" or c.a3k) else c.K
        assert d["A"].shape == (c.M, d["lda"]) and d["W"].shape == (c.N, kw) and d["lda"] >= ka
        assert np.isfinite(d["A"][:, :ka]).all() and np.isnan(d["A"][:, ka:]).all()
        if c.a3k:
            assert not np.array_equal(d["A"][:, :c.K], d["A"][:, c.K:2 * c.K]) and not np.array_equal(d["A"][:, :c.K], d["A"][:, 2 * c.K:])
        if c.api == "x3":
            assert np.array_equal(d["A"][:, :c.K], d["A"][:, 2 * c.K:3 * c.K]) and np.array_equal(d["W"][:, :c.K], d["W"][:, c.K:2 * c.K])
        if d["resid"] is not None:
            assert np.isnan(d["resid"][:, c.N:]).all() and d["resid"].shape[1] == d["ldr"]
        if c.family == "census":
            assert X.census_digits(d["want"][0, 0], c) == "1" * (c.K // 32)
        # ---- the launch it is meant for
        sh, kn = X.plan_inputs(c)
        assert kn.get("splitk", 1) < 2 or kn["splitk"] & 0xff, c.name                            # a forced split plan names its slices
        p = R.gemm_plan(sh, kn)
        kind, tile_m, tile_n, splits, grid_x = c.plan
        assert (p["kind"], p["tile_m"], p["tile_n"], p["splits"], p["grid_x"], p["grid_y"]) == (kind, tile_m, tile_n, splits, grid_x, splits), (c.name, p)
        if c.api == "splitk":
            assert R.splitk_bytes(c.M, c.N, c.K, kn["splitk"]) >= splits * c.M * c.N * 4 > 0


def test_the_table_covers_what_it_is_for():
    """Every kernel kind, both operand types, every stage-count residue and walk length the issue names."""
    by_kind = {}
    for c in X.CASES:
        by_kind.setdefault((c.plan[0], c.plan[1]), set()).add(c.dt)
    for key in ((1, 128), (1, 64), (5, 64), (2, 256), (3, 256), (4, 256), (6, 256), (9, 256)):
        assert by_kind[key] == {"bf16", "f16"}, key
    assert by_kind[(8, 256)] == {"f16"}
    assert {(c.K // 32) % 3 for c in X.CASES if c.plan[0] in (6, 9) and c.family == "ints"} == {0, 1, 2}
    assert {c.plan[4] for c in X.CASES if c.plan[0] in (6, 8) and c.N == 512} == {3, 5, 8}
    assert {c.variant for c in X.CASES if c.family == "census"} == {"w", "hi", "lo", "w0", "w2"}
    assert {c.plan[0] for c in X.CASES if c.family == "subnormal-lo"} == {1, 6, 8, 9}


def test_reassociated_float32_sums_equal_the_integer_result():
    """The condition at work: float32 sums of one case's products in random chunk orders are bit-equal to the float64 `@`."""
    c = next(c for c in X.CASES if c.api == "x3" and c.K == 320 and c.family == "ints")
    d = X.build(c)
    g = np.random.default_rng(0)
    terms = np.concatenate([d["a"][0][:64, None, :] * d["b"][0][None, :64, :], d["a"][1][:64, None, :] * d["b"][0][None, :64, :],
                            d["a"][0][:64, None, :] * d["b"][1][None, :64, :]], 2).astype(np.float32)
    extra = d["bias"][None, :64] + d["resid"][:64, :64]
    for _ in range(4):
        acc = np.zeros((64, 64), np.float32)
        for chunk in np.array_split(g.permutation(terms.shape[2]), 7):
            part = np.zeros((64, 64), np.float32)
            for k in chunk:
                part += terms[:, :, k]
            acc += part
        assert np.array_equal((acc + extra).astype(np.float64), d["want"][:64, :64])


def test_split_k_knob_without_slices_is_refused():
    """ofx_tune(5, v) with v >= 2 and a zero low byte would force a plan of 0 slices (a division by zero in the planner): refused,
    and the knob keeps its value.  The library loads without a device; ofx_tune touches none."""
    from outfitx_amd import _lib
    lib = _lib.load()
    try:
        assert lib.ofx_tune(5, 0x103) == 0
        for bad in (256, 512, 0x300, 1 << 16):
            assert lib.ofx_tune(5, bad) == -1 and b"ofx_tune(5)" in lib.ofx_last_error()
        for ok in (0, 1, 2, 16, 255, 257):
            assert lib.ofx_tune(5, ok) == 0
    finally:
        assert lib.ofx_tune(5, 1) == 0
