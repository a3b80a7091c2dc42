"""The FORWARD epilogues of every NT GEMM kernel, element by element and route by route (tests/gemm_epilogue_cases.py holds the case
table, the inputs and the float64 model; tests/test_cpu_gemm_epilogue_exact.py checks what the cases claim and that each modelled
defect - a neighbour's constant, a rounding mode, a swapped column group, a wrong activation constant ... - fails here).  The
accumulator of every case is exact (tests/gemm_exact_cases.py's condition), so all the freedom the kernels have is in the epilogue.

HOW EACH OUTPUT IS JUDGED
  A1 - A5 (lattice: integer bias / residual / col_sum / mean, rstd a power of two)   bit equality with torch's round-to-nearest-even cast of
      the float64 value (fp32 outputs: == on values); out_kind 2: the three column blocks are hi = cast(v), lo = cast(fp32(v - hi)), hi.
      A2 plants ties in both directions, their neighbours, 65504 / 65519 / 65520 (-> inf, as torch) at every (row mod 16, column mod 64).
  B (real-valued constants)   per element |got - float64| <= one half-ulp per fp32 operation of epi_value / epi_residual (real_bound:
      s1 = acc + bias, s2 = s1 + resid; fold: t1 = cs mu, t2 = acc - t1, t3 = t2 rs, t4 = t3 + bias - an earlier error scaled by rs),
      + half an ulp of T for operand-type outputs; out_kind 1 == torch's cast of THE SAME ROUTE'S fp32 run, out_kind 2 == (hi, lo, hi)
      of it, bit for bit (the check that catches a multiply or an add merged into the conversion).
  C (activations, pre-activation u a known multiple of 2^-6)   per element |got - f64(u)| <= 4 x E_act(u) + FLT_MIN, E_act the error of
      a float32 step-by-step emulation of ofx_common.h's formula (act_bound: maximum over the 64 neighbouring sweep points, at least
      half an fp32 ulp); with a residual the fp32 output == fp32(no-residual output + r) bit for bit; out_kind 1 == cast(fp32 run).
  Everywhere: the routes of one operand set return THE SAME BITS on the rows they share; C beyond N (3 N) and the guard rows behind
  row M keep their payload NaN; the profile record names the kernel of the case's plan.  The record has no field for the epilogue a
  kind-8 launch took: which one it is (epilogue_direct under ofx_tune(18, 1) for out_kind 1 without residual and with act 0 - 2)
  follows from the plan's epi_direct, which the CPU test holds against tests/gemm_plan_ref.py, and both settings must agree to the bit.

WHICH PATH EACH CASE REACHES (routes of gemm_epilogue_cases.ROUTES)
  k1, k5, wrap     `epilogue` of gemm_128x128_kernel: 128-row tiles, 64-row tiles (32 rows per wave), the wrapping A index of split weights
  k2, k3, k4, k6   epilogue2 NP 8 / JW 4 (256 x 256, 256 x 128, ping-pong, dual-weight); k9: NP 4 / JW 4 (gemm_x3_kernel)
  k8               gemm_w2f8_kernel with ofx_tune(18, 0): epilogue2 NP 4 / JW 8, both J0 halves, constants from the cst slot
  k8d              the same with ofx_tune(18, 1): epilogue_direct for out_kind 1 / no residual / act 0 - 2, else epilogue2 again (Mish, a
                   residual, fp32 and split3 outputs must fall through and still be right)
  splitk           two slices + splitk_reduce_kernel (run-time act; no bias = the -0.0 addend)
  fp32 + residual + act none is RAMP 1 of epilogue2 (A4, B), every other fp32 case RAMP 0; operand-type outputs are store8 (store4 in
  `epilogue` and the reduce); A5 / B fold cases: ofx_gemm_fold w_form 0 / 1 and ofx_gemm_w2f8_fold, stat_ld 1 and 3 (A rows 3 K
  wide), odd and even M (the (ra, rb) pair load clamping one row, both, none), 769 x 512 on a 3-block persistent grid.
  ofx.h says out_kind 2 is "bf16 only"; the launcher does not enforce it and the kernels do the same thing for f16: A3 / B hold f16
  to the same rule.
  -0.0 as an INPUT (pre-activation, planted target) does not occur: gemm_epilogue_cases.py says why.

Refusals (a rejected call launches nothing) are held once each at the bottom; "a fold role with a residual" is already held by
tests/test_gpu_fold_ops.py::test_refused_calls_launch_nothing (the producer entry, the only fold entry that takes a residual).

MEASURED on the MI355X (742 launches, 3.3 s for the file)
  Parts A1 - A5: every bit right on the first run, on every route, both types, every M, the planted 65520 -> inf included.
  Part B: worst |err| / bound 1.000 (plain fp32 and fold consumer: a single rounding does reach its half-ulp among 33,000 elements);
      out_kind 1 / 2 == cast / (hi, lo, hi) of the route's own fp32 run everywhere: no conversion is merged with the arithmetic.
  Part C: worst |err| / E_act against F = 4:  QuickGELU 1.38 (u = 1.65625),  GELU 1.46 (u = -0.8125),  Mish 1.18 (u = -0.765625).
      The Mish yardstick takes __expf for what it is, v_exp_f32(u log2(e)): the fp32 product's rounding is |u| log2(e) 2^-24 relative in
      e^u (6 ulp at u = -18), and against an emulation with a correctly rounded exp the kernel reads 41 x E_act at u = -61.4
      (printed, not asserted) - the same two operations act_quick_gelu writes out, where the emulation had them from the start.
  Route pairs: every pair agreed to the bit on the first run but the two below.

FIRST RUN: what failed, and why
  1. The test's own yardstick: E_act's window of "64 neighbouring sweep points" ran over the sorted ELEMENTS, which repeat each value of
     u a dozen times, so it held five distinct points, not 64, and fell to its half-ulp floor where the emulation's error is several
     ulps (QuickGELU 4.3 at u = -5.09, whose exponent's argument 12.5 is itself rounded).  The window now runs over distinct values.
  2. Mish read 54 - 60 x E_act for u < -15 with numpy's exp in the emulation: see MEASURED.  F did not move.
  3. Sign of zero.  epilogue2's fp32 branch adds its prefetched residual register, +0 without a residual, unconditionally (its comment:
     "-0.0 leaves as +0.0"): GELU for u < -5.6, QuickGELU and Mish in the far tail return -0 on `epilogue`, the split-K reduce and every
     operand-type store, +0 from epilogue2 in fp32.  fp32 outputs are therefore compared with a zero equal to a zero of either sign
     (_differ32, _differ_cast); the operand-type outputs must carry the sign of u on every route, and do.
  4. Fold consumer on real constants, `epilogue` (kinds 1, 5) against epi_value's routes: ONE element of 16,384 differs in the f16 /
     bf16 output.  Both chains are the same C expression, (v - cs mu) rs + bias; the compiler contracts `v - cs mu` into an FMA in
     both, and the closing `* rs + bias` into an FMA in epi_value's routes only - in `epilogue` it stays a multiply and an add
     (_fold_forms: the bits of kinds 2, 3, 4, 6, 8 - both epilogues of 8 - match "fma on / on" with no mismatch, those of kinds 1 and 5
     match "fma on / off").  One rounding more or less, both inside real_bound.  The kernels stay as they are (making the two agree
     would change the bits one of them computes today): this pair's bit agreement is replaced by the bound, which every element of
     both meets, and the routes agree bit for bit within each of the two classes (SHARED's last key field).  On the lattice (A5) the
     two are bit-identical, as every intermediate is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_epilogue_cases as E
import gemm_exact_cases as X

pytestmark = pytest.mark.gpu

L = None
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 2
OFX_EINVAL, OFX_ESHAPE = -1, -2
SHARED = {}          # (part, operand set, type, N, out_kind, act, resid, bias, fold) -> (case name, output rows): the routes must agree
FP32_RUNS = {}       # (route, type, part, M, N, act, resid, fold) -> the route's own fp32 output
MEASURED = {}        # what the docstring reports: key -> (worst figure so far, where)
FORMS = {}           # part B, fold consumer: case -> mismatches against each contraction of the chain


@pytest.fixture(scope="module", autouse=True)
def _lib():
    global L
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from outfitx_amd import _lib as lib
    lib.load()
    L = lib
    yield


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, td=None):
    t = torch.from_numpy(np.array(a)).cuda()                # a copy: the case arrays are read-only
    return t if td is None else t.to(td).contiguous()


def _recorded_kinds(lib, cap=16):
    recs = (L.ProfRecord * cap)()
    n = lib.ofx_profile_records(recs, cap)
    ms, fl, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_longlong * 4)()
    L.check(lib.ofx_profile_read(ms, fl, cnt))
    return [recs[i].kind for i in range(n)]


def _poisoned(rows, cols, out_kind):
    if out_kind == 0:
        return torch.full((rows, cols), E.POISON32, dtype=torch.int32, device="cuda")
    return torch.full((rows, cols), E.POISON16, dtype=torch.int16, device="cuda")


def _operands(c, d):
    r = E.ROUTES[c.route]
    t = {"A": dev(d["A"], TD[c.dt]), "W": dev(d["W"], TD[c.dt])}
    if r.oset == "w" and c.dt == "f16":
        # precondition (it FAILS, it does not skip): the packed e4m3 image of lo, decoded, is lo itself
        t["W8"], t["sc"], lo_seen, _ = X._pack_lo8(L, t["W"], c.N, c.K)
        assert np.array_equal(lo_seen, d["lo"].astype(np.float64)), c.name
    return t


def _launch(lib, c, d, t):
    """One launch of case c -> C [M, width] on the host (int32 bit patterns for fp32 outputs, int16 else), after the guards were checked."""
    r = E.ROUTES[c.route]
    M, N, K = c.M, c.N, c.K
    out = _poisoned(M + GUARD, c.ldc, c.out_kind)
    bias = dev(d["bias"]) if d["bias"] is not None else None
    bptr = bias.data_ptr() if bias is not None else None
    res = dev(d["resid"]) if d["resid"] is not None else None
    rptr = res.data_ptr() if res is not None else None
    A, W, op, lda = t["A"], t["W"], X.OP_DTYPE[c.dt], E.lda(c)
    keep = []
    for k, v in E.knobs(c):
        L.check(lib.ofx_tune(k, v))
    lib.ofx_profile_enable(1)
    try:
        if c.fold:
            stat, csum = dev(d["stat"]), dev(d["csum"])
            keep += [stat, csum]
            if r.w_form == 2:
                assert c.stat_ld == 1
                rc = lib.ofx_gemm_w2f8_fold(A.data_ptr(), W.data_ptr(), t["W8"].data_ptr(), t["sc"].data_ptr(), out.data_ptr(), bptr, stat.data_ptr(), csum.data_ptr(),
                                            M, N, K, lda, c.ldc, c.act, stream())
            else:
                rc = lib.ofx_gemm_fold(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, stat.data_ptr(), c.stat_ld, csum.data_ptr(), M, N, K, lda, c.ldc, c.act,
                                       r.w_form, op, stream())
        elif r.api == "gemm":
            rc = lib.ofx_gemm(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, lda, c.ldc, c.ldr, c.act, c.out_kind, op, stream())
        elif r.api == "splitk":
            nb = lib.ofx_gemm_splitk_ws(M, N, K)
            assert nb >= 2 * M * N * 4, (c.name, nb)
            slab = torch.empty(nb, dtype=torch.uint8, device="cuda")
            keep.append(slab)
            rc = lib.ofx_gemm_splitk(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, lda, c.ldc, c.ldr, c.act, c.out_kind, op, slab.data_ptr(), nb, stream())
        elif r.api == "w2":
            rc = lib.ofx_gemm_w2(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, lda, c.ldc, c.ldr, c.act, c.out_kind, op, stream())
        elif r.api == "w2f8":
            rc = lib.ofx_gemm_w2f8(A.data_ptr(), W.data_ptr(), t["W8"].data_ptr(), t["sc"].data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, lda, c.ldc, c.ldr, c.act,
                                   c.out_kind, stream())
        else:
            rc = lib.ofx_gemm_x3(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, lda, c.ldc, c.ldr, c.act, c.out_kind, op, stream())
        L.check(rc, c.name)
        torch.cuda.synchronize()
        kinds = _recorded_kinds(lib)
    finally:
        lib.ofx_profile_enable(0)
        for k, _ in E.knobs(c):
            lib.ofx_tune(k, E.KNOB_DEFAULTS[k])
    assert kinds == [E.plan(c)[0]], (c.name, kinds)
    if res is not None:
        assert torch.equal(res.view(torch.int32), dev(d["resid"]).view(torch.int32)), c.name           # the residual is only read
    got = out.cpu().numpy()
    width = 3 * N if c.out_kind == 2 else N
    poison = np.int32(E.POISON32) if c.out_kind == 0 else np.uint16(E.POISON16).astype(np.int16)
    assert (got[:M, width:] == poison).all(), f"{c.name}: columns of C between {width} and ldc were written"
    assert (got[M:] == poison).all(), f"{c.name}: rows of C behind row M were written"
    return np.ascontiguousarray(got[:M, :width])


def _where(c, bad):
    """Where the elements of the boolean [M, width] array `bad` lie: count, first (m, n), in-tile rows and columns."""
    idx = np.argwhere(bad)
    _, tm, tn, _, _ = E.plan(c)
    m, n = idx[0]
    return (f"{len(idx)} of {bad.size} elements; first at (m, n) = ({m}, {n}); in-tile rows {int((idx[:, 0] % tm).min())}..{int((idx[:, 0] % tm).max())}, "
            f"columns {int((idx[:, 1] % tn).min())}..{int((idx[:, 1] % tn).max())} (mod 64: {sorted(set((idx[:, 1] % 64).tolist()))[:16]}, rows mod 16: {sorted(set((idx[:, 0] % 16).tolist()))})")


def _f32(bits):
    return bits.view(np.float32)


def _differ32(a, b):
    """fp32 outputs (int32 patterns): different bits, but a zero equals a zero of either sign - epilogue2's fp32 branch adds its
    prefetched residual register, +0 without a residual, unconditionally, and -0 + +0 = +0 (its own comment says so)."""
    return (a != b) & ~((_f32(a) == 0) & (_f32(b) == 0))


def _differ_cast(got, own32, dt):
    """Operand-type output against torch's cast of the route's own fp32 run; where that run is a zero, a zero of either sign."""
    want = E.torch_cast(own32, dt)
    return (got != want) & ~((own32 == 0) & ((got & 0x7fff) == 0))


def _split3_of(v32, c):
    hi = E.torch_cast(v32, c.dt)
    with np.errstate(invalid="ignore"):
        lo = E.torch_cast((v32.astype(np.float64) - E.decode(hi, c.dt)).astype(np.float32), c.dt)
    return np.concatenate([hi, lo, hi], 1)


def _fold_forms(c, d, got):
    """Which contraction of (acc - cs mu) rs + bias the route's bits are consistent with: mismatches per form (an FMA = one rounding of the
    exact product-sum, formed in float64: the 48-bit product is exact there)."""
    f, z = np.float32, d["z"]
    mu, rs, cs = d["mean"].astype(np.float64)[:, None], d["rstd"].astype(np.float64)[:, None], d["csum"].astype(np.float64)[None, :]
    bias = d["bias"].astype(np.float64)[None, :]
    out = {}
    for fma1 in (0, 1):
        for fma2 in (0, 1):
            t2 = (z - cs * mu).astype(f) if fma1 else (z - (cs * mu).astype(f).astype(np.float64)).astype(f)
            v = (t2.astype(np.float64) * rs + bias).astype(f) if fma2 else ((t2.astype(np.float64) * rs).astype(f).astype(np.float64) + bias).astype(f)
            out[f"fma {'on' if fma1 else 'off'} / {'on' if fma2 else 'off'}"] = int((E.torch_cast(v, c.dt) != got).sum())
    return out


def _note(key, value, where=""):
    if key not in MEASURED or value > MEASURED[key][0]:
        MEASURED[key] = (value, where)


def _judge(c, d, got, errors):
    N = c.N
    fkey = (c.route, c.dt, c.part, c.M, c.N, c.act, c.resid, c.fold)
    if c.part in ("A1", "A2", "A3", "A4", "A4b", "A5"):
        want = E.expected(c, d)
        bad = (_f32(got) != want) if c.out_kind == 0 else (got != want)
        if bad.any():
            m, n = np.argwhere(bad)[0]
            shown = (_f32(got)[m, n], want[m, n]) if c.out_kind == 0 else (hex(int(got[m, n]) & 0xffff), hex(int(want[m, n]) & 0xffff))
            errors.append(f"{c.name}: {_where(c, bad)}: got {shown[0]}, want {shown[1]}")
        return
    if c.part == "B":
        ref, e = E.real_bound(c, d)
        if c.out_kind == 0:
            FP32_RUNS[fkey] = got
            err = np.abs(_f32(got).astype(np.float64) - ref)
            bad = ~(err <= e)
            _note(f"B fp32 worst |err| / bound ({'fold' if c.fold else 'plain'})", float((err / e).max()), c.name)
        elif c.fold:
            val = E.decode(got, c.dt)
            err, b = np.abs(val - ref), E.out_bound(ref, e, c.dt)
            bad = ~(err <= b)
            _note("B fold consumer worst |err| / bound", float((err / b).max()), c.name)
            FORMS[c.name] = _fold_forms(c, d, got)
        else:
            own = _f32(FP32_RUNS[fkey])
            want = E.torch_cast(own, c.dt) if c.out_kind == 1 else _split3_of(own, c)
            bad = got != want
        if bad.any():
            errors.append(f"{c.name}: {'bound' if (c.out_kind == 0 or c.fold) else 'cast of its own fp32 run'}: {_where(c, bad)}")
        return
    # ---- part C
    u = d["z"] + d["bias"].astype(np.float64)[None, :]
    if c.out_kind == 0 and c.resid == "none":
        FP32_RUNS[fkey] = got
        ref, b = E.act_bound(u, c.act)
        val = _f32(got).astype(np.float64)
        err = np.abs(val - ref)
        bad = ~(err <= b)
        unit = (b - E.FLT_MIN) / E.F_ACT
        ratio = np.where(np.isfinite(err), np.maximum(err - E.FLT_MIN, 0.0) / unit, np.inf)
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        _note(f"C act {c.act} worst |err| / E_act", float(ratio[i]), f"u = {float(u[i])!r} ({c.name})")
        if c.act == 3:
            _, b2 = E.act_bound(u, 3, "libexp")
            r2 = np.maximum(err - E.FLT_MIN, 0.0) / ((b2 - E.FLT_MIN) / E.F_ACT)
            j = np.unravel_index(np.argmax(r2), r2.shape)
            _note("C act 3 worst |err| / E_act were __expf a correctly rounded exp (not asserted)", float(r2[j]), f"u = {float(u[j])!r} ({c.name})")
        tail = np.abs(u) > 55
        if not np.isfinite(val[tail]).all():
            errors.append(f"{c.name}: NaN or inf in the far tails")
        if bad.any():
            m, n = np.argwhere(bad)[0]
            errors.append(f"{c.name}: bound: {_where(c, bad)}: u = {u[m, n]!r}, got {val[m, n]!r}, float64 {ref[m, n]!r}, bound {b[m, n]:.3e}, worst ratio {ratio[i]:.2f} at u = {u[i]!r}")
    elif c.out_kind == 0:
        FP32_RUNS[fkey] = got
        base = _f32(FP32_RUNS[(c.route, c.dt, c.part, c.M, c.N, c.act, "none", c.fold)])
        want = (base + d["resid"][:, :N]).astype(np.float32)
        bad = _differ32(got, want.view(np.int32))
        if bad.any():
            errors.append(f"{c.name}: fp32(activation + residual) of its own no-residual run: {_where(c, bad)}")
    else:
        bad = _differ_cast(got, _f32(FP32_RUNS[fkey]), c.dt)
        if bad.any():
            errors.append(f"{c.name}: cast of its own fp32 run: {_where(c, bad)}")
        if c.resid == "none":                     # no operand-type store loses the sign of a zero: -0 in the negative tails
            zero = (got & 0x7fff) == 0
            wrong = zero & ((got < 0) != np.signbit(u))
            if wrong.any() or not (zero & (got < 0)).any():
                errors.append(f"{c.name}: sign of zero: {_where(c, wrong) if wrong.any() else 'no -0 among the outputs'}")


def _order(cases):
    """fp32 runs first, the no-residual ones before the others: the later cases are judged against them."""
    return sorted(cases, key=lambda c: (c.out_kind != 0, c.resid != "none"))


@pytest.mark.parametrize("group", list(E.GROUPS))
def test_forward_epilogue(group):
    lib = L.load()
    ops, errors = {}, []
    for c in _order(E.GROUPS[group]):
        d = E.inputs(c)
        okey = (c.M, c.N, c.stat_ld)
        if okey not in ops:
            ops[okey] = _operands(c, d)
        got = _launch(lib, c, d, ops[okey])
        _judge(c, d, got, errors)
        # ---- every route of the operand set: the same bits on the rows they share
        # (part B, fold consumer: `epilogue` - kind 1 and 5 - and epi_value's routes are two classes, see FIRST RUN in the module text)
        skey = (c.part, E.ROUTES[c.route].oset, c.dt, c.N, c.out_kind, c.act, c.resid, c.bias, c.fold, c.part == "B" and c.fold and E.plan(c)[0] in (1, 5))
        name, first = SHARED.setdefault(skey, (c.name, got))
        rows = min(len(first), len(got))
        diff = _differ32(first[:rows], got[:rows]) if c.out_kind == 0 else first[:rows] != got[:rows]
        if diff.any():
            errors.append(f"{c.name} differs from {name}: {_where(c, diff)}")
    for k, (v, where) in sorted(MEASURED.items()):                     # the figures the docstring reports (run with -s)
        print(f"MEASURED {k}: {v:.3f} at {where}")
    for k, v in sorted(FORMS.items()):
        print(f"FORMS {k}: {v}")
    FORMS.clear()
    assert not errors, "\n".join(errors)


def test_refused_calls_launch_nothing():
    """ofx_launch_gemm's rules on the forward epilogue, through the op-level entries that can reach them: a fold consumer with Mish or
    MISH_GRAD (OFX_EINVAL), ldc < 3 N for out_kind 2, an ldc that is no multiple of 8 for an operand-type output, an ldr that is no
    multiple of 4 (OFX_ESHAPE).  Nothing is launched: the output keeps its poison and no profile record appears."""
    lib = L.load()
    M, N, K = 16, 256, 128
    a = torch.ones((M, K), dtype=torch.float16, device="cuda")
    w = torch.ones((N, 2 * K), dtype=torch.float16, device="cuda")
    f = lambda *s: torch.ones(s, dtype=torch.float32, device="cuda")
    bias, stat, csum, res = f(N), f(M, 2), f(N), f(M, N + 8)
    out = _poisoned(M + GUARD, 3 * N + 16, 1)
    before = out.clone()
    w8, sc = torch.zeros((N, K), dtype=torch.uint8, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    lib.ofx_profile_enable(1)
    try:
        for act in (3, 4):
            for form in (0, 1):
                assert lib.ofx_gemm_fold(a.data_ptr(), w.data_ptr(), out.data_ptr(), bias.data_ptr(), stat.data_ptr(), 1, csum.data_ptr(), M, N, K, K, N, act, form, 2,
                                         stream()) == OFX_EINVAL, (act, form)
            assert lib.ofx_gemm_w2f8_fold(a.data_ptr(), w.data_ptr(), w8.data_ptr(), sc.data_ptr(), out.data_ptr(), bias.data_ptr(), stat.data_ptr(), csum.data_ptr(),
                                          M, N, K, K, N, act, stream()) == OFX_EINVAL, act
        gemm = lambda ldc, ldr, ok, r=None: lib.ofx_gemm(a.data_ptr(), w.data_ptr(), out.data_ptr(), bias.data_ptr(), r, M, N, K, K, ldc, ldr, 0, ok, 2, stream())
        assert gemm(3 * N - 8, 0, 2) == OFX_ESHAPE and gemm(2 * N, 0, 2) == OFX_ESHAPE                  # ldc < 3 N for [hi | lo | hi]
        assert gemm(N + 4, 0, 1) == OFX_ESHAPE and gemm(3 * N + 4, 0, 2) == OFX_ESHAPE                  # operand outputs: ldc % 8
        assert gemm(N, N + 2, 1, res.data_ptr()) == OFX_ESHAPE and gemm(N, N + 2, 0, res.data_ptr()) == OFX_ESHAPE      # ldr % 4
        torch.cuda.synchronize()
        assert _recorded_kinds(lib) == []
    finally:
        lib.ofx_profile_enable(0)
    assert torch.equal(out, before), "a refused call wrote something"
