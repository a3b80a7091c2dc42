"""fused_qkv_attn_kernel (csrc/fused_qkv_attn.hip; ofx_fused_qkv_attention and ofx_fused_qkv_attention_w2) on a real MI355X, through the C
ABI, on inputs for which q | k | v are known bit for bit (tests/fused_qkv_cases.py states the condition and the cases,
tests/test_cpu_fused_qkv_exact.py checks them and shows what each of eleven plausible slips of this kernel would change):

  A  `ints` cases: the output EQUALS the unfused pair's - projection GEMM (ofx_gemm | ofx_gemm_w2 | ofx_gemm_fold w_form 0 | 1, out_kind 1,
     the weight rows padded with zero rows to the GEMM's multiple of 128) -> ofx_attention on the same operands - value for value, no NaN
     (a -0 / +0 difference is not a finding).  Both run attn_scores / attn_softmax_p / attn_pv_store of csrc/attn_wave.h at NT = 4; with
     these operands both hold the same q | k | v bits, so anything but equality is a defect.  The GEMM's q | k | v are compared with the
     model's first: the precondition really held on the device.
  B  `ints` cases, per (image, head) block against float64: ||got - ref|| <= 1.6 max(||emul - ref||, 1e-2 u ||ref||), ref = attn_fwd_ref and
     emul = attn_fwd_emul (oracle/attn_fwd.py) on the model's q | k | v, u = 2^-8 bf16 | 2^-11 f16: factor and floor of the same wave core
     in tests/test_gpu_attention_fwd.py (F_OP), not retuned.
  C  `route` cases: the output is the model's routed v rows, value for value - no other kernel involved.
  D  in every call: two guard rows behind every output keep their bits, columns width .. ldo - 1 are still NaN, every written element is
     finite.
  E  refusals return what include/ofx.h and the launcher state and launch nothing.

MEASURED (MI355X), per kernel and operand type: 35 fused launches (27 `ints` + 8 `route`), 27 projection GEMMs and 27 ofx_attention calls.
                           A (27 calls)                      B worst ratio (factor 1.6)   C (8 calls)
  single-product  bf16     value for value in all 27 calls   1.002                        value for value in all 8 calls
  single-product  f16      value for value in all 27 calls   1.017                        value for value in all 8 calls
  dual-weight     bf16     value for value in all 27 calls   1.001                        value for value in all 8 calls
  dual-weight     f16      value for value in all 27 calls   1.023                        value for value in all 8 calls
  The unfused GEMM's q | k | v were the model's bits in all 108 calls; D held in all 140 + 108 + 108 calls; E: every refusal returned the
  stated code with `out` untouched.  B lands on the emulation (fp32 accumulation and the hardware exp2 are all that is left), as the same
  wave core does in tests/test_gpu_attention_fwd.py (worst 1.016 there).  No finding: nothing in csrc/ changed.
  The file: 46 tests, about 5.3 s, the slowest test 0.5 s (the first one: it loads the library).
"""
import functools

import numpy as np
import pytest
import torch

import fused_qkv_cases as F

pytestmark = pytest.mark.gpu

DT = {"bf16": 1, "f16": 2}
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 0x5AA5
L = None


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


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def dev(a, td=torch.float32):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(td).contiguous()


def ptr(t):
    return None if t is None else t.data_ptr()


def poisoned(rows, cols, td):
    """[rows + 2, cols] of NaN followed by two guard rows of GUARD bits -> the buffer and a copy of its bits."""
    buf = torch.full((rows + 2, cols), float("nan"), dtype=td, device="cuda")
    bits(buf)[rows:].fill_(GUARD if buf.element_size() == 2 else (GUARD << 16 | GUARD))
    return buf, bits(buf).clone()


def settle(buf, before, n_cols, label):
    """After the call (D): the guard rows and the columns from n_cols on keep their bits, every written element is finite -> the written
    columns as float64 numpy."""
    torch.cuda.synchronize()
    rows = buf.shape[0] - 2
    now = bits(buf)
    assert torch.equal(now[rows:], before[rows:]), (label, "guard rows")
    assert torch.equal(now[:rows, n_cols:], before[:rows, n_cols:]), (label, "a column past the width was written")
    vals = buf[:rows, :n_cols].double().cpu().numpy()
    assert np.isfinite(vals).all(), (label, "a written element is not finite", np.argwhere(~np.isfinite(vals))[:4].tolist())
    return vals


@functools.lru_cache(maxsize=2)
def _operands(c):
    d = F.build(c)
    td = TD[c.dt]
    return dict(X=dev(d["X"], td), W=dev(d["Wmat"], td), bias=dev(d["bias"]), stat=dev(d["stat"]) if c.fold else None,
                cs=dev(d["col_sum"]) if c.fold else None)


@functools.lru_cache(maxsize=None)
def fused(c):
    """One launch of the fused kernel on the case's arrays -> out [M, width] float64 after the buffer contract (D) is checked."""
    d, t, lib = F.build(c), _operands(c), L.load()
    fn = lib.ofx_fused_qkv_attention if c.kernel == "single" else lib.ofx_fused_qkv_attention_w2
    out, before = poisoned(d["M"], d["ldo"], TD[c.dt])
    L.check(fn(t["X"].data_ptr(), t["W"].data_ptr(), t["bias"].data_ptr(), ptr(t["stat"]), ptr(t["cs"]), out.data_ptr(), c.n_img, c.S, d["W"], c.heads,
               d["ldx"], d["ldo"], F.SCALE, DT[c.dt], stream()), c.name)
    vals = settle(out, before, d["W"], c.name)
    vals.setflags(write=False)
    return vals


def unfused(c, m):
    """GEMM -> ofx_attention on the same operands -> out [M, width] float64; the GEMM's q | k | v must be the model's."""
    d, t, lib = F.build(c), _operands(c), L.load()
    W, M, td = d["W"], d["M"], TD[c.dt]
    N = 3 * W
    Np = (N + 127) // 128 * 128                                            # the GEMMs want N % 128 == 0: zero weight rows behind the 3 W live ones
    Wp = torch.zeros(Np, t["W"].shape[1], dtype=td, device="cuda")
    Wp[:N] = t["W"]
    bias = torch.zeros(Np, device="cuda")
    bias[:N] = t["bias"]
    q2, qb = poisoned(M, Np, td)
    if c.fold:
        cs = torch.zeros(Np, device="cuda")
        cs[:N] = t["cs"]
        rc = lib.ofx_gemm_fold(t["X"].data_ptr(), Wp.data_ptr(), q2.data_ptr(), bias.data_ptr(), t["stat"].data_ptr(), 1, cs.data_ptr(), M, Np, W, d["ldx"], Np,
                               0, int(c.kernel == "dual"), DT[c.dt], stream())
    else:
        gemm = lib.ofx_gemm if c.kernel == "single" else lib.ofx_gemm_w2
        rc = gemm(t["X"].data_ptr(), Wp.data_ptr(), q2.data_ptr(), bias.data_ptr(), None, M, Np, W, d["ldx"], Np, 0, 0, 1, DT[c.dt], stream())
    L.check(rc, c.name + " projection GEMM")
    qkv = settle(q2, qb, Np, c.name + " projection GEMM")
    bad = np.argwhere(qkv[:, :N] != m.qkv)
    assert bad.size == 0, (c.name, "the unfused GEMM's q | k | v are not the model's", len(bad), bad[:4].tolist())
    assert not qkv[:, N:].any()
    o2, ob = poisoned(M, d["ldo"], td)
    L.check(lib.ofx_attention(q2.data_ptr(), o2.data_ptr(), None, c.n_img, c.S, c.heads, Np, d["ldo"], W, 2 * W, 0, 0, F.SCALE, DT[c.dt], stream()), c.name + " ofx_attention")
    return settle(o2, ob, W, c.name + " ofx_attention")


def _mismatch(c, got, want):
    """None when got == want as values, else the message: the count, the first element, and every (image, head) block that differs with its
    group, its wave and the rows and columns inside the block."""
    bad = got != want
    if not bad.any():
        return None
    G = F.group_size(c.S)
    blocks = F.to_heads(bad, c)
    lines = []
    for i, h in zip(*np.nonzero(blocks.any((-1, -2)))):
        r, col = np.nonzero(blocks[i, h])
        lines.append(f"image {i} (group {i // G}, wave {i % G}) head {h}: {len(r)} elements, rows {r.min()}..{r.max()}, columns {col.min()}..{col.max()}")
    row, col = np.argwhere(bad)[0]
    return (f"{c.name}: {int(bad.sum())} of {bad.size} elements differ in {len(lines)} of {c.n_img * c.heads} blocks; first at (row, column) = ({row}, {col}): "
            f"got {got[row, col]!r}, want {want[row, col]!r}\n  " + "\n  ".join(lines[:16]) + ("\n  ..." if len(lines) > 16 else ""))


INTS_GROUPS = [g for g, cs in F.GROUPS.items() if cs[0].family == "ints"]
ROUTE_GROUPS = [g for g, cs in F.GROUPS.items() if cs[0].family == "route"]


@pytest.mark.parametrize("group", INTS_GROUPS)
def test_fused_equals_the_unfused_pair_value_for_value(group):
    errors = []
    for c in F.GROUPS[group]:
        msg = _mismatch(c, fused(c), unfused(c, F.model(c)))
        if msg:
            errors.append(msg)
    c = F.GROUPS[group][0]
    print(f"EXACT A {c.kernel} {c.dt} {c.sweep}: {len(F.GROUPS[group]) - len(errors)} of {len(F.GROUPS[group])} calls value for value")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("group", INTS_GROUPS)
def test_fused_per_block_against_float64(group):
    worst, errors = 0.0, []
    for c in F.GROUPS[group]:
        m = F.model(c)
        ratio = F.block_ratio(F.to_heads(fused(c), c), m.ref, m.emul, c.dt)
        worst = max(worst, float(ratio.max()))
        G = F.group_size(c.S)
        errors += [f"{c.name}: image {i} (group {i // G}, wave {i % G}) head {h}: ratio {ratio[i, h]:.3g}" for i, h in zip(*np.nonzero(~(ratio <= F.F_OP)))]
    c = F.GROUPS[group][0]
    print(f"RATIO B {c.kernel} {c.dt} {c.sweep}: worst={worst:.3f} over {len(F.GROUPS[group])} calls")
    assert not errors, "\n".join(errors[:40])


@pytest.mark.parametrize("group", ROUTE_GROUPS)
def test_route_cases_return_the_routed_v_rows(group):
    errors = []
    for c in F.GROUPS[group]:
        msg = _mismatch(c, fused(c), F.model(c).out)
        if msg:
            errors.append(msg)
    c = F.GROUPS[group][0]
    print(f"EXACT C {c.kernel} {c.dt} route: {len(F.GROUPS[group]) - len(errors)} of {len(F.GROUPS[group])} calls value for value")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("kernel", F.KERNELS)
def test_refusals_launch_nothing(kernel):
    lib = L.load()
    fn = lib.ofx_fused_qkv_attention if kernel == "single" else lib.ofx_fused_qkv_attention_w2
    n, W, heads, ld = 2, 128, 2, 136
    X = torch.zeros(n * 65, ld, dtype=torch.float16, device="cuda")
    Wq = torch.zeros(3 * W, 2 * W, dtype=torch.float16, device="cuda")
    bias, stat = torch.zeros(3 * W, device="cuda"), torch.ones(n * 65, 2, device="cuda")
    out, before = poisoned(n * 65, ld, torch.float16)

    def call(S=50, width=W, h=heads, ldx=W, ldo=W, x=X.data_ptr(), st=None, c=None):
        rc = fn(x, Wq.data_ptr(), bias.data_ptr(), st, c, out.data_ptr(), n, S, width, h, ldx, ldo, F.SCALE, DT["f16"], stream())
        assert rc == F.admission(S, width, h, ldx, ldo, n, X=x is not None, row_stat=st is not None, col_sum=c is not None)
        return rc

    for S in F.REFUSED_S:
        assert call(S=S) == F.OFX_ESHAPE, S
    for S in (35, 36, 42):
        assert call(S=S) == F.OFX_ESHAPE and b"pad rows" in lib.ofx_last_error(), S
    assert call(width=64, h=1) == F.OFX_ESHAPE
    assert call(ldx=W + 4) == F.OFX_ESHAPE and call(ldo=W + 4) == F.OFX_ESHAPE and call(ldo=W - 8) == F.OFX_ESHAPE
    assert call(st=stat.data_ptr()) == F.OFX_EINVAL
    assert call(x=None) == F.OFX_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(bits(out), before), "a refused call wrote to out"

