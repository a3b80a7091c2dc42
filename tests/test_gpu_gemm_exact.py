"""The main loops of every NT GEMM kernel - operand staging, the stage rotation over k-steps and over a persistent block's tiles, the
`kt % ka_tiles` wrap of split weights, the hi / lo / fp8 products, the split-K slices - on inputs for which every product and every
partial sum is exact in float32 (tests/gemm_exact_cases.py states the condition, tests/test_cpu_gemm_exact.py checks it and that each
case reaches the kernel it is meant for).  The result then does not depend on the summation order, so EVERY assertion here is bit
equality with the float64 product of the same arrays: fp32 output, integer bias, integer fp32 residual (in place unless the case says
otherwise).  Cases of one group that share their arrays (the grids of one shape; gemm_x3_kernel and the K-concatenated path) are
thereby bit-identical to each other as well.  With per-launch records on, the kernel that ran is the one the case names.

What this file leaves out - real-valued data, activations, the LayerNorm-fold epilogues and operand-type outputs - is held element by
element, on every route of the forward epilogue, by test_gpu_gemm_epilogue_exact.py (the training features and the fold producer by
test_gpu_bwd_ops.py and test_gpu_fold_ops.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_exact_cases as X

pytestmark = pytest.mark.gpu

L = None
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")


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
    t = torch.from_numpy(np.array(a)).cuda()
    return t if td is None else t.to(td).contiguous()


def _recorded_kinds(lib, cap=16):
    """Kernel kinds (GemmKind, csrc/gemm_plan.h) of the GEMM launches since ofx_profile_enable(1)."""
    recs = (L.ProfRecord * cap)()
    n = lib.ofx_profile_records(recs, cap)
    ms, fl, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_longlong * 4)()
    L.check(lib.ofx_profile_read(ms, fl, cnt))
    return [recs[i].kind for i in range(n)]


def _mismatch(c, got, want):
    """None when got == want bit for bit (as values: both are finite), else the message: count, first (m, n), the tiles and the in-tile
    row / column box of the mismatches, and for a census case the digit strings (one binary digit per 32-column step, step 0 first)."""
    bad = np.argwhere(got.astype(np.float64) != want)
    if bad.size == 0:
        return None
    _, tm, tn, _, _ = c.plan
    m, n = bad[0]
    tiles = sorted({(int(i) // tm, int(j) // tn) for i, j in bad})
    msg = (f"{c.name} knobs {dict(c.knobs)}: {len(bad)} of {got.size} elements differ; first at (m, n) = ({m}, {n}): got {got[m, n]!r}, want {want[m, n]!r}; "
           f"tiles (tile_m {tm}, tile_n {tn}) {tiles[:12]}{' ...' if len(tiles) > 12 else ''}; in-tile rows {int((bad[:, 0] % tm).min())}..{int((bad[:, 0] % tm).max())}, "
           f"columns {int((bad[:, 1] % tn).min())}..{int((bad[:, 1] % tn).max())}")
    if c.family == "census":
        msg += f"; census digits got {X.census_digits(float(got[m, n]), c)} want {X.census_digits(float(want[m, n]), c)}"
    return msg


def _launch(lib, c, d, t):
    """One launch of case c on the device tensors t (operands, shared by the cases with the same arrays) -> C [M, ldc] float32 on the host."""
    M, N, K = c.M, c.N, c.K
    ldc, ldr = d["ldc"], d["ldr"]
    out = torch.full((M, ldc), NAN, device="cuda")
    rbuf = None
    if c.resid == "inplace":
        out[:, :N] = t["resid"][:, :N]
        rptr = out.data_ptr()
    elif c.resid == "separate":
        rbuf = t["resid"].clone()
        rptr = rbuf.data_ptr()
    else:
        rptr, ldr = None, 0
    bptr = t["bias"].data_ptr() if c.bias else None
    A, W = t["A"], t["W"]
    op = X.OP_DTYPE[c.dt]
    slab = None
    for k, v in c.knobs:
        L.check(lib.ofx_tune(k, v))
    lib.ofx_profile_enable(1)
    try:
        if c.api == "gemm":
            rc = lib.ofx_gemm(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, d["lda"], ldc, ldr, 0, 0, op, stream())
        elif c.api == "splitk":
            nb = lib.ofx_gemm_splitk_ws(M, N, K)
            assert nb >= c.plan[3] * M * N * 4, (c.name, nb)                      # the slab covers the plan
            slab = torch.empty(nb, dtype=torch.uint8, device="cuda")
            rc = lib.ofx_gemm_splitk(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, d["lda"], ldc, ldr, 0, 0, op, slab.data_ptr(), nb, stream())
        elif c.api == "w2":
            rc = lib.ofx_gemm_w2(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, d["lda"], ldc, ldr, 0, 0, op, stream())
        elif c.api == "w2f8":
            rc = lib.ofx_gemm_w2f8(A.data_ptr(), W.data_ptr(), t["W8"].data_ptr(), t["sc"].data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, d["lda"], ldc, ldr, 0, 0, stream())
        else:
            rc = lib.ofx_gemm_x3(A.data_ptr(), W.data_ptr(), out.data_ptr(), bptr, rptr, M, N, K, d["lda"], ldc, ldr, 0, 0, op, stream())
        L.check(rc, c.name)
        torch.cuda.synchronize()
        kinds = _recorded_kinds(lib)
    finally:
        lib.ofx_profile_enable(0)
        for k, _ in c.knobs:
            lib.ofx_tune(k, X.KNOB_DEFAULTS[k])
    assert kinds == [c.plan[0]], (c.name, kinds)
    if rbuf is not None:
        assert torch.equal(rbuf.view(torch.int32), t["resid"].view(torch.int32)), c.name      # a separate residual is only read
    return out.cpu().numpy()


def _operands(lib, c, d):
    td = TD[c.dt]
    t = {"d": d, "A": dev(d["A"], td), "W": dev(d["W"], td)}
    if d["bias"] is not None:
        t["bias"] = dev(d["bias"])
    if d["resid"] is not None:
        t["resid"] = dev(d["resid"])
    if c.api == "w2f8":
        # precondition (it FAILS, it does not skip): the packed e4m3 image of lo, decoded, is lo itself
        t["W8"], t["sc"], lo_seen, sw = X._pack_lo8(L, t["W"], c.N, c.K)
        assert np.array_equal(lo_seen, d["b"][1].astype(np.float64)), c.name
        if c.family == "ints-fp8":
            assert sw[3] == 0 and (np.delete(sw, 3) == 4).all()
    return t


@pytest.mark.parametrize("group", list(X.GROUPS))
def test_gemm_main_loop_is_exact(group):
    lib = L.load()
    ops, first, errors, pins = {}, {}, [], []
    for c in X.GROUPS[group]:
        d = X.build(c)
        key = (id(d), c.dt)
        pins.append(d)                                        # keeps id(d) unique for the length of the test
        if key not in ops:
            ops.clear()                                       # one set of operands on the device at a time
            ops[key] = _operands(lib, c, d)
        got = _launch(lib, c, d, ops[key])
        assert np.isnan(got[:, c.N:]).all(), f"{c.name}: columns of C between N and ldc were written"
        got = got[:, :c.N]
        msg = _mismatch(c, got, d["want"])
        if msg:
            errors.append(msg)
        same = first.setdefault(key + (c.resid, c.bias), got)
        assert msg or np.array_equal(same, got)               # the same arrays: the same bits, whatever the grid or the kernel
    assert not errors, "\n".join(errors)
