"""The glue between gemm_plan.h and the launches: ofx_launch_gemm launches what the header planned.  One op-level GEMM per kernel kind
at the smallest shape the kernel takes, with per-launch records on: the record's (M, N, logical K, kind, K multiplier, FLOPs, bytes)
equals what tests/gemm_plan_ref.py - the launch code as it stood before the header, which tests/test_gemm_plan.py pins the header to -
gives for that call.  Kinds 1-6 are forced with ofx_tune(2, v); 8 is reached from 6 by passing the fp8 weight copy, 9 by ofx_tune(15, 2).
What the kernels compute stays with the op-level tests of each of them (test_gpu_ops.py, test_gpu_fold_ops.py, test_gpu_bwd_ops.py)."""
import ctypes as C

import pytest
import torch

import gemm_plan_ref as R

pytestmark = pytest.mark.gpu

L = None
F16, BF16 = 2, 1


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


def _records(lib, cap=16):
    recs = (L.ProfRecord * cap)()
    n = lib.ofx_profile_records(recs, cap)
    ms, fl, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_longlong * 4)()
    L.check(lib.ofx_profile_read(ms, fl, cnt))
    return [(r.cat, r.M, r.N, r.K, r.kind, r.kmul, r.flops, r.bytes) for r in recs[:n]]


def _want(shape, knobs):
    p = R.gemm_plan(shape, knobs)
    return p, (0, shape["M"], shape["N"], p["k_logical"], p["kind"], p["kmul"], p["flops"], p["bytes"])


def _buf(rows, cols, dtype):
    return torch.zeros(rows, cols, dtype=dtype, device="cuda")


def test_every_kind_is_launched_and_recorded_as_planned():
    lib = L.load()
    M, N = 256, 256
    out = _buf(M, N, torch.float32)
    want, kinds = [], []
    lib.ofx_profile_enable(1)
    try:
        # kinds 1-5: the single-product kernels, K = 128, in both operand types
        for dt, td in ((BF16, torch.bfloat16), (F16, torch.float16)):
            A, W = _buf(M, 128, td), _buf(N, 128, td)
            for kind in (1, 2, 3, 4, 5):
                L.check(lib.ofx_tune(2, kind))
                L.check(lib.ofx_gemm(A.data_ptr(), W.data_ptr(), out.data_ptr(), None, None, M, N, 128, 128, N, 0, 0, 0, dt, stream()))
                p, w = _want(dict(M=M, N=N, K=128, f16=int(dt == F16)), dict(kernel=kind))
                want.append(w); kinds.append(kind)
                assert p["kind"] == kind
        # kinds 6 and 8: split weights [hi | lo], a_wrap = 128, f16; the fp8 copy of the lo half turns 6 into 8
        A, W2 = _buf(M, 128, torch.float16), _buf(N, 256, torch.float16)
        W8, sc = _buf(N, 128, torch.uint8), _buf(1, N, torch.uint8)
        L.check(lib.ofx_tune(2, 6))
        L.check(lib.ofx_gemm_w2(A.data_ptr(), W2.data_ptr(), out.data_ptr(), None, None, M, N, 128, 128, N, 0, 0, 0, F16, stream()))
        L.check(lib.ofx_gemm_w2f8(A.data_ptr(), W2.data_ptr(), W8.data_ptr(), sc.data_ptr(), out.data_ptr(), None, None, M, N, 128, 128, N, 0, 0, 0, stream()))
        for has_w8, kind in ((0, 6), (1, 8)):
            p, w = _want(dict(M=M, N=N, K=256, a_wrap=128, f16=1, has_w8=has_w8), dict(kernel=6))
            want.append(w); kinds.append(kind)
            assert p["kind"] == kind and p["kmul"] == 2 and p["k_logical"] == 128
        L.check(lib.ofx_tune(2, 0))
        # kind 9: three products, K = 3 x 64
        A3, W3 = _buf(M, 192, torch.bfloat16), _buf(N, 192, torch.bfloat16)
        L.check(lib.ofx_tune(15, 2))
        L.check(lib.ofx_gemm_x3(A3.data_ptr(), W3.data_ptr(), out.data_ptr(), None, None, M, N, 64, 192, N, 0, 0, 0, BF16, stream()))
        p, w = _want(dict(M=M, N=N, K=192, k_mult=3), dict(x3_kernel=2))
        want.append(w); kinds.append(9)
        assert p["kind"] == 9 and p["kmul"] == 3 and p["k_logical"] == 64
        L.check(lib.ofx_tune(15, 1))
        # a split-K plan: the first launch and the reduce share one record, kind 1
        Ms, Ns, Ks = 64, 512, 4096
        As, Ws, outs = _buf(Ms, Ks, torch.bfloat16), _buf(Ns, Ks, torch.bfloat16), _buf(Ms, Ns, torch.float32)
        slab_bytes = lib.ofx_gemm_splitk_ws(Ms, Ns, Ks)
        assert slab_bytes == R.splitk_bytes(Ms, Ns, Ks) > 0
        slab = _buf(1, slab_bytes, torch.uint8)
        L.check(lib.ofx_gemm_splitk(As.data_ptr(), Ws.data_ptr(), outs.data_ptr(), None, None, Ms, Ns, Ks, Ks, Ns, 0, 0, 0, BF16, slab.data_ptr(), slab_bytes, stream()))
        p, w = _want(dict(M=Ms, N=Ns, K=Ks, can_split=1), None)
        want.append(w); kinds.append(1)
        assert p["splits"] > 1 and p["second_pass"] == R.PASS_REDUCE and slab_bytes >= p["splits"] * Ms * Ns * 4
        torch.cuda.synchronize()
        got = _records(lib)
    finally:
        lib.ofx_profile_enable(0); lib.ofx_tune(2, 0); lib.ofx_tune(15, 1)
    assert [g[4] for g in got] == kinds
    assert got == want
