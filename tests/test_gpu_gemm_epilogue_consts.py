"""The per-tile epilogue constants of gemm_w2f8_kernel (row statistics, bias, column sums), which every wave requests at the top of a
tile and hands to its epilogue through LDS: a constant that is stale, belongs to the neighbouring tile or comes from the wrong lane is
off by O(1), so every row gets its own (mean, rstd), every column its own bias and column sum, and the shapes make consecutive tiles
of one block differ in their row AND column origin.  Through ofx_gemm_w2f8_fold, the op-level entry of the LayerNorm-fold consumer
epilogue (qkv and fc1 of the ViT layers)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

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


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return torch.cuda.current_stream().cuda_stream


def _e4m3_decode(b):
    b = b.astype(np.int64)
    s, e, m = b >> 7, (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    return np.where(s == 1, -v, v)


def _weights(g, N, K):
    """Split f16 weights [N, hi(K) | lo(K)], their fp8 lo copy + scale bytes, and (hi, lo as the kernel sees it) in float64."""
    lib = L.load()
    src = dev((g.standard_normal((N, K), dtype=np.float32) / np.float32(np.sqrt(K))).astype(np.float32))
    W2 = torch.empty(N, 2 * K, dtype=torch.float16, device="cuda")
    L.check(lib.ofx_convert(src.data_ptr(), W2.data_ptr(), N, K, 3, 2, stream()))
    W8 = torch.zeros(N, K, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(N, dtype=torch.uint8, device="cuda")
    L.check(lib.ofx_pack_lo8(W2.data_ptr(), W8.data_ptr(), sc.data_ptr(), N, K, stream()))
    torch.cuda.synchronize()
    b = W8.cpu().numpy().reshape(N, K // 128, 4, 4, 8)                 # [n][block][g][s][j] <- k = 32 s + 8 g + j
    nat = _e4m3_decode(b).transpose(0, 1, 3, 2, 4).reshape(N, K)
    scb = sc.cpu().numpy().reshape(N // 128, 16, 8)                    # [(n >> 7)][n & 15][(n >> 4) & 7]
    n = np.arange(N)
    sw = 127 - scb[n >> 7, n & 15, (n >> 4) & 7].astype(np.int64)
    return W2, W8, sc, W2[:, :K].double().cpu().numpy(), nat * 2.0 ** (-sw[:, None].astype(np.float64))


def _recorded_kinds(lib, cap=16):
    recs = (L.ProfRecord * cap)()
    n = lib.ofx_profile_records(recs, cap)
    ms, fl, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_longlong * 4)()
    L.check(lib.ofx_profile_read(ms, fl, cnt))
    return [recs[i].kind for i in range(n)]


# (M, N, K): a single one-row tile of one super-step; two tiles that differ in the column tile only; six tiles with a ragged last row
# panel (one block walking all of them meets every (m0, n0) transition and both ways into a tile: after a full and after a ragged
# one; four blocks: two tiles beside one); the bench's K (six super-steps).  Every shape runs on grids of 1 and 4 blocks and one
# block per CU (= one per tile here).
SHAPES = [(1, 256, 128), (255, 512, 128), (600, 512, 256), (600, 768, 768)]
GRIDS = (1, 4, -1)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fold_consumer_epilogue_takes_each_tiles_own_constants(M, N, K, act):
    """ofx_gemm_w2f8_fold = act(((A hi^T + bf8(A) lo_seen^T) - col_sum mean) rstd + bias) in f16, forced onto gemm_w2f8_kernel:
    (a) the epilogue straight from the accumulators (ofx_tune(18, 1)) and the one through LDS (18, 0) agree bit for bit, (b) so do
    persistent grids of 1, 4 and one block per CU, (c) against float64 arithmetic on the quantised operands to 1e-3 - the f16
    rounding of the output (2^-11) and the fp32 accumulation; a wrong constant is off by O(1) - and the columns beyond N of a
    wider row stay untouched."""
    g = np.random.default_rng(1000 * act + M + N + K)
    ldc = N + 64
    A = dev(g.standard_normal((M, K), dtype=np.float32)).half().contiguous()
    W2, W8, sc, hi, lo_seen = _weights(g, N, K)
    mean = g.standard_normal(M).astype(np.float32)
    rstd = g.uniform(0.5, 2.0, M).astype(np.float32)
    stat = dev(np.stack([mean, rstd], 1))
    bias_h = g.standard_normal(N).astype(np.float32)
    csum_h = g.standard_normal(N).astype(np.float32)
    bias, csum = dev(bias_h), dev(csum_h)
    lib = L.load()
    outs = {}
    lib.ofx_tune(2, 6)
    lib.ofx_profile_enable(1)
    try:
        for grid in GRIDS:
            lib.ofx_tune(11, grid)
            for direct in (1, 0):
                lib.ofx_tune(18, direct)
                out = torch.full((M, ldc), -7.0, dtype=torch.float16, device="cuda")
                L.check(lib.ofx_gemm_w2f8_fold(A.data_ptr(), W2.data_ptr(), W8.data_ptr(), sc.data_ptr(), out.data_ptr(), bias.data_ptr(),
                                               stat.data_ptr(), csum.data_ptr(), M, N, K, K, ldc, act, stream()))
                torch.cuda.synchronize()
                outs[(grid, direct)] = out
        kinds = _recorded_kinds(lib)
    finally:
        lib.ofx_profile_enable(0); lib.ofx_tune(2, 0); lib.ofx_tune(11, -1); lib.ofx_tune(18, 1)
    assert kinds == [8] * (2 * len(GRIDS))                               # gemm_w2f8_kernel ran every time
    A8 = A.float().clamp(-57344.0, 57344.0).to(torch.float8_e5m2).double().cpu().numpy()
    z = A.double().cpu().numpy() @ hi.T + A8 @ lo_seen.T
    z = (z - csum_h.astype(np.float64)[None, :] * mean.astype(np.float64)[:, None]) * rstd.astype(np.float64)[:, None] + bias_h.astype(np.float64)[None, :]
    want = z / (1.0 + np.exp(-1.702 * z)) if act else z
    first = outs[(GRIDS[0], 1)]
    for key, out in outs.items():
        got = out.float().cpu().numpy()
        err = rel_err(got[:, :N], want)
        print(f"fold epilogue {M}x{N}x{K} act {act} grid {key[0]} direct {key[1]}: rel.err {err:.2e}")
        assert (got[:, N:] == -7.0).all(), key                           # nothing written beyond the N columns of a wider row
        assert err < 1e-3, (key, err)                                    # (c), for every grid and both epilogues
        assert torch.equal(out, first), key                              # (a) and (b)
