"""Op-level float64 tests of the four attention kernels of the training step on a real MI355X, through the C ABI (ctypes):

  MFMA path (ofx_tune(7, 1), the default): attention_mfma_kernel in its varlen mode (cu_seqlens, only_row0, dropout on P)
                                           and set_attention_bwd_mfma_kernel          - ofx_attention_varlen, ofx_set_attention_bwd(mfma = 1)
  VALU path (ofx_tune(7, 0)):              set_attention_kernel<T, SMAX, T> on operand-type q | k | v with dropout
                                           and set_attention_bwd_kernel               - ofx_set_attention_op, ofx_set_attention_bwd(mfma = 0)

Reference: oracle/attn_train.py (plain numpy float64, pinned to float64 autograd by tests/test_cpu_attn_train_ref.py).

Accuracy is judged PER BLOCK - one (sequence, head, tensor in {O, dQ, dK, dV}), S x 64 values - so that one bad head, tile or sequence
cannot be averaged away.  For every block, relative to ||ref||:
    e_kernel = ||got - ref||,  e_emul = ||emul - ref||,   assert e_kernel <= F max(e_emul, 1e-2 u),   u = 2^-8 (bf16) | 2^-11 (f16)
where emul is the float64 computation with the kernels' stated roundings (dO, P . m and dS to the operand type before the products,
outputs to the operand type) and exact accumulation; the floor only keeps blocks with an accidentally tiny emulation error from dividing
by noise.  Blocks whose reference is identically zero (dQ and dK at S = 1, dQ rows > 0 under only_row0) must be exactly zero.

Shapes: n_head = 3 (D = 192), 7 sequences, so 21 (sequence, head) pairs: the last MFMA block has one live and three dead waves.
max_len 16 / 32 reach NT = 1 / 2 of the MFMA kernels and SMAX 20 / 32 of the VALU ones, max_len 8 the SMAX = 8 forward; lengths 1, 2,
one below, at and one above a 16-row tile, and the full 32.  Sequence 2 has q x 4 (a peaked softmax: the max subtraction).

MEASURED worst e_kernel / max(e_emul, 1e-2 u) over all 24 cases of a path (MI355X), per (path, dtype, tensor):
    mfma bf16: O 1.000  dQ 1.000  dK 1.000  dV 1.000      mfma f16: O 1.008  dQ 1.009  dK 1.003  dV 1.003
    valu bf16: O 1.000  dQ 0.993  dK 1.000  dV 1.000      valu f16: O 1.000  dQ 0.998  dK 0.991  dV 1.000
  worst per path 1.009 (MFMA; 1.008 without dropout) and 1.000 (VALU), the same with and without dropout.  The VALU kernels keep P . m
  and dS in fp32, so they sit at or below the emulation; the MFMA kernels land on it, as fp32 accumulation and exp2 (2^-20) should.
F = 1.5 x the worst ratio of the path, rounded up to one decimal (cap 3): F_MFMA = 1.6, F_VALU = 1.5.
Finding of the first run, fixed in set_attention_bwd_mfma_kernel: under dropout dK of a one-row set came out as the rounding error of
dP . m (3e-8 .. 5e-7 of ||dO||) instead of zero - the compiler fused that product into the softmax-backward subtraction in the
[query][key] orientation only.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import attn_train as A

pytestmark = pytest.mark.gpu

OFX_EINVAL, OFX_ESHAPE = -1, -2
H, DH = 3, 64
D = H * DH
SCALE = 0.125
SEED, SITE = 0xC0FFEE, 5
LENS = {8: [1, 2, 8, 5, 7, 3, 8], 16: [1, 2, 9, 16, 15, 7, 16], 32: [1, 17, 32, 16, 31, 2, 20]}
DT = {"bf16": 1, "f16": 2}
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
F = {"mfma": 1.6, "valu": 1.5}
GUARD = 0x5AA5                       # bit pattern of the two guard rows behind every output
TENSORS = ("O", "dQ", "dK", "dV")

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


def poisoned(rows, cols, dt):
    """[rows + 2, cols] operand type: NaN rows followed by two guard rows of GUARD bits; and a copy of its bits."""
    buf = torch.full((rows + 2, cols), float("nan"), dtype=TD[dt], device="cuda")
    buf[rows:].view(torch.int16).fill_(GUARD)
    return buf, buf.view(torch.int16).clone()


@functools.lru_cache(maxsize=None)
def inputs(max_len, dt):
    """Seeded q | k | v (operand type), dO (fp32), cu_seqlens - on the device and as float64 per-sequence [H, S, 64] stacks."""
    lens = LENS[max_len]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = int(cu[-1])
    g = np.random.default_rng(100 + max_len)
    qkv = g.standard_normal((rows, 3 * D), dtype=np.float32)
    qkv[cu[2]:cu[3], :D] *= 4.0
    qkv_t = torch.from_numpy(qkv).cuda().to(TD[dt]).contiguous()
    dO = g.standard_normal((rows, D), dtype=np.float32)
    heads = lambda a, b: a[cu[b]:cu[b + 1]].reshape(lens[b], H, DH).transpose(1, 0, 2)
    qkv64 = qkv_t.double().cpu().numpy()
    per_seq = [tuple(heads(qkv64[:, i * D:(i + 1) * D], b) for i in range(3)) + (heads(dO.astype(np.float64), b),) for b in range(len(lens))]
    return dict(lens=lens, cu=cu, rows=rows, qkv=qkv_t, cu_t=torch.from_numpy(cu).cuda(), dO=torch.from_numpy(dO).cuda(),
                dO0=torch.from_numpy(np.ascontiguousarray(dO[cu[:-1]])).cuda(), per_seq=per_seq)


@functools.lru_cache(maxsize=None)
def masks(max_len, p):
    """The library's own mask of the site, [nseq, H, 32, 32]: row = seq * n_head + head, col = query * 32 + key."""
    nseq = len(LENS[max_len])
    if p == 0:
        return None
    m = torch.empty(nseq * H, 1024, device="cuda")
    L.check(L.load().ofx_dropout_mask(p, SEED, SITE, nseq * H, 1024, m.data_ptr(), stream()), "ofx_dropout_mask")
    m = m.double().cpu().numpy().reshape(nseq, H, 32, 32)
    assert set(np.unique(m)) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}
    return m


@functools.lru_cache(maxsize=None)
def expected(max_len, dt, row0, p):
    """Per sequence: (ref, emul), each (O, dQ, dK, dV) as [H, S, 64] float64; under only_row0 dO is zero behind row 0."""
    inp, m = inputs(max_len, dt), masks(max_len, p)
    out = []
    for b, S in enumerate(inp["lens"]):
        q, k, v, dO = inp["per_seq"][b]
        if row0:
            dO = dO.copy(); dO[:, 1:] = 0.0
        mb = None if m is None else m[b, :, :S, :S]
        out.append((A.attn_train_ref(q, k, v, mb, dO, SCALE), A.attn_train_emul(q, k, v, mb, dO, SCALE, dt)))
    return out


@functools.lru_cache(maxsize=None)
def run(max_len, dt, row0, p, path):
    """One forward and one backward call of `path` -> per sequence (O, dQ, dK, dV) [H, S, 64] float64, after the buffer contracts
    (guard rows, poison, finiteness) are checked."""
    inp = inputs(max_len, dt)
    lens, cu, rows, nseq = inp["lens"], inp["cu"], inp["rows"], len(inp["lens"])
    lib = L.load()
    out, out_bits = poisoned(rows, D, dt)
    if path == "mfma":
        L.check(lib.ofx_attention_varlen(inp["qkv"].data_ptr(), out.data_ptr(), inp["cu_t"].data_ptr(), nseq, max_len, H, 3 * D, D, D, 2 * D,
                                         row0, SCALE, p, SEED, SITE, DT[dt], stream()), "ofx_attention_varlen")
    else:
        L.check(lib.ofx_set_attention_op(inp["qkv"].data_ptr(), out.data_ptr(), inp["cu_t"].data_ptr(), nseq, H, D, D, 1, max_len,
                                         row0, SCALE, p, SEED, SITE, DT[dt], stream()), "ofx_set_attention_op")
    dqkv, dq_bits = poisoned(rows, 3 * D, dt)
    d_o = inp["dO0"] if row0 else inp["dO"]
    L.check(lib.ofx_set_attention_bwd(inp["qkv"].data_ptr(), d_o.data_ptr(), dqkv.data_ptr(), inp["cu_t"].data_ptr(), nseq, H, D, max_len,
                                      row0, SCALE, p, SEED, SITE, 1 if path == "mfma" else 0, DT[dt], stream()), "ofx_set_attention_bwd")
    torch.cuda.synchronize()
    # ---- buffer contracts
    assert torch.equal(out.view(torch.int16)[rows:], out_bits[rows:]) and torch.equal(dqkv.view(torch.int16)[rows:], dq_bits[rows:]), "guard rows"
    written = torch.zeros(rows, dtype=torch.bool)
    written[torch.from_numpy(cu[:-1].astype(np.int64))] = True
    if not row0:
        written[:] = True
    o64, g64 = out[:rows].double().cpu(), dqkv[:rows].double().cpu()
    assert torch.isfinite(o64[written]).all() and torch.isfinite(g64).all()
    assert torch.equal(out.view(torch.int16)[:rows].cpu()[~written], out_bits[:rows].cpu()[~written]), "only_row0: the other rows are not stored"
    o64, g64 = o64.numpy(), g64.numpy()
    res = []
    for b, S in enumerate(lens):
        heads = lambda a: a[cu[b]:cu[b + 1]].reshape(S, H, DH).transpose(1, 0, 2)
        dQ = heads(g64[:, :D])
        if row0:
            assert not dQ[:, 1:].any(), "only_row0: dQ rows > 0 are exactly zero"
        res.append((heads(o64), dQ, heads(g64[:, D:2 * D]), heads(g64[:, 2 * D:])))
    return res


def blocks(max_len, dt, row0, p, path):
    """-> per tensor name: (e_kernel, yardstick = max(e_emul, 1e-2 u), ref_is_zero, got_is_zero), arrays over [nseq, H]."""
    got, exp = run(max_len, dt, row0, p, path), expected(max_len, dt, row0, p)
    out = {}
    for i, name in enumerate(TENSORS):
        nq = (lambda a: a[:, :1]) if (row0 and name == "O") else (lambda a: a)      # only_row0 forward: row 0 is all there is
        ek = np.stack([A.block_err(nq(g[i]), nq(e[0][i])) for g, e in zip(got, exp)])
        ee = np.stack([A.block_err(nq(e[1][i]), nq(e[0][i])) for e in exp])
        rz = np.stack([~nq(e[0][i]).any((-1, -2)) for e in exp])
        gz = np.stack([~nq(g[i]).any((-1, -2)) for g in got])
        out[name] = (ek, np.maximum(ee, 1e-2 * U[dt]), rz, gz)
    return out


CASES = [(ml, dt, row0, p) for ml in (8, 16, 32) for dt in ("bf16", "f16") for row0 in (0, 1) for p in (0.0, 0.3)]


@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("max_len,dt,row0,p", CASES)
def test_training_attention_kernels_per_block(max_len, dt, row0, p, path):
    bl = blocks(max_len, dt, row0, p, path)
    lens = LENS[max_len]
    bad = []
    for name, (ek, yard, ref_zero, got_zero) in bl.items():
        live = ~ref_zero
        print(f"RATIO {path} {dt} {name} max_len={max_len} row0={row0} p={p} worst={np.max(ek[live] / yard[live], initial=0.0):.3f}")
        expect_zero = np.zeros_like(ref_zero)
        if name in ("dQ", "dK"):
            expect_zero[[b for b, S in enumerate(lens) if S == 1]] = True             # one key: a constant softmax
        # ... and with dropout whatever else the mask empties: O and dV at S = 1 when its one probability is dropped
        assert np.array_equal(ref_zero, expect_zero) if p == 0 else ref_zero[expect_zero].all(), name
        assert got_zero[ref_zero].all(), (name, "a block whose reference is zero must be exactly zero")
        for b, h in zip(*np.nonzero(live & ~(ek <= F[path] * yard))):
            bad.append((name, f"seq {b} (S={lens[b]}) head {h}", float(ek[b, h]), float(yard[b, h])))
    assert not bad, bad


@pytest.mark.parametrize("max_len,dt,row0,p", CASES)
def test_mfma_and_valu_paths_agree_per_block(max_len, dt, row0, p):
    """The two paths on identical inputs: per block ||mfma - valu|| <= (F_mfma + F_valu) x the yardstick, times ||ref||."""
    gm, gv, exp = run(max_len, dt, row0, p, "mfma"), run(max_len, dt, row0, p, "valu"), expected(max_len, dt, row0, p)
    yard = blocks(max_len, dt, row0, p, "mfma")
    bad = []
    for i, name in enumerate(TENSORS):
        nq = (lambda a: a[:, :1]) if (row0 and name == "O") else (lambda a: a)
        for b, (m_, v_, e_) in enumerate(zip(gm, gv, exp)):
            diff = np.sqrt(((nq(m_[i]) - nq(v_[i])) ** 2).sum((-1, -2)))
            bound = (F["mfma"] + F["valu"]) * yard[name][1][b] * np.sqrt((nq(e_[0][i]) ** 2).sum((-1, -2)))
            for h in np.nonzero(~(diff <= bound))[0]:
                bad.append((name, b, int(h), float(diff[h]), float(bound[h])))
    assert not bad, bad


def test_rejected_calls_launch_nothing():
    """NULL pointers, nseq <= 0 and dropout_p outside [0, 1) are OFX_EINVAL, dropout beyond 32 rows per sequence (mask columns are keyed
    query * 32 + key) and a backward beyond 32 rows OFX_ESHAPE - at all three entry points; the poisoned outputs keep their bits."""
    inp = inputs(16, "bf16")
    rows, nseq = inp["rows"], len(inp["lens"])
    lib = L.load()
    q, c, g = inp["qkv"].data_ptr(), inp["cu_t"].data_ptr(), inp["dO"].data_ptr()
    out, out_bits = poisoned(rows, D, "bf16")
    dqkv, dq_bits = poisoned(rows, 3 * D, "bf16")
    o, d = out.data_ptr(), dqkv.data_ptr()

    def fwd_m(qkv=q, out_=o, cu=c, n=nseq, ml=16, p=0.0):
        return lib.ofx_attention_varlen(qkv, out_, cu, n, ml, H, 3 * D, D, D, 2 * D, 0, SCALE, p, SEED, SITE, 1, stream())

    def fwd_v(qkv=q, out_=o, cu=c, n=nseq, ml=16, p=0.0):
        return lib.ofx_set_attention_op(qkv, out_, cu, n, H, D, D, 1, ml, 0, SCALE, p, SEED, SITE, 1, stream())

    def bwd(mfma, qkv=q, d_o=g, dq=d, cu=c, n=nseq, ml=16, p=0.0):
        return lib.ofx_set_attention_bwd(qkv, d_o, dq, cu, n, H, D, ml, 0, SCALE, p, SEED, SITE, mfma, 1, stream())

    calls = [fwd_m, fwd_v, functools.partial(bwd, 1), functools.partial(bwd, 0)]
    for f in calls:
        for kw in (dict(qkv=None), dict(cu=None), dict(n=0), dict(n=-3), dict(p=1.0), dict(p=-0.25), dict(p=float("nan")), dict(p=1.5)):
            assert f(**kw) == OFX_EINVAL, (f, kw)
            assert b"bad argument" in lib.ofx_last_error()
        assert f(ml=33, p=0.3) == OFX_ESHAPE, f
        assert f(ml=0) == OFX_ESHAPE, f
    assert fwd_m(out_=None) == OFX_EINVAL and fwd_v(out_=None) == OFX_EINVAL
    for mfma in (0, 1):
        assert bwd(mfma, d_o=None) == OFX_EINVAL and bwd(mfma, dq=None) == OFX_EINVAL
        assert bwd(mfma, ml=33) == OFX_ESHAPE
    assert fwd_m(ml=64, p=0.3) == OFX_ESHAPE and b"query * 32 + key" in lib.ofx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), out_bits) and torch.equal(dqkv.view(torch.int16), dq_bits)
