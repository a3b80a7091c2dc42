"""Op-level float64 tests of attention_mfma_long_kernel - the MFMA attention over 65 .. 256 rows (ViT-B/16: 197) - on a real MI355X,
through ofx_attention_ex.  Cases: tests/attn_long_cases.py (pinned and shown sharp on the CPU by tests/test_cpu_attention_long.py);
helpers, buffer contract and criterion: tests/test_gpu_attention_fwd.py, unchanged -

  every output buffer NaN-poisoned with two guard rows behind it; guards and every not-to-be-written element (pad columns, rows behind
  row 0 under only_row0) bit-equal after the call, every written element finite; both operand types; accuracy per (sequence, head) block:
      e_kernel <= 1.6 max(e_emul, 1e-2 u),  emul = oracle/attn_fwd.attn_fwd_emul (P rounded to the operand type, the output rounded once)
  padded rows (ld + 8, NaN in the pad) bit-equal to packed rows; only_row0 rows bit-equal to the full call's; split3 rows: copies 0 and 2
  equal, copy 0 bit-equal to the plain call, hi + lo judged against the split3 emulation; fully masked query rows exactly zero in every
  copy; refusals (S = 257, varlen at max_len 65, mask_ld < seq_len) launch nothing; S = 64 and S = 50 through the same entry point keep
  the single-tile kernel's bits.

The three kernel instances: 8 key tiles (S <= 128: 65, 80, 81, 128), 13 (S <= 208: 129, 196, 197), 16 (241, 256).

MEASURED (MI355X), worst e_kernel / max(e_emul, 1e-2 u) over the packed rows and the split3 rows, per mask family and instance 8 | 13 | 16
key tiles:
    bf16: none 1.002 1.000 1.001   causal 1.000 1.000 1.000   tail 1.000 1.000 1.000   holes 1.000 1.000 1.000   causal+holes 1.000 1.000 1.001
    f16:  none 1.001 1.001 1.001   causal 1.002 1.001 1.001   tail 1.001 1.001 1.001   holes 1.001 1.002 1.001   causal+holes 1.000 1.000 1.000
  the kernel lands on its emulation as the single-tile kernel does (fp32 accumulation and the hardware exp2 are all that is left): worst
  1.002 against the factor 1.6; fully masked rows: worst 1.007 (f16, key0, S = 65); S = 50 / 64 through ofx_attention_ex: bit-equal to
  ofx_attention, worst 1.010.  All 63 cases run in 4.5 s.
"""
import functools

import numpy as np
import pytest
import torch

import attn_long_cases as C
from oracle import attn_fwd as A
from test_gpu_attention_fwd import cols_written, dev_mask, judge, poisoned, ptr, settle, split3_sum, stream

pytestmark = pytest.mark.gpu

OFX_ESHAPE = -2
H, W, NSEQ, SCALE, MASK_LD = C.H, C.W, C.NSEQ, C.SCALE, C.MASK_LD
DT = {"bf16": 1, "f16": 2}
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
F_OP, U = C.F_OP, C.U

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


def tiles_of(S):
    return 8 if S <= 128 else 13 if S <= 208 else 16


@functools.lru_cache(maxsize=None)
def inputs(S, dt):
    """q | k | v rounded to the operand type: packed [rows, 3 W] and padded [rows, 3 W + 8] (NaN in the pad) device rows, float64 heads."""
    rows = NSEQ * S
    packed = torch.from_numpy(C.qkv(S)).cuda().to(TD[dt]).contiguous()
    padded = torch.full((rows, 3 * W + 8), float("nan"), dtype=TD[dt], device="cuda")
    padded[:, :3 * W] = packed
    q64 = packed.double().cpu().numpy()
    return packed, padded, tuple(A.heads(q64[:, i * W:(i + 1) * W], S) for i in range(3))


def call(S, dt, mask_t, causal, padded, row0, split3, mask_ld=MASK_LD):
    """One ofx_attention_ex call -> the output rows (float64 numpy [rows, ldo]) after the buffer contract is checked."""
    pk, pd, _ = inputs(S, dt)
    rows = NSEQ * S
    qkv, ld = (pd, 3 * W + 8) if padded else (pk, 3 * W)
    ncol = 3 * W if split3 else W
    ldo = ncol + (8 if padded else 0)
    out, before = poisoned(rows, ldo, TD[dt])
    L.check(L.load().ofx_attention_ex(qkv.data_ptr(), out.data_ptr(), ptr(mask_t), NSEQ, S, H, ld, ldo, W, 2 * W, mask_ld, causal, row0,
                                      W if split3 else 0, SCALE, DT[dt], stream()), "ofx_attention_ex")
    return settle(out, before, cols_written(rows, ldo, ncol, np.arange(NSEQ) * S if row0 else None))


@pytest.mark.parametrize("S,family", C.CASES)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_long_fixed_length_per_block(dt, S, family):
    mask, causal = C.key_mask(family, S)
    mask_t = dev_mask(mask)
    q, k, v = inputs(S, dt)[2]
    dead = A.dead_of(mask, causal, S)
    ref = A.attn_fwd_ref(q, k, v, dead, SCALE)
    emul, emul3 = (A.attn_fwd_emul(q, k, v, dead, SCALE, dt, split3=s3) for s3 in (False, True))
    floor = 1e-2 * U[dt]
    plain = call(S, dt, mask_t, causal, False, 0, False)
    worst = judge(A.heads(plain, S), ref, emul, floor, F_OP, "packed")
    padded = call(S, dt, mask_t, causal, True, 0, False)
    assert np.array_equal(padded[:, :W], plain), "padded rows: other bits than packed rows"
    first = np.arange(NSEQ) * S
    row0 = call(S, dt, mask_t, causal, False, 1, False)
    assert np.array_equal(row0[first], plain[first]), "only_row0: row b S differs from the full call's"
    for pad in (False, True):
        s3 = call(S, dt, mask_t, causal, pad, 0, True)
        assert np.array_equal(s3[:, :W], plain), "split3 copy 0 differs from the plain call"
        worst = max(worst, judge(A.heads(split3_sum(s3, W, "split3"), S), ref, emul3, floor, F_OP, f"split3 pad={pad}"))
    s3r = call(S, dt, mask_t, causal, True, 1, True)
    assert np.array_equal(s3r[first, :3 * W], s3[first, :3 * W]), "only_row0 with split3 rows"
    print(f"RATIO L mfma-long {dt} {family} KT={tiles_of(S)} S={S} worst={worst:.3f}")


@pytest.mark.parametrize("case", ["key0", "allzero"])
@pytest.mark.parametrize("S", [65, 197])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fully_masked_rows_are_zero(dt, S, case):
    mask, causal = next((m, c) for n, m, c in C.masked_row_cases(S) if n == case)
    mask_t = dev_mask(mask)
    q, k, v = inputs(S, dt)[2]
    dead = np.broadcast_to(A.dead_of(mask, causal, S), (NSEQ, H, S, S))
    full = dead.all(-1)
    assert full.any()
    ref = A.attn_fwd_ref(q, k, v, dead, SCALE)
    plain = call(S, dt, mask_t, causal, False, 0, False)              # settle: every written element finite
    got = A.heads(plain, S)
    assert not got[full].any(), "a fully masked query row must be exactly zero"
    worst = judge(got, ref, A.attn_fwd_emul(q, k, v, dead, SCALE, dt), 1e-2 * U[dt], F_OP, "plain")
    s3 = call(S, dt, mask_t, causal, True, 0, True)
    for c in range(3):
        assert not A.heads(s3[:, c * W:(c + 1) * W], S)[full].any(), f"split3 copy {c} of a fully masked row must be exactly zero"
    assert np.array_equal(s3[:, :W], plain)
    worst = max(worst, judge(A.heads(split3_sum(s3, W, "split3"), S), ref, A.attn_fwd_emul(q, k, v, dead, SCALE, dt, split3=True), 1e-2 * U[dt], F_OP,
                             "split3"))
    r0 = call(S, dt, mask_t, causal, False, 1, False)
    assert np.array_equal(r0[np.arange(NSEQ) * S], plain[np.arange(NSEQ) * S])
    print(f"RATIO L mfma-long masked-rows {dt} {case} S={S} worst={worst:.3f}")


def test_refusals_launch_nothing():
    lib = L.load()
    S = 257
    rows = NSEQ * S
    qkv = torch.zeros(rows, 3 * W, dtype=torch.bfloat16, device="cuda")
    mask_t = torch.ones(NSEQ, MASK_LD, dtype=torch.int64, device="cuda")
    out, before = poisoned(rows, W, torch.bfloat16)
    st = stream()
    assert lib.ofx_attention_ex(qkv.data_ptr(), out.data_ptr(), None, NSEQ, 257, H, 3 * W, W, W, 2 * W, 0, 0, 0, 0, SCALE, 1, st) == OFX_ESHAPE
    assert b"[1,256]" in lib.ofx_last_error()
    assert lib.ofx_attention(qkv.data_ptr(), out.data_ptr(), None, NSEQ, 257, H, 3 * W, W, W, 2 * W, 0, 0, SCALE, 1, st) == OFX_ESHAPE
    # a key mask narrower than the sequence
    assert lib.ofx_attention_ex(qkv.data_ptr(), out.data_ptr(), mask_t.data_ptr(), NSEQ, 197, H, 3 * W, W, W, 2 * W, 196, 0, 0, 0, SCALE, 1, st) == OFX_ESHAPE
    # varlen mode stays single-tile: max_len 65 is refused, 64 is not (7 sequences of 64 rows)
    cu = torch.arange(NSEQ + 1, dtype=torch.int32, device="cuda") * 64
    assert lib.ofx_attention_varlen(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), NSEQ, 65, H, 3 * W, W, W, 2 * W, 0, SCALE, 0.0, 0, 0, 1, st) == OFX_ESHAPE
    assert b"varlen" in lib.ofx_last_error()
    settle(out, before, np.zeros((rows, W), bool))
    assert lib.ofx_attention_varlen(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), NSEQ, 64, H, 3 * W, W, W, 2 * W, 0, SCALE, 0.0, 0, 0, 1, st) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [50, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_up_to_64_rows_keep_the_single_tile_kernel(dt, S):
    """seq_len <= 64 through ofx_attention_ex is attention_mfma_kernel's result, bit for bit: against ofx_attention - the single-tile
    instance's own entry point - and against that kernel's criterion."""
    lib = L.load()
    rows = NSEQ * S
    mask, causal = A.key_mask("holes", S)
    mask_t = dev_mask(mask)
    packed = torch.from_numpy(A.fixed_qkv(S)).cuda().to(TD[dt]).contiguous()
    q64 = packed.double().cpu().numpy()
    q, k, v = (A.heads(q64[:, i * W:(i + 1) * W], S) for i in range(3))
    outs = []
    for ex in (False, True):
        out, before = poisoned(rows, W, TD[dt])
        if ex:
            rc = lib.ofx_attention_ex(packed.data_ptr(), out.data_ptr(), mask_t.data_ptr(), NSEQ, S, H, 3 * W, W, W, 2 * W, A.MASK_LD, causal, 0, 0, SCALE, DT[dt], stream())
        else:
            rc = lib.ofx_attention(packed.data_ptr(), out.data_ptr(), mask_t.data_ptr(), NSEQ, S, H, 3 * W, W, W, 2 * W, A.MASK_LD, causal, SCALE, DT[dt], stream())
        L.check(rc, "ofx_attention")
        outs.append(settle(out, before, np.ones((rows, W), bool)))
    assert np.array_equal(outs[0], outs[1])
    dead = A.dead_of(mask, causal, S)
    worst = judge(A.heads(outs[0], S), A.attn_fwd_ref(q, k, v, dead, SCALE), A.attn_fwd_emul(q, k, v, dead, SCALE, dt), 1e-2 * U[dt], F_OP, "single tile")
    print(f"RATIO L mfma single-tile {dt} S={S} worst={worst:.3f}")
