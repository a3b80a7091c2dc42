"""Op-level float64 tests of the scoring path's attention kernels and of the split-K consumers on a real MI355X, through the C ABI:

  A  attention_mfma_kernel, fixed length (ofx_attention_ex): every 16-row tile edge of NT = 1, 2, 4, five mask families, packed and
     padded rows, only_row0, split3 rows
  B  fully masked query rows, both kernels (ofx_attention_ex, ofx_attention_f32): exactly zero, the library's stated rule
  C  attention_mfma_kernel, varlen beyond 32 rows (ofx_attention_varlen at max_len 48 / 64), and set_attention_kernel<T, 64, T>
     (ofx_set_attention_op at max_len 64)
  D  set_attention_kernel<T, SMAX, float>, all four SMAX instances (ofx_set_attention), and its fixed-length masked mode (ofx_attention_f32)
  E  the split-K consumers: set_attention_kernel reading slabs (ofx_set_attention_slabs) and splitk_reduce_ln_kernel (ofx_splitk_reduce_ln),
     exact where the code promises exactness

References: oracle/attn_fwd.py and oracle/splitk_ops.py (plain numpy, pinned on the CPU by tests/test_cpu_attn_fwd_ref.py).  Method of
tests/test_gpu_attention_train.py: n_head = 3 and 7 sequences (21 (sequence, head) pairs: the last MFMA block has one live wave and three
dead ones), sequence 2 with q x 4 (a peaked softmax), both operand types; every output buffer NaN-poisoned with two guard rows of a fixed
bit pattern behind it, guards and every not-to-be-written element (pad columns, rows behind row 0 under only_row0, rows past a live
count) compared bit for bit after the call, every written element finite.  Accuracy is judged PER BLOCK - one (sequence, head), S x 64
values, relative to ||ref|| - so that one wrong head, tile or short sequence cannot hide behind the largest element of the tensor.

Criteria (u = 2^-8 bf16 | 2^-11 f16):
  MFMA kernel, and every operand-type output:   e_kernel <= 1.6 max(e_emul, 1e-2 u), emul = the float64 computation with the kernel's stated
      roundings (attn_fwd_emul; for the fp32 kernel with P unrounded).  1.6 is what the project holds the same wave core to in its varlen
      training mode (tests/test_gpu_attention_train.py F["mfma"]).
  fp32 kernel, fp32 output:   e_kernel <= 2 max(e over the float32 yardstick orders, 2^-26): the formula restated in np.float32 in five
      summation orders, none of them the kernel's.  The CPU test shows a held-out sixth order - the kernel's blocks of four - inside
      1.25 x that envelope on these very inputs (worst 1.04); the rest of the factor 2 is the device expf and fma contraction.  At S = 1,
      P = 1 and the output is v bit for bit.
  split3 rows: copies 0 and 2 bit-equal, copy 0 bit-equal to the plain call, hi + lo judged against the split3 emulation.
  E: bit for bit against numpy float32 in the stated order (slabs ascending, bias, residual); the LayerNorm against float64 of the x the
      kernel wrote, per element, inside oracle/splitk_ops.ln_bound - derived there from the row's float64 magnitudes for ANY two-pass fp32
      LayerNorm (mean: (D + 2) u32 mean|x|; variance: (D + 6) u32 and the squared mean error; rsqrt; the affine map; the output
      rounding), checked on the CPU against a float32 numpy LayerNorm, never tuned on the kernel.  ofx_layernorm on the same x agrees to
      twice that fp32 bound - NOT bit for bit, as csrc/norm_act.hip says: its sums take another order.

MEASURED (MI355X), worst ratio to the yardstick:
  A  MFMA fixed length, worst e_kernel / max(e_emul, 1e-2 u) over S, both layouts and the split3 rows, per mask family and NT = 1 | 2 | 4:
         bf16: none 1.000 1.000 1.001   causal 1.000 1.000 1.000   tail 1.000 1.000 1.002   holes 1.000 1.000 1.000   causal+holes 1.000 1.000 1.000
         f16:  none 1.000 1.005 1.002   causal 1.005 1.016 1.002   tail 1.000 1.004 1.004   holes 1.000 1.001 1.010   causal+holes 1.005 1.001 1.003
     the kernel lands on its emulation (fp32 accumulation and the hardware exp2 are all that is left), worst 1.016 against the factor 1.6.
  C  MFMA varlen at max_len 48 / 64, with and without only_row0: bf16 1.000, f16 1.003; set_attention_kernel<T, 64, T>: 1.000 both types.
  D  fp32 kernel, fp32 output, worst e_kernel / max(e over the float32 orders, 2^-26) per SMAX 8 | 20 | 32 | 64:
         varlen sets (ofx_set_attention)          1.190  0.829  0.961  1.125
         fixed length, masks (ofx_attention_f32)  0.938  0.972  1.055  0.818
     nothing above the factor 2, so nothing to explain; operand-type output 1.000, split3 rows 0.07 - 0.08 of the floor 1e-2 u.
  E  slab input and x: bit for bit in all 72 + 216 calls.  LayerNorm worst err / bound 0.989 (bf16) and 0.946 (f16) - the output rounding
     at its sharp worst case u |y|; the fp32 part alone (out_kind 0) reads at most 0.0067 of its worst-case bound, and ofx_layernorm on the same x differs
     from the fused kernel by at most 0.0093 of that bound, never bit-equal over a whole tensor.

FINDING, fixed in csrc/attn_wave.h (attn_softmax_p): a fully masked query row came out of the MFMA kernel as NaN, not as the zeros its
comment promises - every e is 0, the sum is 0, and 0 * v_rcp_f32(0) = 0 * inf.  The normalisation is now 0 for a zero sum, as in the
fp32 kernel; every other row keeps its bits (the bit-identity tests of the fused, indexed, graph and persistent paths pass unchanged).
Measured before the fix through ofx_attention: all-NaN on every fully masked row (S = 1, 17, 50, both masks, both types), no NaN elsewhere.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import attn_fwd as A
from oracle import splitk_ops as K

pytestmark = pytest.mark.gpu

OFX_EINVAL, OFX_ESHAPE = -1, -2
H, DH, W, NSEQ, SCALE, MASK_LD = A.H, A.DH, A.W, A.NSEQ, A.SCALE, A.MASK_LD
DT = {"bf16": 1, "f16": 2}
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
F_OP, F_F32, FLOOR_F32 = 1.6, 2.0, 2.0 ** -26
GUARD = 0x5AA5
EPS = 1e-5

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


def poisoned(rows, cols, td, fill=None):
    """[rows + 2, cols] of NaN (or `fill` [rows, cols]) followed by two guard rows of GUARD bits -> the buffer and a copy of its bits."""
    buf = torch.full((rows + 2, cols), float("nan"), dtype=td, device="cuda")
    if fill is not None:
        buf[:rows] = fill
    bits(buf)[rows:].fill_(GUARD if buf.element_size() == 2 else (GUARD << 16 | GUARD))
    return buf, bits(buf).clone()


def settle(buf, before, written):
    """After the call: the guard rows and every element outside `written` (bool [rows, cols], numpy) keep their bits, every written element
    is finite -> the rows as float64 numpy."""
    torch.cuda.synchronize()
    rows = written.shape[0]
    now = bits(buf)
    assert torch.equal(now[rows:], before[rows:]), "guard rows"
    same = (now[:rows] == before[:rows]).cpu().numpy()
    assert same[~written].all(), "an element that must not be written changed"
    vals = buf[:rows].double().cpu().numpy()
    assert np.isfinite(vals[written]).all(), "a written element is not finite"
    return vals


def cols_written(rows, cols, n_cols, row_sel=None):
    w = np.zeros((rows, cols), bool)
    w[:, :n_cols] = True
    if row_sel is not None:
        keep = np.zeros(rows, bool)
        keep[row_sel] = True
        w[~keep] = False
    return w


def dev_mask(mask):
    return None if mask is None else torch.from_numpy(mask).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def judge(got, ref, yard_src, floor, factor, label):
    """Per block: ||got - ref|| <= factor max(||yard_src - ref||, floor ||ref||) -> the worst ratio.  yard_src: one emulation or a list."""
    ek = A.block_err(got, ref)
    srcs = yard_src if isinstance(yard_src, (list, tuple)) else [yard_src]
    yard = np.maximum(np.max([A.block_err(s, ref) for s in srcs], axis=0), floor)
    live = np.asarray(ref).any((-1, -2))
    assert not np.asarray(got)[~live].any(), (label, "a block whose reference is zero must be exactly zero")
    ratio = np.where(live, ek / yard, 0.0)
    bad = [(tuple(int(i) for i in idx), float(ek[idx]), float(yard[idx])) for idx in zip(*np.nonzero(~(ratio <= factor)))]
    assert not bad, (label, bad)
    return float(ratio.max(initial=0.0))


def split3_sum(vals, w, label):
    """[rows, >= 3 w] of [hi | lo | hi] -> hi + lo, after copies 0 and 2 are found equal value for value and sign for sign (rows that were not
    written hold the same poison in both)."""
    hi, lo, hi2 = vals[:, :w], vals[:, w:2 * w], vals[:, 2 * w:3 * w]
    assert np.array_equal(hi, hi2, equal_nan=True) and np.array_equal(np.signbit(hi), np.signbit(hi2)), (label, "split3 copies 0 and 2 differ")
    return hi + lo


def nt_of(S):
    return 1 if S <= 16 else 2 if S <= 32 else 4


# ------------------------------------------------------------------------------------------------ A, B: MFMA, fixed length
@functools.lru_cache(maxsize=None)
def mfma_inputs(S, dt):
    """q | k | v rounded to the operand type: packed [rows, 3 W] and padded [rows, 3 W + 8] (NaN in the pad) device rows, float64 heads."""
    rows = NSEQ * S
    packed = torch.from_numpy(A.fixed_qkv(S)).cuda().to(TD[dt]).contiguous()
    padded = torch.full((rows, 3 * W + 8), float("nan"), dtype=TD[dt], device="cuda")
    padded[:, :3 * W] = packed
    q64 = packed.double().cpu().numpy()
    return packed, padded, tuple(A.heads(q64[:, i * W:(i + 1) * W], S) for i in range(3))


def call_mfma(S, dt, mask_t, causal, padded, row0, split3):
    """One ofx_attention_ex call -> the output rows (float64 numpy [rows, ldo]) after the buffer contract is checked."""
    pk, pd, _ = mfma_inputs(S, dt)
    rows = NSEQ * S
    qkv, ld = (pd, 3 * W + 8) if padded else (pk, 3 * W)
    ncol = 3 * W if split3 else W
    ldo = ncol + (8 if padded else 0)
    out, before = poisoned(rows, ldo, TD[dt])
    L.check(L.load().ofx_attention_ex(qkv.data_ptr(), out.data_ptr(), ptr(mask_t), NSEQ, S, H, ld, ldo, W, 2 * W, MASK_LD, causal, row0,
                                      W if split3 else 0, SCALE, DT[dt], stream()), "ofx_attention_ex")
    return settle(out, before, cols_written(rows, ldo, ncol, np.arange(NSEQ) * S if row0 else None))


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("S", A.FIXED_S_MFMA)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_mfma_fixed_length_per_block(dt, S, family):
    mask, causal = A.key_mask(family, S)
    mask_t = dev_mask(mask)
    q, k, v = mfma_inputs(S, dt)[2]
    dead = A.dead_of(mask, causal, S)
    ref = A.attn_fwd_ref(q, k, v, dead, SCALE)
    emul, emul3 = (A.attn_fwd_emul(q, k, v, dead, SCALE, dt, split3=s3) for s3 in (False, True))
    floor = 1e-2 * U[dt]
    plain = call_mfma(S, dt, mask_t, causal, False, 0, False)
    worst = judge(A.heads(plain, S), ref, emul, floor, F_OP, "packed")
    padded = call_mfma(S, dt, mask_t, causal, True, 0, False)
    assert np.array_equal(padded[:, :W], plain), "padded rows: other bits than packed rows"
    first = np.arange(NSEQ) * S
    row0 = call_mfma(S, dt, mask_t, causal, False, 1, False)
    assert np.array_equal(row0[first], plain[first]), "only_row0: row b S differs from the full call's"
    for pad in (False, True):
        s3 = call_mfma(S, dt, mask_t, causal, pad, 0, True)
        assert np.array_equal(s3[:, :W], plain), "split3 copy 0 differs from the plain call"
        worst = max(worst, judge(A.heads(split3_sum(s3, W, "split3"), S), ref, emul3, floor, F_OP, f"split3 pad={pad}"))
    s3r = call_mfma(S, dt, mask_t, causal, True, 1, True)
    assert np.array_equal(s3r[first, :3 * W], s3[first, :3 * W]), "only_row0 with split3 rows"
    print(f"RATIO A mfma {dt} {family} NT={nt_of(S)} S={S} worst={worst:.3f}")


@pytest.mark.parametrize("case", ["key0", "allzero"])
@pytest.mark.parametrize("S", [1, 2, 17, 50])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fully_masked_rows_are_zero_mfma(dt, S, case):
    mask, causal = next((m, c) for n, m, c in A.masked_row_cases(S) if n == case)
    mask_t = dev_mask(mask)
    q, k, v = mfma_inputs(S, dt)[2]
    dead = np.broadcast_to(A.dead_of(mask, causal, S), (NSEQ, H, S, S))
    full = dead.all(-1)
    assert full.any()
    ref = A.attn_fwd_ref(q, k, v, dead, SCALE)
    plain = call_mfma(S, dt, mask_t, causal, False, 0, False)           # settle: every written element finite
    got = A.heads(plain, S)
    assert not got[full].any(), "a fully masked query row must be exactly zero"
    judge(got, ref, A.attn_fwd_emul(q, k, v, dead, SCALE, dt), 1e-2 * U[dt], F_OP, "plain")
    s3 = call_mfma(S, dt, mask_t, causal, True, 0, True)
    for c in range(3):
        assert not A.heads(s3[:, c * W:(c + 1) * W], S)[full].any(), f"split3 copy {c} of a fully masked row must be exactly zero"
    assert np.array_equal(s3[:, :W], plain)
    judge(A.heads(split3_sum(s3, W, "split3"), S), ref, A.attn_fwd_emul(q, k, v, dead, SCALE, dt, split3=True), 1e-2 * U[dt], F_OP, "split3")
    r0 = call_mfma(S, dt, mask_t, causal, False, 1, False)
    assert np.array_equal(r0[np.arange(NSEQ) * S], plain[np.arange(NSEQ) * S])


# ------------------------------------------------------------------------------------------------ C: varlen beyond 32 rows
@functools.lru_cache(maxsize=None)
def varlen_inputs(max_len, dt):
    lens = [min(n, max_len) for n in A.VARLEN_LENS]
    cu, qkv = A.varlen_qkv(lens)
    qkv_t = torch.from_numpy(qkv).cuda().to(TD[dt]).contiguous()
    q64 = qkv_t.double().cpu().numpy()
    per_seq = [tuple(A.seq_heads(q64[cu[b]:cu[b + 1], i * W:(i + 1) * W], S) for i in range(3)) for b, S in enumerate(lens)]
    return lens, cu, qkv_t, torch.from_numpy(cu).cuda(), per_seq


def judge_varlen(vals, lens, cu, per_seq, row0, dt, round_p, label):
    worst = 0.0
    for b, S in enumerate(lens):
        q, k, v = per_seq[b]
        nq = 1 if row0 else S
        ref = A.attn_fwd_ref(q, k, v, None, SCALE)[:, :nq]
        emul = A.attn_fwd_emul(q, k, v, None, SCALE, dt, round_p=round_p)[:, :nq]
        got = A.seq_heads(vals[cu[b]:cu[b + 1], :W], S)[:, :nq]
        worst = max(worst, judge(got, ref, emul, 1e-2 * U[dt], F_OP, f"{label} seq {b} S={S}"))
    return worst


@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("max_len", [48, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_mfma_varlen_beyond_32_rows(dt, max_len, row0):
    lens, cu, qkv_t, cu_t, per_seq = varlen_inputs(max_len, dt)
    rows = int(cu[-1])
    out, before = poisoned(rows, W + 8, TD[dt])
    L.check(L.load().ofx_attention_varlen(qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, max_len, H, 3 * W, W + 8, W, 2 * W, row0, SCALE,
                                          0.0, 0, 0, DT[dt], stream()), "ofx_attention_varlen")
    vals = settle(out, before, cols_written(rows, W + 8, W, cu[:-1] if row0 else None))
    worst = judge_varlen(vals, lens, cu, per_seq, row0, dt, True, "varlen")
    print(f"RATIO C mfma-varlen {dt} max_len={max_len} row0={row0} worst={worst:.3f}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_valu_operand_type_input_at_64_rows(dt):
    """set_attention_kernel<T, 64, T>: operand-type q | k | v, fp32 P, the output rounded once."""
    lens, cu, qkv_t, cu_t, per_seq = varlen_inputs(64, dt)
    rows = int(cu[-1])
    out, before = poisoned(rows, W + 8, TD[dt])
    L.check(L.load().ofx_set_attention_op(qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, H, W, W + 8, 1, 64, 0, SCALE, 0.0, 0, 0, DT[dt],
                                          stream()), "ofx_set_attention_op")
    vals = settle(out, before, cols_written(rows, W + 8, W))
    print(f"RATIO C valu-op {dt} max_len=64 worst={judge_varlen(vals, lens, cu, per_seq, 0, dt, False, 'set_attention_op'):.3f}")


# ------------------------------------------------------------------------------------------------ D: the fp32 VALU kernel
def f32_out(rows, kind, dt):
    """-> buffer, bits before, ldo, written columns: fp32 [W + 4] | operand type [W + 8] | [3 W + 8]."""
    ncol = 3 * W if kind == 2 else W
    ldo = ncol + (4 if kind == 0 else 8)
    buf, before = poisoned(rows, ldo, torch.float32 if kind == 0 else TD[dt])
    return buf, before, ldo, ncol


def judge_f32(vals, kind, dt, ref, orders, emul_of, to_blocks, label):
    """kind 0 against the float32 yardsticks; 1 and 2 against the emulation with only the output rounded."""
    if kind == 0:
        return judge(to_blocks(vals[:, :W]), ref, list(orders.values()), FLOOR_F32, F_F32, label)
    got = vals[:, :W] if kind == 1 else split3_sum(vals, W, label)
    return judge(to_blocks(got), ref, emul_of(kind == 2), 1e-2 * U[dt], F_OP, label)


@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("max_len", sorted(A.SET_LENS))
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_f32_set_attention_every_smax(dt, max_len, kind, row0):
    lens = A.SET_LENS[max_len]
    assert {1, max_len - 1, max_len} <= set(lens)
    cu, qkv = A.varlen_qkv(lens)
    rows = int(cu[-1])
    qkv_t, cu_t = torch.from_numpy(qkv).cuda(), torch.from_numpy(cu).cuda()
    out, before, ldo, ncol = f32_out(rows, kind, dt)
    L.check(L.load().ofx_set_attention(qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, H, W, ldo, kind, max_len, row0, SCALE, DT[dt],
                                       stream()), "ofx_set_attention")
    vals = settle(out, before, cols_written(rows, ldo, ncol, cu[:-1] if row0 else None))
    worst = 0.0
    for b, (S, (ref, orders)) in enumerate(zip(lens, A.f32_yardsticks_varlen(max_len))):
        nq = 1 if row0 else S
        sl = qkv[cu[b]:cu[b + 1]].astype(np.float64)
        q, k, v = (A.seq_heads(sl[:, i * W:(i + 1) * W], S) for i in range(3))
        emul_of = lambda s3: A.attn_fwd_emul(q, k, v, None, SCALE, dt, split3=s3, round_p=False)[:, :nq]
        blocks = lambda a: A.seq_heads(a[cu[b]:cu[b + 1]], S)[:, :nq]
        worst = max(worst, judge_f32(vals, kind, dt, ref[:, :nq], {o: a[:, :nq] for o, a in orders.items()}, emul_of, blocks, f"seq {b} S={S}"))
        if S == 1 and kind == 0:
            got32 = out[int(cu[b]), :W].cpu().numpy()
            assert np.array_equal(got32.view(np.int32), qkv[cu[b], 2 * W:].view(np.int32)), "S = 1: P = 1, the output is v bit for bit"
    print(f"RATIO D f32-set {dt} SMAX={max_len} kind={kind} row0={row0} worst={worst:.3f}")


def call_f32_fixed(S, dt, kind, mask_t, causal):
    rows = NSEQ * S
    qkv_t = torch.from_numpy(A.fixed_qkv(S)).cuda()
    out, before, ldo, ncol = f32_out(rows, kind, dt)
    L.check(L.load().ofx_attention_f32(qkv_t.data_ptr(), out.data_ptr(), ptr(mask_t), NSEQ, S, H, W, ldo, kind, MASK_LD, causal, SCALE, DT[dt],
                                       stream()), "ofx_attention_f32")
    return settle(out, before, cols_written(rows, ldo, ncol)), out


def f32_fixed_emul(S, dead, dt):
    qkv = A.fixed_qkv(S).astype(np.float64)
    q, k, v = (A.heads(qkv[:, i * W:(i + 1) * W], S) for i in range(3))
    return lambda s3: A.attn_fwd_emul(q, k, v, dead, SCALE, dt, split3=s3, round_p=False)


def smax_of(S):
    return 8 if S <= 8 else 20 if S <= 20 else 32 if S <= 32 else 64


@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("S", A.FIXED_S_F32)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_f32_fixed_length_masked_attention(dt, S, family):
    mask, causal = A.key_mask(family, S)
    mask_t = dev_mask(mask)
    ref, orders, dead = A.f32_yardsticks_fixed(S, family)
    emul_of = f32_fixed_emul(S, dead, dt)
    for kind in (0, 1, 2):
        vals, out = call_f32_fixed(S, dt, kind, mask_t, causal)
        worst = judge_f32(vals, kind, dt, ref, orders, emul_of, lambda a: A.heads(a, S), f"kind {kind}")
        if S == 1 and kind == 0:
            assert np.array_equal(out[:NSEQ, :W].contiguous().cpu().numpy().view(np.int32), np.ascontiguousarray(A.fixed_qkv(S)[:, 2 * W:]).view(np.int32)), "S = 1: the output is v"
        print(f"RATIO D f32-fixed {dt} SMAX={smax_of(S)} S={S} {family} kind={kind} worst={worst:.3f}")


@pytest.mark.parametrize("case", ["key0", "allzero"])
@pytest.mark.parametrize("S", [1, 2, 17, 50])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fully_masked_rows_are_zero_f32(dt, S, case):
    mask, causal = next((m, c) for n, m, c in A.masked_row_cases(S) if n == case)
    mask_t = dev_mask(mask)
    ref, orders, dead = A.f32_yardsticks_fixed(S, None, case)
    full = np.broadcast_to(dead, (NSEQ, H, S, S)).all(-1)
    assert full.any() and not ref[full].any()
    emul_of = f32_fixed_emul(S, dead, dt)
    for kind in (0, 1, 2):
        vals, _ = call_f32_fixed(S, dt, kind, mask_t, causal)
        for c in range(3 if kind == 2 else 1):
            assert not A.heads(vals[:, c * W:(c + 1) * W], S)[full].any(), f"kind {kind} copy {c}: a fully masked row must be exactly zero"
        judge_f32(vals, kind, dt, ref, orders, emul_of, lambda a: A.heads(a, S), f"kind {kind}")


# ------------------------------------------------------------------------------------------------ E: the split-K consumers
def slab_case(splits, max_len):
    lens = A.SET_LENS[max_len]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = int(cu[-1])
    g = np.random.default_rng(31 * splits + max_len)
    slabs = K.cancelling_slabs(g, splits, (rows, 3 * W), n_pairs=64)
    bias = (0.5 * g.standard_normal(3 * W)).astype(np.float32)
    return lens, cu, rows, slabs, bias


def slab_buffer(slabs, rows):
    """The slabs on the device with a gap of 64 floats between them (the plane stride is not the slab size) -> tensor, plane."""
    plane = rows * 3 * W + 64
    buf = torch.full((slabs.shape[0], plane), float("nan"), device="cuda")
    buf[:, :rows * 3 * W] = torch.from_numpy(slabs.reshape(slabs.shape[0], -1)).cuda()
    return buf, plane


@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("max_len", [8, 20, 32])
@pytest.mark.parametrize("splits", [2, 5, 16])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_set_attention_from_slabs_is_the_separate_pass_bit_for_bit(dt, splits, max_len, row0, kind):
    lens, cu, rows, slabs, bias = slab_case(splits, max_len)
    lib = L.load()
    cu_t, bias_t = torch.from_numpy(cu).cuda(), torch.from_numpy(bias).cuda()
    summed = torch.from_numpy(K.slab_sum(slabs, bias)).cuda()           # numpy float32, slabs ascending, then the bias

    def run(f):
        out, before, ldo, ncol = f32_out(rows, kind, dt)
        L.check(f(out.data_ptr(), ldo), "set attention")
        settle(out, before, cols_written(rows, ldo, ncol, cu[:-1] if row0 else None))
        return bits(out).cpu().numpy()

    want = run(lambda o, ldo: lib.ofx_set_attention(summed.data_ptr(), o, cu_t.data_ptr(), NSEQ, H, W, ldo, kind, max_len, row0, SCALE, DT[dt], stream()))
    buf, plane = slab_buffer(slabs, rows)
    slab_call = lambda b: (lambda o, ldo: lib.ofx_set_attention_slabs(b.data_ptr(), plane, splits, bias_t.data_ptr(), o, cu_t.data_ptr(), NSEQ, H, W, ldo,
                                                                     kind, max_len, row0, SCALE, DT[dt], stream()))
    assert np.array_equal(run(slab_call(buf)), want), "slab input: other bits than ofx_set_attention on the summed array"
    one = run(lambda o, ldo: lib.ofx_set_attention_slabs(summed.data_ptr(), 0, 1, None, o, cu_t.data_ptr(), NSEQ, H, W, ldo, kind, max_len, row0, SCALE,
                                                         DT[dt], stream()))
    assert np.array_equal(one, want), "splits = 1 is the plain fp32 path"
    if row0:                                                            # q of rows > 0 is never read: NaN there in every slab changes nothing
        nanq = slabs.copy()
        later = np.ones(rows, bool)
        later[cu[:-1]] = False
        nanq[:, later, :W] = np.nan
        assert np.array_equal(run(slab_call(slab_buffer(nanq, rows)[0])), want), "only_row0: q of a row > 0 was read"


def test_set_attention_slabs_refusals_launch_nothing():
    lens, cu, rows, slabs, bias = slab_case(2, 32)
    lib = L.load()
    cu_t, bias_t = torch.from_numpy(cu).cuda(), torch.from_numpy(bias).cuda()
    buf, plane = slab_buffer(slabs, rows)
    out, before, ldo, _ = f32_out(rows, 0, "bf16")

    def call(slab=buf.data_ptr(), plane_=plane, splits=2, b=bias_t.data_ptr(), o=out.data_ptr(), c=cu_t.data_ptr(), ml=32, n=NSEQ, kind=0, dt=1):
        return lib.ofx_set_attention_slabs(slab, plane_, splits, b, o, c, n, H, W, ldo, kind, ml, 0, SCALE, dt, stream())

    for kw in (dict(ml=33), dict(b=None), dict(plane_=0)):              # the launcher's own rules for slab input
        assert call(**kw) == OFX_EINVAL and b"slab input" in lib.ofx_last_error(), kw
    for kw in (dict(slab=None), dict(o=None), dict(c=None), dict(n=0), dict(splits=0), dict(dt=0), dict(plane_=plane + 2), dict(slab=buf.data_ptr() + 4)):
        assert call(**kw) == OFX_EINVAL, kw
    for kw in (dict(kind=3), dict(ml=65, splits=1), dict(ml=0)):
        assert call(**kw) == OFX_ESHAPE, kw
    settle(out, before, np.zeros((rows, ldo), bool))


@pytest.mark.parametrize("splits", [1, 2, 16])
@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_splitk_reduce_ln(dt, D, splits):
    rows, live_dev = 37, 29
    slabs, bias, resid, gamma, beta = K.ln_inputs(D, splits, rows)
    lib = L.load()
    plane = rows * D + 32
    slab_t = torch.full((splits, plane), float("nan"), device="cuda")
    slab_t[:, :rows * D] = torch.from_numpy(slabs.reshape(splits, -1)).cuda()
    bias_t, gamma_t, beta_t = (torch.from_numpy(a).cuda() for a in (bias, gamma, beta))
    resid_t = torch.full((rows, D + 4), float("nan"), device="cuda")
    resid_t[:, :D] = torch.from_numpy(resid).cuda()
    m_t = torch.tensor([live_dev], dtype=torch.int32, device="cuda")
    ldx = D + 4
    worst = 0.0

    def call(live, use_bias, res, kind):
        """-> x (float32 numpy [live, D]), y (float64 numpy [live, ldy]) after both buffer contracts."""
        ncol = 3 * D if kind == 2 else D
        ldy = ncol + 8
        fill = None
        if res == "alias":
            fill = torch.full((rows, ldx), float("nan"), device="cuda")
            fill[:, :D] = resid_t[:, :D]
        x, x_before = poisoned(rows, ldx, torch.float32, fill)
        y, y_before = poisoned(rows, ldy, torch.float32 if kind == 0 else TD[dt])
        rp, ldr = (None, 0) if res == "none" else (resid_t.data_ptr(), D + 4) if res == "separate" else (x.data_ptr(), ldx)
        L.check(lib.ofx_splitk_reduce_ln(slab_t.data_ptr(), plane, splits, bias_t.data_ptr() if use_bias else None, rp, ldr, x.data_ptr(), ldx,
                                         gamma_t.data_ptr(), beta_t.data_ptr(), y.data_ptr(), ldy, kind, EPS, rows, m_t.data_ptr() if live < rows else None,
                                         D, DT[dt], stream()), "ofx_splitk_reduce_ln")
        torch.cuda.synchronize()
        settle(x, x_before, cols_written(rows, ldx, D, np.arange(live)))
        yv = settle(y, y_before, cols_written(rows, ldy, ncol, np.arange(live)))
        return x[:live, :D].cpu().numpy(), yv[:live], x

    for live in (live_dev, rows):
        for use_bias in (True, False):
            for res in ("none", "separate", "alias"):
                want = K.slab_sum(slabs[:, :live], bias if use_bias else None, None if res == "none" else resid[:live])
                for kind in (1, 2):
                    xg, yv, _ = call(live, use_bias, res, kind)
                    assert np.array_equal(xg.view(np.int32), want.view(np.int32)), ("x: not the float32 sum in the stated order", live, use_bias, res)
                    got = yv[:, :D] if kind == 1 else split3_sum(yv, D, "y")
                    err, bound = np.abs(got - K.ln_ref(xg, gamma, beta, EPS)), K.ln_bound(xg, gamma, beta, EPS, (dt, kind))
                    worst = max(worst, float((err / bound).max()))
                    assert (err <= bound).all(), (live, use_bias, res, kind, float((err / bound).max()))
    # against ofx_layernorm on the same x, both as fp32: each inside the fp32 bound, so within twice it of each other - not bit for bit
    xg, y0, x_t = call(rows, True, "separate", 0)
    xc = x_t[:rows, :D].contiguous()
    y_ln, ln_before = poisoned(rows, D, torch.float32)
    L.check(lib.ofx_layernorm(xc.data_ptr(), None, gamma_t.data_ptr(), beta_t.data_ptr(), y_ln.data_ptr(), rows, D, D, 0, DT[dt], EPS, stream()), "ofx_layernorm")
    ln = settle(y_ln, ln_before, np.ones((rows, D), bool))
    b32 = K.ln_bound(xg, gamma, beta, EPS)
    e32 = np.abs(y0[:, :D] - K.ln_ref(xg, gamma, beta, EPS))
    assert (e32 <= b32).all() and (np.abs(y0[:, :D] - ln) <= 2 * b32).all()
    print(f"RATIO E splitk_reduce_ln {dt} D={D} splits={splits} worst err/bound={worst:.4f} fp32 output err/bound={float((e32 / b32).max()):.4f} "
          f"vs ofx_layernorm max|d|/bound={float((np.abs(y0[:, :D] - ln) / b32).max()):.4f} bit-equal={bool(np.array_equal(y0[:, :D], ln))}")


def test_splitk_reduce_ln_refusals_launch_nothing():
    rows, D = 5, 512
    lib = L.load()
    slab = torch.zeros(2, rows * D, device="cuda")
    g = torch.ones(D, device="cuda")
    x, xb = poisoned(rows, D, torch.float32)
    y, yb = poisoned(rows, D, torch.bfloat16)

    def call(s=slab.data_ptr(), plane=rows * D, xp=x.data_ptr(), yp=y.data_ptr(), gp=g.data_ptr(), d=D, ldx=D, ldy=D, kind=1, dt=1, n=rows):
        return lib.ofx_splitk_reduce_ln(s, plane, 2, None, None, 0, xp, ldx, gp, g.data_ptr(), yp, ldy, kind, EPS, n, None, d, dt, stream())

    for kw in (dict(s=None), dict(xp=None), dict(yp=None), dict(gp=None), dict(dt=0), dict(plane=rows * D + 2), dict(xp=x.data_ptr() + 4), dict(yp=y.data_ptr() + 2)):
        assert call(**kw) == OFX_EINVAL, kw
    for kw in (dict(d=640), dict(ldx=D - 4), dict(ldy=D + 2), dict(kind=2), dict(kind=3), dict(n=0), dict(plane=rows * D - 4)):
        assert call(**kw) == OFX_ESHAPE, kw
    settle(x, xb, np.zeros((rows, D), bool))
    settle(y, yb, np.zeros((rows, D), bool))
