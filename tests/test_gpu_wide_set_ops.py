"""Op-level float64 tests, on a real MI355X and through the C ABI, of what the wide outfit transformer (16 heads of 96, d_model 1536)
adds on the hot path: set_attention_kernel's HD = 96 instances in every input mode and the LayerNorm / split-K-reduce-LN instances at
D = 1536.

Method, helpers and factors are tests/test_gpu_attention_fwd.py's, unchanged (its docstring says where each factor comes from): n_head = 3
(D = 288), 7 sets, sequence 2 with q x 4, both operand types, every output NaN-poisoned with two guard rows behind it and every
not-to-be-written element compared bit for bit; accuracy per (set, head) block relative to ||ref||.
  fp32 output:            e_kernel <= 2 max(e over the five float32 orders, 2^-26); the kernel's own order is shown inside 1.25 x that
                          envelope on these very inputs by tests/test_cpu_wide_set.py
  operand type / split3:  e_kernel <= 1.6 max(e_emul with P unrounded, 1e-2 u)
  S = 1: the output is v bit for bit; split3 copies 0 and 2 bit-equal, copy 0 bit-equal to the plain call
  slab input: bit for bit ofx_set_attention on the numpy float32 sum ((s0 + s1) + ...) + bias, with cancelling pairs in the slabs
  LayerNorm at 1536: x bit for bit the stated sum, y per element inside oracle/splitk_ops.ln_bound, the two kernels within twice the fp32 bound
Every SMAX instance (8, 20, 32, 64) ships at heads of 96 - the 64-row one declares 68.6 KB of LDS, inside gfx950's 160 KiB per workgroup -
so the longest set is 64 rows as at heads of 64, and the refusal beyond it is the same one.

MEASURED (MI355X), worst ratio to the yardstick (every test prints its RATIO lines):
  fp32 output / max(e over the float32 orders, 2^-26), per SMAX 8 | 20 | 32 | 64:  varlen sets 1.141  1.016  0.977  1.213 (same for both
      operand types: the output is fp32); fixed length with the tail mask, S = 8 | 17 | 33: 1.017  0.741  0.739 - nothing near the factor 2
  operand-type output 1.000 of its emulation everywhere (also ofx_set_attention_op), split3 rows 0.03 - 0.10 of the floor 1e-2 u
  slab input and the LayerNorm's x: bit for bit in every call; LayerNorm y worst err / bound 0.972 (bf16), 0.894 (f16); the fused kernel and
      ofx_layernorm on the same x differ by at most 0.0036 of the fp32 bound
"""
import ctypes as C

import numpy as np
import pytest
import torch

import wide_set_cases as WS
from oracle import attn_fwd as A
from oracle import splitk_ops as K
from test_gpu_attention_fwd import (DT, EPS, F_F32, F_OP, FLOOR_F32, OFX_EINVAL, OFX_ESHAPE, TD, U, bits, cols_written, judge, poisoned, settle,
                                    split3_sum, stream)

pytestmark = pytest.mark.gpu

H, W, NSEQ, SCALE = WS.H, WS.W, WS.NSEQ, WS.SCALE
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


def f32_out(rows, kind, dt):
    """-> buffer, bits before, ldo, written columns: fp32 [W + 4] | operand type [W + 8] | [3 W + 8]."""
    ncol = 3 * W if kind == 2 else W
    ldo = ncol + (4 if kind == 0 else 8)
    buf, before = poisoned(rows, ldo, torch.float32 if kind == 0 else TD[dt])
    return buf, before, ldo, ncol


def judge_f32(vals, kind, dt, ref, orders, emul_of, to_blocks, label):
    if kind == 0:
        return judge(to_blocks(vals[:, :W]), ref, list(orders.values()), FLOOR_F32, F_F32, label)
    got = vals[:, :W] if kind == 1 else split3_sum(vals, W, label)
    return judge(to_blocks(got), ref, emul_of(kind == 2), 1e-2 * U[dt], F_OP, label)


# ------------------------------------------------------------------------------------------------ ofx_set_attention at heads of 96
@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("max_len", sorted(WS.SET_LENS))
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_f32_set_attention_head_96_every_smax(dt, max_len, row0):
    lens = WS.SET_LENS[max_len]
    assert {1, max_len - 1, max_len} <= set(lens)
    cu, qkv = WS.varlen_qkv(lens)
    rows = int(cu[-1])
    qkv_t, cu_t = torch.from_numpy(qkv).cuda(), torch.from_numpy(cu).cuda()
    plain_bits = None
    for kind in (1, 0, 2):
        out, before, ldo, ncol = f32_out(rows, kind, dt)
        L.check(L.load().ofx_set_attention(qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, H, W, ldo, kind, max_len, row0, SCALE, DT[dt],
                                           stream()), "ofx_set_attention")
        vals = settle(out, before, cols_written(rows, ldo, ncol, cu[:-1] if row0 else None))
        if kind == 1:
            plain_bits = bits(out)[:rows, :W].cpu().numpy()
        if kind == 2:
            assert np.array_equal(bits(out)[:rows, :W].cpu().numpy(), plain_bits), "split3 copy 0 differs from the plain call"
        worst = 0.0
        for b, (S, (ref, orders)) in enumerate(zip(lens, WS.f32_yardsticks_varlen(max_len))):
            nq = 1 if row0 else S
            sl = qkv[cu[b]:cu[b + 1]].astype(np.float64)
            q, k, v = (WS.seq_heads(sl[:, i * W:(i + 1) * W], S) for i in range(3))
            emul_of = lambda s3: A.attn_fwd_emul(q, k, v, None, SCALE, dt, split3=s3, round_p=False)[:, :nq]
            blocks = lambda a: WS.seq_heads(a[cu[b]:cu[b + 1]], S)[:, :nq]
            worst = max(worst, judge_f32(vals, kind, dt, ref[:, :nq], {o: a[:, :nq] for o, a in orders.items()}, emul_of, blocks, f"seq {b} S={S}"))
            if S == 1 and kind == 0:
                got32 = out[int(cu[b]), :W].cpu().numpy()
                assert np.array_equal(got32.view(np.int32), qkv[cu[b], 2 * W:].view(np.int32)), "S = 1: P = 1, the output is v bit for bit"
        print(f"RATIO head96 f32-set {dt} SMAX={max_len} kind={kind} row0={row0} worst={worst:.3f}")


@pytest.mark.parametrize("max_len", [20, 64])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_set_attention_op_head_96(dt, max_len):
    """set_attention_kernel<T, SMAX, T, 96>: operand-type q | k | v, fp32 P, the output rounded once (not on this model's path)."""
    lens = WS.SET_LENS[max_len]
    cu, qkv = WS.varlen_qkv(lens)
    rows = int(cu[-1])
    qkv_t, cu_t = torch.from_numpy(qkv).cuda().to(TD[dt]).contiguous(), torch.from_numpy(cu).cuda()
    q64 = qkv_t.double().cpu().numpy()
    out, before = poisoned(rows, W + 8, TD[dt])
    L.check(L.load().ofx_set_attention_op(qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, H, W, W + 8, 1, max_len, 0, SCALE, 0.0, 0, 0, DT[dt],
                                          stream()), "ofx_set_attention_op")
    vals = settle(out, before, cols_written(rows, W + 8, W))
    worst = 0.0
    for b, S in enumerate(lens):
        q, k, v = (WS.seq_heads(q64[cu[b]:cu[b + 1], i * W:(i + 1) * W], S) for i in range(3))
        ref = A.attn_fwd_ref(q, k, v, None, SCALE)
        emul = A.attn_fwd_emul(q, k, v, None, SCALE, dt, round_p=False)
        worst = max(worst, judge(WS.seq_heads(vals[cu[b]:cu[b + 1], :W], S), ref, emul, 1e-2 * U[dt], F_OP, f"seq {b} S={S}"))
    print(f"RATIO head96 valu-op {dt} max_len={max_len} worst={worst:.3f}")


# ------------------------------------------------------------------------------------------------ ofx_set_attention_slabs at heads of 96
@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("max_len", [8, 20, 32])
@pytest.mark.parametrize("splits", [1, 2, 5])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_set_attention_from_slabs_head_96_is_the_separate_pass_bit_for_bit(dt, splits, max_len, row0, kind):
    lens = WS.SET_LENS[max_len]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = int(cu[-1])
    g = np.random.default_rng(96 + 31 * splits + max_len)
    slabs = K.cancelling_slabs(g, splits, (rows, 3 * W), n_pairs=64)
    slabs[:, cu[WS.PEAKED]:cu[WS.PEAKED + 1], :W] *= np.float32(2.0)
    bias = (0.5 * g.standard_normal(3 * W)).astype(np.float32) if splits > 1 else None       # one slab is the plain path: nothing is added
    lib = L.load()
    cu_t = torch.from_numpy(cu).cuda()
    bias_t = None if bias is None else torch.from_numpy(bias).cuda()
    summed = torch.from_numpy(K.slab_sum(slabs, bias)).cuda()           # numpy float32, slabs ascending, then the bias
    plane = rows * 3 * W + 64
    buf = torch.full((splits, plane), float("nan"), device="cuda")
    buf[:, :rows * 3 * W] = torch.from_numpy(slabs.reshape(splits, -1)).cuda()

    def run(f):
        out, before, ldo, ncol = f32_out(rows, kind, dt)
        L.check(f(out.data_ptr(), ldo), "set attention")
        settle(out, before, cols_written(rows, ldo, ncol, cu[:-1] if row0 else None))
        return bits(out).cpu().numpy()

    want = run(lambda o, ldo: lib.ofx_set_attention(summed.data_ptr(), o, cu_t.data_ptr(), NSEQ, H, W, ldo, kind, max_len, row0, SCALE, DT[dt], stream()))
    got = run(lambda o, ldo: lib.ofx_set_attention_slabs(buf.data_ptr(), plane, splits, None if bias_t is None else bias_t.data_ptr(), o, cu_t.data_ptr(),
                                                         NSEQ, H, W, ldo, kind, max_len, row0, SCALE, DT[dt], stream()))
    assert np.array_equal(got, want), "slab input: other bits than ofx_set_attention on the summed array"
    if splits == 5:                                                     # the inputs show a wrong order: the last two slabs swapped give other bits
        swapped = torch.from_numpy(K.slab_sum(slabs[[0, 1, 2, 4, 3]], bias)).cuda()
        assert not torch.equal(swapped, summed)


# ------------------------------------------------------------------------------------------------ the fixed-length masked mode at heads of 96
@pytest.mark.parametrize("S", [8, 17, 33])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_f32_fixed_length_masked_attention_head_96(dt, S):
    """ofx_attention_f32: one mask family (per-sequence tails) plus a sequence that ignores every key - its rows exactly zero."""
    mask, dead = WS.tail_mask(S)
    mask_t = torch.from_numpy(mask).cuda()
    qkv = WS.fixed_qkv(S)
    rows = NSEQ * S
    q, k, v = (WS.heads(qkv[:, i * W:(i + 1) * W].astype(np.float64), S) for i in range(3))
    ref = A.attn_fwd_ref(q, k, v, dead, SCALE)
    full = np.broadcast_to(dead, (NSEQ, H, S, S)).all(-1)
    assert full.any() and not ref[full].any()
    orders = {o: A.attn_fwd_f32(q, k, v, dead, SCALE, o) for o in A.ORDERS}
    emul_of = lambda s3: A.attn_fwd_emul(q, k, v, dead, SCALE, dt, split3=s3, round_p=False)
    qkv_t = torch.from_numpy(qkv).cuda()
    for kind in (0, 1, 2):
        out, before, ldo, ncol = f32_out(rows, kind, dt)
        L.check(L.load().ofx_attention_f32(qkv_t.data_ptr(), out.data_ptr(), mask_t.data_ptr(), NSEQ, S, H, W, ldo, kind, WS.MASK_LD, 0, SCALE, DT[dt],
                                           stream()), "ofx_attention_f32")
        vals = settle(out, before, cols_written(rows, ldo, ncol))
        for c in range(3 if kind == 2 else 1):
            assert not WS.heads(vals[:, c * W:(c + 1) * W], S)[full].any(), f"kind {kind} copy {c}: a fully masked row must be exactly zero"
        worst = judge_f32(vals, kind, dt, ref, orders, emul_of, lambda a: WS.heads(a, S), f"kind {kind}")
        print(f"RATIO head96 f32-fixed {dt} S={S} kind={kind} worst={worst:.3f}")


# ------------------------------------------------------------------------------------------------ LayerNorm at D = 1536
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_layernorm_and_splitk_reduce_ln_at_1536(dt, splits):
    D, rows, live_dev = 1536, 37, 29
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
        settle(x, x_before, cols_written(rows, ldx, D, np.arange(live)))
        yv = settle(y, y_before, cols_written(rows, ldy, ncol, np.arange(live)))
        return x[:live, :D].cpu().numpy(), yv[:live], x

    for live in (live_dev, rows):
        for use_bias, res in ((True, "separate"), (False, "none"), (True, "alias")):
            want = K.slab_sum(slabs[:, :live], bias if use_bias else None, None if res == "none" else resid[:live])
            for kind in (0, 1, 2):
                xg, yv, _ = call(live, use_bias, res, kind)
                assert np.array_equal(xg.view(np.int32), want.view(np.int32)), ("x: not the float32 sum in the stated order", live, use_bias, res)
                got = split3_sum(yv, D, "y") if kind == 2 else yv[:, :D]
                err, bound = np.abs(got - K.ln_ref(xg, gamma, beta, EPS)), K.ln_bound(xg, gamma, beta, EPS, (dt, kind) if kind else None)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (live, use_bias, res, kind, float((err / bound).max()))
    # ofx_layernorm on the same x: every out_kind inside its bound, and as fp32 within twice the fp32 bound of the fused kernel
    xg, y0, x_t = call(rows, True, "separate", 0)
    xc = x_t[:rows, :D].contiguous()
    b32 = K.ln_bound(xg, gamma, beta, EPS)
    ref = K.ln_ref(xg, gamma, beta, EPS)
    for kind in (0, 1, 2):
        ncol = 3 * D if kind == 2 else D
        y_ln, ln_before = poisoned(rows, ncol + 8, torch.float32 if kind == 0 else TD[dt])
        L.check(lib.ofx_layernorm(xc.data_ptr(), None, gamma_t.data_ptr(), beta_t.data_ptr(), y_ln.data_ptr(), rows, D, ncol + 8, kind, DT[dt], EPS, stream()),
                "ofx_layernorm")
        ln = settle(y_ln, ln_before, cols_written(rows, ncol + 8, ncol))
        got = split3_sum(ln, D, "ln") if kind == 2 else ln[:, :D]
        assert (np.abs(got - ref) <= K.ln_bound(xg, gamma, beta, EPS, (dt, kind) if kind else None)).all(), kind
        if kind == 0:
            assert (np.abs(y0[:, :D] - got) <= 2 * b32).all()
            print(f"RATIO head96 ln D=1536 {dt} splits={splits} fused worst err/bound={worst:.4f} fused vs ofx_layernorm max|d|/bound="
                  f"{float((np.abs(y0[:, :D] - got) / b32).max()):.4f}")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_eshape_and_write_nothing():
    lib = L.load()
    lens = WS.SET_LENS[8]
    cu, qkv = WS.varlen_qkv(lens)
    rows = int(cu[-1])
    cu_t = torch.from_numpy(cu).cuda()
    qkv_t = torch.from_numpy(qkv).cuda()
    qkv_op = qkv_t.to(torch.bfloat16).contiguous()
    out, before, ldo, _ = f32_out(rows, 0, "bf16")
    outb, beforeb = poisoned(rows, 3 * W, torch.bfloat16)
    d_o = torch.zeros(rows, W, device="cuda")
    # heads of 80: D = n_head * 80
    assert lib.ofx_set_attention(qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, H, H * 80, ldo, 0, 8, 0, SCALE, 1, stream()) == OFX_ESHAPE
    assert b"64 or 96" in lib.ofx_last_error()
    # heads of 96 beyond the longest set (64 rows, as at heads of 64)
    assert lib.ofx_set_attention(qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, H, W, ldo, 0, 65, 0, SCALE, 1, stream()) == OFX_ESHAPE
    # the slab input keeps its own limit of 32 rows
    assert lib.ofx_set_attention_slabs(qkv_t.data_ptr(), rows * 3 * W, 2, qkv_t.data_ptr(), out.data_ptr(), cu_t.data_ptr(), NSEQ, H, W, ldo, 0, 33, 0, SCALE,
                                       1, stream()) == OFX_EINVAL
    # the MFMA kernels are head-64 only
    assert lib.ofx_attention_varlen(qkv_op.data_ptr(), outb.data_ptr(), cu_t.data_ptr(), NSEQ, 8, H, 3 * W, 3 * W, W, 2 * W, 0, SCALE, 0.0, 0, 0, 1,
                                    stream()) == OFX_ESHAPE
    assert b"heads of 96" in lib.ofx_last_error()
    for mfma in (1, 0):
        assert lib.ofx_set_attention_bwd(qkv_op.data_ptr(), d_o.data_ptr(), outb.data_ptr(), cu_t.data_ptr(), NSEQ, H, W, 8, 0, SCALE, 0.0, 0, 0, mfma, 1,
                                         stream()) == OFX_ESHAPE, mfma
    settle(out, before, np.zeros((rows, ldo), bool))
    settle(outb, beforeb, np.zeros((rows, 3 * W), bool))


def test_create_refuses_other_head_widths_and_training_is_refused_at_entry():
    lib = L.load()

    def desc(d_model, n_head, prec=L.PREC_BF16):
        d = L.default_desc()
        d.d_model, d.n_head, d.outfit_precision = d_model, n_head, prec
        return d

    for d_model, n_head in ((1536, 24), (1280, 20), (1280, 16), (1024, 0)):        # (1536 as 24 heads of 64 is no model of the reference: refused too)
        assert lib.ofx_create(0, C.byref(desc(d_model, n_head))) is None, (d_model, n_head)
        assert b"n_head*96" in lib.ofx_last_error()
    h = lib.ofx_create(0, C.byref(desc(1536, 16)))
    assert h
    try:
        B, Lmax = 2, 4
        x = torch.zeros(B, Lmax, 1536, device="cuda")
        mask = torch.zeros(B, Lmax, dtype=torch.uint8, device="cuda")
        logits, lb = poisoned(B, 4, torch.float32)
        tape, tb = poisoned(64, 1024, torch.float32)
        ws, wb = poisoned(64, 1024, torch.float32)
        rc = lib.ofx_cp_train_fwd(h, x.data_ptr(), mask.data_ptr(), B, Lmax, logits.data_ptr(), tape.data_ptr(), 64 * 1024 * 4, ws.data_ptr(), 64 * 1024 * 4,
                                  0.0, 0, stream())
        assert rc == OFX_ESHAPE and b"training needs heads of 64" in lib.ofx_last_error()
        for buf, b4, shape in ((logits, lb, (B, 4)), (tape, tb, (64, 1024)), (ws, wb, (64, 1024))):
            settle(buf, b4, np.zeros(shape, bool))
    finally:
        lib.ofx_destroy(h)
