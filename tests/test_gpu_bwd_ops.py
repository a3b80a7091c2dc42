"""Op-level float64 tests of the non-attention kernels of the training backward on a real MI355X, through the C ABI (ctypes):
everything in outfitx_amd/csrc/backward.hip but the attention (tests/test_gpu_attention_train.py) and the loss, the training-only features
of the GEMM epilogue (OFX_ACT_MISH_GRAD, dropout, aux_out, m_dev) - one value chain, reached by every route the kernels take to it -, and
the TN GEMM's partial / accumulating stores.

Reference: oracle/bwd_ops.py (plain numpy float64, pinned to float64 autograd by tests/test_cpu_bwd_ops_ref.py, which also asserts the
sharpness of every sum case below).  Every op is called twice and must return the same bits; every output is poisoned with a payload NaN
and followed by guard rows / entries whose bits are checked; rows at or past a live count hold NaN in every input and must keep the poison.
Dropout masks are fetched with ofx_dropout_mask for the same (p, seed, site) and must equal oracle.bwd_ops.drop_mask bit for bit.

HOW EACH OUTPUT IS JUDGED
  exact (bit equality)
    ofx_transpose_cast: dst and row_dst = torch's round-to-nearest cast; padding columns keep the poison.
    ofx_head_bwd: dX = fp32(fp32(dlogit w) mask_head), dXb = cast(fp32(dX mask_below)), reproduced in np.float32.
    ofx_layernorm_bwd: dx_op == cast(dx . mask) from the fp32 dx the kernel returned.
    every accumulate = 1 result == fp32(prefill + the accumulate = 0 result);  aux_out == the fp32 output of the same plan with act NONE
    and the same bias;  operand-type output of ofx_gemm_train == cast(its fp32-output run);  guards, poison, determinism.
  sums (dgamma, dbeta, dcols, every ofx_colsum output, db): per column |got - ref| <= (h + 3) 2^-24 sum |terms|, ref the float64 sum of
    the terms (dcols: of the kernel's own returned fp32 dx . mask), h the longest chain of dependent fp32 additions, DERIVED from the code:
      ln_bwd_kernel + colsum_final_kernel   h = ceil(live / 1024) [rows per wave] + 3 [waves 1..3 onto wave 0] + 9 [256 block partials:
                                                16 per row group as two chains of 8, joined] + 15 [16 row groups]        (oracle.ln_h)
      colsum_partial + colsum_final         h = per + (ceil(ceil(nchunk / 16) / 2) + 1) + 15                              (oracle.cs_h)
      cp_head_bwd_kernel db                 h = ceil(B / 256) + 8 [tree over 256 threads]                                 (oracle.head_h)
  row-wise fp32 arithmetic (dx): per row e_kernel = ||got - ref|| / ||ref|| against e_emul of the np.float32 emulation of the formula:
    e_kernel <= F max(e_emul, 2^-24).
  mish' (the sweep): err = max |kernel - float64| per epilogue route; condition err <= 2^-14, assertion err <= 2 x the measured value;
    all routes return the same bits (one value chain; the sweep's accumulator is exactly 1, so split-K's order of summation cannot
    show).  Composite: |got - z32 mask mish'64(resid)| <= |z32 mask| err + 3 2^-24 |ref|, z32 the fp32 output
    of the same plan with act NONE and p = 0.

WHICH PATH EACH CASE REACHES
  ln_bwd_kernel: all six instantiations (D 512 / 768 / 1024 x bf16 / f16, oracle.LN_CASES).  M = 1: 255 idle blocks and three idle waves;
    5; 1024: one row per wave; 1025: wave 0 of block 0 takes two; 2500 static / 2309 live: 2 or 3 rows per wave, m_dev < M; 64 / 0: none.
    add none / full / [9, D] through a scattered, out-of-order add_map; p 0 / 0.1; dcols NULL / given; accumulate 0 / 1 - each at
    D = 1024 and at a smaller D.
  colsum (oracle.CS_CASES, (nchunk, per) in brackets): M = 1 (1, 1), 15 (1, 15: unrolled x 3 + tail 3), 16 (1, 16), 17 (1, 17),
    31 (1, 31), 100 (6, 17), 4095 (255, 17: odd count in the strided pass), 4096 (256, 16), 4100 (256, 17: the cap, last chunks short),
    4096 with a device count of 37 (256, 1: 219 chunks start past it), of 0, 4100 / 2311 (256, 10).  fp32 / bf16 / f16 rows, C = 4, 1020,
    1024, 2048 (valid 2024), 3072, 512 in ld 1024; gather, row_scale, three outputs (seg 1024, 340), a NULL middle output, accumulate.
  cp_head_bwd_kernel: CP with / without cu, CIR with / without cu and once with w aliasing dX; B 1 / 7 / 300 (db past 256), D 4 / 1024 /
    1028 (second trip of the column loop); head site only, below only, both with cu[b] != b.
  training epilogues, by ofx_tune(2, v) (PLANS): v = 1 epilogue (128 rows), 5 epilogue (64 rows), 2 / 3 / 4 epilogue2 in the 256x256,
    256x128 and ping-pong kernels - fp32 branch and operand-type branch -, v = 1 with ofx_tune(5, 2) and a slab: splitk_reduce_kernel.
  gemm_tn_kernel: m_valid 200 / n_valid 248 / ldc 248 / K 200 (last k-tile zero-filled in LDS) direct and through 4 slabs; accumulate.
  transpose_cast_kernel: R or C = 2024 (not a multiple of 64) in ldd 2048 / 1024, one element, 65 x 63; with and without row_dst.

  rows [m_dev, M) of a GEMM output: under every plan above they keep their poison in C and in aux_out (asserted), as include/ofx.h says.

MEASURED on the MI355X
  dx, worst e_kernel / max(e_emul, 2^-24) over all cases, per (D, dtype):
      1024 bf16 0.964   1024 f16 0.962   768 bf16 0.957   768 f16 0.962   512 bf16 0.943   512 f16 0.955
    every row sits at the 2^-24 floor (e_kernel 4.9e-8 .. 5.7e-8; the emulation's own error is smaller still): one wave's fp32 work is as
    good as numpy's.  F_DX = 1.5 x 0.964 rounded up to one decimal = 1.5.
  mish' err = max |kernel - float64| over the sweep: 4.590e-06 at u = 19.751987, the same value and place for all six routes and both
    operand types (they agree bit for bit on the sweep, as asserted): 13 x under 2^-14 = 6.1e-5.  It is twice the 2.3e-6 of
    the formula with an exact division, and for a reason that can be read off: near u = 20, n = e^u (e^u + 2) ~ 1.5e17 swallows the + 2,
    the true 1 - t^2 is ~ 3e-17, and a t that lands k ulps (k 2^-24) under 1 gives t + u (1 - t^2) - 1 = k 2^-24 (2 u - 1).  A correctly
    rounded division gives k <= 1 (2.3e-6 at u = 19.75); n x rcp(n + 2) with the 1-ulp reciprocal and the product's rounding gives k = 2:
    2 x 2^-24 x 38.5 = 4.59e-6, the measured figure to three digits.  MISH_ERR = 4.6e-6; the assertion is err <= 2 MISH_ERR.
  sums: worst err / bound 0.075 (dgamma at 5 rows); composite mish' 0.29 of its allowance; TN GEMM 0.005 of (K + 3) 2^-24 sum |a b|.
  No kernel failed its first run, and nowhere did an operand-type output differ from the cast of the fp32 run: no allowance above "exact".
"""
import functools

import numpy as np
import pytest
import torch

from oracle import bwd_ops as R

pytestmark = pytest.mark.gpu

OFX_EINVAL, OFX_ESHAPE, OFX_EWORKSPACE = -1, -2, -4
ACT_NONE, ACT_MISH, ACT_MISH_GRAD = 0, 3, 4
DT = {"bf16": 1, "f16": 2}
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
U32 = 2.0 ** -24
SEED = R.SEED
NAN32 = 0x7FC0BEEF                   # poison of fp32 outputs: a NaN no kernel computes
NANOP = {"bf16": 0x7FC5, "f16": 0x7E05}
GUARD16, GUARD32 = 0x5AA5, 0x5AA55AA5
F_DX = 1.5                           # e_kernel <= F_DX max(e_emul, 2^-24): 1.5 x the worst measured ratio (0.964), one decimal up; cap 4
MISH_ERR = 4.6e-6                    # measured max |kernel - float64| of mish' over the sweep, the same for every epilogue route

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


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def poison32(rows, cols, guard=2):
    """fp32 [rows + guard, cols]: payload NaNs followed by guard rows; and the int32 view's bits"""
    buf = torch.empty((rows + guard, cols), dtype=torch.float32, device="cuda")
    buf.view(torch.int32)[:rows] = NAN32
    buf.view(torch.int32)[rows:] = GUARD32
    return buf


def poison_op(rows, cols, dt, guard=2):
    buf = torch.empty((rows + guard, cols), dtype=TD[dt], device="cuda")
    buf.view(torch.int16)[:rows] = NANOP[dt]
    buf.view(torch.int16)[rows:] = GUARD16
    return buf


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def is_poison(t):
    """elementwise: still the poison bits"""
    return bits(t) == (NAN32 if t.dtype == torch.float32 else (NANOP["bf16"] if t.dtype == torch.bfloat16 else NANOP["f16"]))


def guards_ok(t, rows):
    return bool((bits(t)[rows:] == (GUARD32 if t.dtype == torch.float32 else GUARD16)).all())


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def nan_rows(a, M, dtype=torch.float32):
    """device [M, ...] whose first len(a) rows are `a` and the rest NaN"""
    t = torch.full((M,) + a.shape[1:], float("nan"), dtype=dtype, device="cuda")
    if len(a):
        t[:len(a)] = dev(a).to(dtype)
    return t


def fetched_mask(p, site, rows, cols):
    """The library's mask of the site, fp32 [rows, cols] on the device - and it equals the oracle's hash bit for bit."""
    if p == 0 or site < 0 or rows == 0:
        return torch.ones((rows, cols), dtype=torch.float32, device="cuda")
    m = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
    L.check(L.load().ofx_dropout_mask(p, SEED, site, rows, cols, m.data_ptr(), stream()), "ofx_dropout_mask")
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), R.drop_mask(p, SEED, site, rows, cols)), "ofx_dropout_mask != oracle.drop_mask"
    return m


def sum_sheet(n_out, width, prefill=None, given=None):
    """fp32 [n_out, width + 8]: one output per row, 8 guard entries behind each; poisoned, or `prefill` in the first `width` entries"""
    buf = torch.empty((n_out, width + 8), dtype=torch.float32, device="cuda")
    buf.view(torch.int32)[:, :width] = NAN32
    buf.view(torch.int32)[:, width:] = GUARD32
    if prefill is not None:
        for k in range(n_out):
            if given is None or given[k]:
                buf[k, :prefill.shape[1]] = dev(prefill[k])
    return buf


def check_sum(name, got, terms, h, ref=None):
    """|got - ref| <= (h + 3) 2^-24 sum |terms| per column"""
    terms = np.asarray(terms, np.float64)
    ref = terms.sum(0) if ref is None else ref
    bound = R.sum_bound(terms, h)
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300), initial=0.0)) if terms.shape[0] else float(err.max(initial=0.0))
    print(f"SUM {name} h={h} worst err/bound={worst:.3f}")
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (name, bad[:8], err[bad[:8]], bound[bad[:8]])


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_call(i, accumulate):
    D, dt, M, live, add_kind, p, dcols, acc = R.LN_CASES[i]
    inp, n = R.ln_inputs(i), R.ln_live(R.LN_CASES[i])
    lib = L.load()
    dy, x, stats = nan_rows(inp["dy"], M), nan_rows(inp["x"], M), nan_rows(inp["stats"], M)
    gamma = dev(inp["gamma"])
    add = add_map = None
    if add_kind == "full":
        add = nan_rows(inp["add"], M)
    elif add_kind == "map":
        add = dev(inp["add"])
        add_map = torch.zeros(M, dtype=torch.int32, device="cuda")           # dead rows: a VALID index, so that a read would only show as a value
        add_map[:n] = dev(inp["add_map"])
    m_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
    dx, dx_op = poison32(M, D), poison_op(M, D, dt)
    sums = sum_sheet(3, D, inp["prefill"] if accumulate else None, given=(1, 1, dcols))
    ws_bytes = lib.ofx_layernorm_bwd_ws(D)
    assert ws_bytes == 256 * 3 * D * 4
    ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(lib.ofx_layernorm_bwd(dy.data_ptr(), x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), ptr(add), ptr(add_map), dx.data_ptr(), dx_op.data_ptr(),
                                  sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr() if dcols else None, M, ptr(m_dev), D, p, SEED, R.LN_SITE,
                                  accumulate, DT[dt], ws.data_ptr(), ws_bytes, stream()), "ofx_layernorm_bwd")
    torch.cuda.synchronize()
    return dx, dx_op, sums


@pytest.mark.parametrize("i", range(len(R.LN_CASES)), ids=[f"D{c[0]}-{c[1]}-M{c[2]}-live{c[3]}-{c[4]}-p{c[5]}-dcols{int(c[6])}-acc{c[7]}" for c in R.LN_CASES])
def test_layernorm_bwd(i):
    case = R.LN_CASES[i]
    D, dt, M, live, add_kind, p, dcols, acc = case
    inp, n, h = R.ln_inputs(i), R.ln_live(case), R.ln_h(case)
    dx, dx_op, sums = ln_call(i, 0)
    dx2, dx_op2, sums2 = ln_call(i, 0)
    assert same_bits(dx, dx2) and same_bits(dx_op, dx_op2) and same_bits(sums, sums2), "two calls, two results"
    # ---- buffer contracts
    assert guards_ok(dx, M) and guards_ok(dx_op, M) and bool((bits(sums)[:, D:] == GUARD32).all())
    assert bool(is_poison(dx[n:M]).all()) and bool(is_poison(dx_op[n:M]).all()), "rows at or past the live count are not written"
    assert bool(torch.isfinite(dx[:n]).all()) and bool(torch.isfinite(dx_op[:n].float()).all())
    assert dcols or bool(is_poison(sums[2, :D]).all()), "NULL dcols"
    mask = fetched_mask(p, R.LN_SITE, n, D)
    ref = R.ln_reference(i, mask.cpu().numpy())
    # ---- dx_op == cast(dx . mask), from the kernel's own fp32 dx
    dropped = dx[:n] * mask
    assert same_bits(dx_op[:n], dropped.to(TD[dt])), "dx_op != cast(dx . mask)"
    # ---- dx, row by row against the fp32 emulation
    if n:
        got = dx[:n].double().cpu().numpy()
        emul = R.ln_bwd_dx_emul(inp["dy"], inp["x"], inp["stats"][:, 0], inp["stats"][:, 1], inp["gamma"], inp["add"], inp["add_map"]).astype(np.float64)
        nr = np.linalg.norm(ref["dx"], axis=1)
        ek, ee = np.linalg.norm(got - ref["dx"], axis=1) / nr, np.linalg.norm(emul - ref["dx"], axis=1) / nr
        ratio = ek / np.maximum(ee, U32)
        print(f"RATIO dx D={D} {dt} M={M} live={n} add={add_kind} worst={ratio.max():.3f} (row {ratio.argmax()}, e_kernel {ek[ratio.argmax()]:.3e})")
        bad = np.nonzero(~(ek <= F_DX * np.maximum(ee, U32)))[0]
        assert bad.size == 0, (bad[:8], ek[bad[:8]], ee[bad[:8]])
    # ---- the three column sums
    check_sum("dgamma", sums[0, :D].cpu().numpy(), ref["t_dgamma"], h, ref["dgamma"])
    check_sum("dbeta", sums[1, :D].cpu().numpy(), ref["t_dbeta"], h, ref["dbeta"])
    if dcols:
        check_sum("dcols", sums[2, :D].cpu().numpy(), dropped.double().cpu().numpy(), h)
    if n == 0:
        assert not sums[:2, :D].any(), "no live row: the sums are exactly zero"
    # ---- accumulate: one fp32 addition onto the prefill
    if acc:
        dx3, dx_op3, sums3 = ln_call(i, 1)
        assert same_bits(dx3, dx) and same_bits(dx_op3, dx_op)
        rows = [0, 1] + ([2] if dcols else [])
        want = dev(inp["prefill"])[rows] + sums[rows, :D]
        assert same_bits(sums3[rows, :D], want), "accumulate != fp32(prefill + result)"
        assert bool((bits(sums3)[:, D:] == GUARD32).all()) and (dcols or bool(is_poison(sums3[2, :D]).all()))


# ------------------------------------------------------------------------------------------------ column sums
def cs_call(i, accumulate):
    kind, C, ld, M, live, gather, scale, outs, valid, acc = R.CS_CASES[i]
    inp, n = R.cs_inputs(i), R.cs_live(R.CS_CASES[i])
    lib = L.load()
    td = torch.float32 if kind == "f32" else TD[kind]
    table = inp["table"].copy()
    table[:, C:] = np.nan                                       # columns C .. ld - 1 are never read
    if gather:
        x = dev(table).to(td) if len(table) else torch.full((1, ld), float("nan"), dtype=td, device="cuda")
        gi = torch.zeros(M, dtype=torch.int32, device="cuda")
        gi[:n] = dev(inp["gather"])
    else:
        x, gi = nan_rows(table, M, td), None
    sc = nan_rows(inp["scale"], M) if scale else None
    m_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
    seg = C // len(outs)
    sheet = sum_sheet(len(outs), seg, inp["prefill"][:, :(valid or seg)] if accumulate else None, given=outs)
    o = [sheet[k].data_ptr() if k < len(outs) and outs[k] else None for k in range(3)]
    ws_bytes = lib.ofx_colsum_ws(C)
    assert ws_bytes == 256 * C * 4
    ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(lib.ofx_colsum(x.data_ptr(), 0 if kind == "f32" else 1, ld, ptr(gi), ptr(sc), o[0], o[1], o[2], seg, C, valid, M, ptr(m_dev), accumulate,
                           DT.get(kind, 1), ws.data_ptr(), ws_bytes, stream()), "ofx_colsum")
    torch.cuda.synchronize()
    return sheet


@pytest.mark.parametrize("i", range(len(R.CS_CASES)), ids=[f"{c[0]}-C{c[1]}-ld{c[2]}-M{c[3]}-live{c[4]}-g{c[5]}-s{c[6]}-o{len(c[7])}-v{c[8]}-acc{c[9]}" for c in R.CS_CASES])
def test_colsum(i):
    case = R.CS_CASES[i]
    kind, C, ld, M, live, gather, scale, outs, valid, acc = case
    n, h, seg, inp = R.cs_live(case), R.cs_h(case), C // len(case[7]), R.cs_inputs(i)
    v = valid or seg
    sheet = cs_call(i, 0)
    assert same_bits(sheet, cs_call(i, 0)), "two calls, two results"
    assert bool((bits(sheet)[:, seg:] == GUARD32).all()), "guards behind every output"
    assert bool(is_poison(sheet[:, v:seg]).all()), "entries at or past `valid` are not written"
    ref, terms = R.cs_reference(i)
    for k, on in enumerate(outs):
        if not on:
            assert bool(is_poison(sheet[k, :seg]).all()), "a NULL output's neighbours in the sheet"
            continue
        check_sum(f"out{k}", sheet[k, :v].cpu().numpy(), terms[:, k * seg:k * seg + v], h)
        if n == 0:
            assert not sheet[k, :v].any(), "no live row: zeros"
    if acc:
        sheet2 = cs_call(i, 1)
        on = [k for k, o_ in enumerate(outs) if o_]
        assert same_bits(sheet2[on, :v], dev(inp["prefill"])[on, :v] + sheet[on, :v]), "accumulate != fp32(prefill + result)"
        assert bool((bits(sheet2)[:, seg:] == GUARD32).all()) and bool(is_poison(sheet2[:, v:seg]).all())


# ------------------------------------------------------------------------------------------------ head backward
HEAD_DB_NULL = {3}                   # CP cases whose db is NULL


def head_call(i, accumulate):
    mode, B, D, cu, hs, bs, acc, alias, dt = R.HEAD_CASES[i]
    inp = R.head_inputs(i)
    rows = inp["rows"]
    dX, dXb = poison32(rows, D), poison_op(rows, D, dt)
    if alias:
        dX[:B] = dev(inp["w"])
        w = dX
    else:
        w = dev(inp["w"])
    dl = None if mode == "cir" else dev(inp["dlogits"])
    cu_t = dev(inp["cu"]) if cu else None
    db = None
    if mode == "cp" and i not in HEAD_DB_NULL:
        db = sum_sheet(1, 1, np.full((1, 1), inp["prefill"], np.float32) if accumulate else None)
    L.check(L.load().ofx_head_bwd(ptr(dl), w.data_ptr(), ptr(cu_t), dX.data_ptr(), dXb.data_ptr(), ptr(db), B, D, R.HEAD_P, SEED, hs, bs, accumulate,
                                  DT[dt], stream()), "ofx_head_bwd")
    torch.cuda.synchronize()
    return dX, dXb, db


@pytest.mark.parametrize("i", range(len(R.HEAD_CASES)), ids=[f"{c[0]}-B{c[1]}-D{c[2]}-cu{c[3]}-head{c[4]}-below{c[5]}-acc{c[6]}-alias{c[7]}-{c[8]}" for c in R.HEAD_CASES])
def test_head_bwd(i):
    mode, B, D, cu, hs, bs, acc, alias, dt = R.HEAD_CASES[i]
    inp = R.head_inputs(i)
    rows = inp["rows"]
    r_of = inp["cu"].astype(np.int64) if cu else np.arange(B)
    dX, dXb, db = head_call(i, 0)
    dX2, dXb2, db2 = head_call(i, 0)
    assert same_bits(dX, dX2) and same_bits(dXb, dXb2) and (db is None or same_bits(db, db2)), "two calls, two results"
    assert guards_ok(dX, rows) and guards_ok(dXb, rows)
    other = np.setdiff1d(np.arange(rows), r_of)
    assert bool(is_poison(dX[other]).all()) and bool(is_poison(dXb[other]).all()), "rows of no outfit are not written"
    # the two masks, from the library; their row indices differ: outfit b for the head site, global row cu[b] for the site below
    mh = fetched_mask(R.HEAD_P, hs, B, D).cpu().numpy()
    mb = fetched_mask(R.HEAD_P, bs, rows, D).cpu().numpy()[r_of]
    f = np.float32
    v = inp["w"].astype(f) if mode == "cir" else (inp["w"].astype(f)[None, :] * inp["dlogits"].astype(f)[:, None]).astype(f)
    v = (v * mh).astype(f) if hs >= 0 else v
    assert np.array_equal(dX[r_of].cpu().numpy().view(np.int32), v.view(np.int32)), "dX != fp32(fp32(dlogit w) mask_head)"
    want_b = dev((v * mb).astype(f) if bs >= 0 else v, TD[dt])
    assert same_bits(dXb[r_of], want_b), "dXb != cast(fp32(dX mask_below))"
    ref, _ = R.head_bwd_ref(inp["dlogits"], inp["w"], mh if hs >= 0 else None)
    assert np.abs(v - ref).max() <= 2 * U32 * np.abs(ref).max()                  # and the np.float32 replica is the float64 reference
    if hs >= 0 and bs >= 0 and cu:
        assert not np.array_equal(mh, mb), "the two sites' masks differ"
    if db is not None:
        t = inp["dlogits"].astype(np.float64)[:, None]
        check_sum("db", db[0, :1].cpu().numpy(), t, R.head_h(B))
        assert bool((bits(db)[0, 1:] == GUARD32).all())
        if acc:
            _, _, db3 = head_call(i, 1)
            assert same_bits(db3[0, :1], torch.tensor([inp["prefill"]], device="cuda") + db[0, :1]) and bool((bits(db3)[0, 1:] == GUARD32).all())


# ------------------------------------------------------------------------------------------------ transpose + cast
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("with_rows", [0, 1])
@pytest.mark.parametrize("Rr,C,ldd", [(2024, 1024, 2048), (1024, 2024, 1024), (1, 1, 8), (65, 63, 72)])
def test_transpose_cast(Rr, C, ldd, with_rows, dt):
    g = np.random.default_rng(Rr * 7 + C)
    src = (g.standard_normal((Rr, C)) * np.exp2(g.integers(-12, 12, (Rr, C)))).astype(np.float32)
    # ties of both types (1 + 2^-8, 1 + 3 2^-8: to even, down and up; 1 + 2^-11 likewise), overflow of f16, its subnormals, -0
    special = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 70000.0, -65520.0, 65519.0, 1e-6, 6e-8, 2.9e-8, -0.0], np.float32)
    flat = src.reshape(-1)
    k = min(len(special), flat.size)
    flat[g.choice(flat.size, k, replace=False)] = special[:k]
    s = dev(src)
    ld_row = (C + 7) // 8 * 8 + 8
    dst, row_dst = poison_op(C, ldd, dt), (poison_op(Rr, ld_row, dt) if with_rows else None)
    dst2, row_dst2 = poison_op(C, ldd, dt), (poison_op(Rr, ld_row, dt) if with_rows else None)
    lib = L.load()
    for d_, r_ in ((dst, row_dst), (dst2, row_dst2)):
        L.check(lib.ofx_transpose_cast(s.data_ptr(), d_.data_ptr(), Rr, C, ldd, ptr(r_), ld_row if with_rows else 0, DT[dt], stream()), "ofx_transpose_cast")
    torch.cuda.synchronize()
    want = s.to(TD[dt])
    assert same_bits(dst, dst2) and guards_ok(dst, C)
    assert same_bits(dst[:C, :Rr], want.t().contiguous()), "dst != cast(src)^T"
    assert bool(is_poison(dst[:C, Rr:]).all()), "padding columns are not written"
    if with_rows:
        assert same_bits(row_dst, row_dst2) and guards_ok(row_dst, Rr)
        assert same_bits(row_dst[:Rr, :C], want) and bool(is_poison(row_dst[:Rr, C:]).all())


# ------------------------------------------------------------------------------------------------ TN GEMM into a sub-block
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("split", [0, 1])
def test_gemm_tn_into(split, dt):
    """C[:200, :248] of a 256 x 256 product with K = 200 live rows of 256 readable ones (the rest NaN: the kernel zero-fills them in LDS),
    ldc = 248 < N.  Values: |got - ref| <= (K + 3) 2^-24 sum_k |a b| (K fp32 additions in any order).  accumulate: one more addition."""
    M = N = 256
    K, mv, nv, ldc = 200, 200, 248, 248
    g = np.random.default_rng(77)
    a, b = R.round_op(R.unit_mag(g, (K, M)), dt), R.round_op(R.unit_mag(g, (K, N)), dt)
    A, B = nan_rows(a, 256, TD[dt]), nan_rows(b, 256, TD[dt])
    prefill = R.unit_mag(g, (mv, ldc)) * np.float32(300.0)
    lib = L.load()
    ws_bytes = lib.ofx_gemm_tn_ws(M, N, K)
    assert ws_bytes == 4 * M * N * 4, "the plan of this shape: 4 slabs"
    slab = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda") if split else None

    def call(accumulate):
        Cb = poison32(mv, ldc)
        if accumulate:
            Cb[:mv] = dev(prefill)
        L.check(lib.ofx_gemm_tn_into(A.data_ptr(), M, B.data_ptr(), N, Cb.data_ptr(), ldc, M, N, K, None, mv, nv, accumulate, ptr(slab),
                                     ws_bytes if split else 0, DT[dt], stream()), "ofx_gemm_tn_into")
        torch.cuda.synchronize()
        return Cb

    c0, c1 = call(0), call(0)
    assert same_bits(c0, c1) and guards_ok(c0, mv), "determinism; nothing past row m_valid (the guard rows sit where row 200 would be)"
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ref, mag = (a64.T @ b64)[:mv, :nv], (np.abs(a64).T @ np.abs(b64))[:mv, :nv]
    err = np.abs(c0[:mv].double().cpu().numpy() - ref)
    print(f"TN split={split} {dt} worst err/bound={np.max(err / ((K + 3) * U32 * mag)):.3f}")
    assert (err <= (K + 3) * U32 * mag).all()
    c2 = call(1)
    assert same_bits(c2[:mv], dev(prefill) + c0[:mv]) and guards_ok(c2, mv), "accumulate != fp32(prefill + result)"


# ------------------------------------------------------------------------------------------------ training epilogues
# name -> (ofx_tune(2, v), ofx_tune(5, v), slab): the route by which the launch reaches the epilogue's value chain (its loads and stores)
PLANS = {"epilogue-128": (1, 1, False), "epilogue-64": (5, 1, False), "epilogue2-256x256": (2, 1, False), "epilogue2-256x128": (3, 1, False),
         "epilogue2-pingpong": (4, 1, False), "splitk-reduce": (1, 2, True)}


class plan:
    """with plan(name): the knobs of PLANS[name]; both restored to their defaults (0, 1) on the way out"""

    def __init__(self, name):
        self.k2, self.k5, self.slab = PLANS[name]

    def __enter__(self):
        lib = L.load()
        try:
            L.check(lib.ofx_tune(2, self.k2), "ofx_tune(2)")
            L.check(lib.ofx_tune(5, self.k5), "ofx_tune(5)")
        except Exception:
            lib.ofx_tune(2, 0); lib.ofx_tune(5, 1)
            raise
        return self

    def __exit__(self, *exc):
        lib = L.load()
        lib.ofx_tune(2, 0); lib.ofx_tune(5, 1)
        return False


def gemm_train(p_, A, W, M, N, K, dt, *, act=ACT_NONE, out_op=False, bias=None, resid=None, aux=False, m_dev=None, p=0.0, site=2):
    """One ofx_gemm_train launch under the knobs of plan `p_` -> (C [M + 2, N], aux_out [M + 2, N] or None), poisoned and guarded."""
    lib = L.load()
    C = poison_op(M, N, dt) if out_op else poison32(M, N)
    auxb = poison32(M, N) if aux else None
    slab = slab_bytes = None
    if p_.slab:
        slab_bytes = lib.ofx_gemm_splitk_ws(M, N, K)
        assert slab_bytes == 2 * M * N * 4, "forced plan: two slabs"
        slab = torch.full((slab_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    L.check(lib.ofx_gemm_train(A.data_ptr(), W.data_ptr(), C.data_ptr(), ptr(bias), ptr(resid), ptr(auxb), M, ptr(m_dev), N, K, K, N, N, act,
                               1 if out_op else 0, p, SEED, site, DT[dt], ptr(slab), slab_bytes or 0, stream()), "ofx_gemm_train")
    torch.cuda.synchronize()
    return C, auxb


@functools.lru_cache(maxsize=None)
def sweep_run(name, dt):
    """mish' over the sweep by the route `name` takes: A and W have column 0 = 1 and zeros elsewhere, so the accumulator is exactly 1 and
    the output is the kernel's mish'(resid) -> (fp32 output [256, 256] numpy, operand-type output as fp32 numpy), checked for determinism."""
    M = N = 256
    K = 128
    A = torch.zeros((M, K), dtype=TD[dt], device="cuda"); A[:, 0] = 1
    W = torch.zeros((N, K), dtype=TD[dt], device="cuda"); W[:, 0] = 1
    u = dev(R.mish_sweep())
    with plan(name) as p_:
        c32, _ = gemm_train(p_, A, W, M, N, K, dt, act=ACT_MISH_GRAD, resid=u)
        c32b, _ = gemm_train(p_, A, W, M, N, K, dt, act=ACT_MISH_GRAD, resid=u)
        cop, _ = gemm_train(p_, A, W, M, N, K, dt, act=ACT_MISH_GRAD, resid=u, out_op=True)
        one, _ = gemm_train(p_, A, W, M, N, K, dt)
    assert same_bits(c32, c32b) and guards_ok(c32, M) and guards_ok(cop, M)
    assert bool((one[:M] == 1.0).all()), "the accumulator of the sweep is exactly 1"
    assert same_bits(cop[:M], c32[:M].to(TD[dt])), "operand-type output != cast(fp32 output)"
    return c32[:M].cpu().numpy()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(PLANS))
def test_mish_grad_sweep(name, dt):
    got = sweep_run(name, dt)
    u = R.mish_sweep()
    ref = R.mish_grad(u.astype(np.float64))
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)
    k = err.argmax()
    print(f"MISH {name} {dt} err={err.max():.3e} at u={u.ravel()[k]!r} (2^-14 = {2.0 ** -14:.3e})")
    assert err.max() <= 2.0 ** -14, "the epilogue's approximation must stay 8 x under f16's 2^-11"
    assert err.max() <= 2.0 * MISH_ERR
    assert (got[u > 20] == 1.0).all() and (np.abs(got[u == -88.0]) < 1e-30).all()
    # one value chain: every route returns the same bits
    first = sweep_run(next(iter(PLANS)), dt)
    assert np.array_equal(got.view(np.int32), first.view(np.int32)), "the routes to the mish' epilogue disagree"


@functools.lru_cache(maxsize=None)
def composite_inputs(dt):
    M, live, N, K = 300, 259, 256, 512
    g = np.random.default_rng(4242)
    a, w = R.round_op(g.standard_normal((live, K)) * 0.5, dt), R.round_op(g.standard_normal((N, K)) * 0.25, dt)
    u = (2.5 * g.standard_normal((live, N))).astype(np.float32)
    bias = g.standard_normal(N).astype(np.float32)
    res = g.standard_normal((live, N)).astype(np.float32)
    return dict(a=a, w=w, u=u, bias=bias, res=res, A=nan_rows(a, M, TD[dt]), W=dev(w, TD[dt]), U=nan_rows(u, M), B=dev(bias), RES=nan_rows(res, M),
                m_dev=torch.tensor([live], dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(PLANS))
def test_gemm_train_composite(name, dt):
    """M = 300 static, 259 live (rows 259 .. 299 of A, resid hold NaN), N = 256, K = 512, p = 0.1.  Rows [259, 300) of C and aux_out keep
    their poison under every plan; nothing at or past row 300 is touched."""
    M, live, N, K, p, site = 300, 259, 256, 512, 0.1, 6
    c = composite_inputs(dt)
    mask = fetched_mask(p, site, live, N)
    m64 = mask.double().cpu().numpy()

    def contracts(*outs):
        for o in outs:
            assert guards_ok(o, M), "rows at or past M"
            assert bool(is_poison(o[live:M]).all()), "rows [m_dev, M) are not written"
            assert bool(torch.isfinite(o[:live].float()).all())

    with plan(name) as p_:
        kw = dict(m_dev=c["m_dev"])
        z32, _ = gemm_train(p_, c["A"], c["W"], M, N, K, dt, **kw)
        # ---- (1) MISH_GRAD with the saved pre-activation in resid and dropout on the accumulator
        g32, _ = gemm_train(p_, c["A"], c["W"], M, N, K, dt, act=ACT_MISH_GRAD, resid=c["U"], p=p, site=site, **kw)
        g32b, _ = gemm_train(p_, c["A"], c["W"], M, N, K, dt, act=ACT_MISH_GRAD, resid=c["U"], p=p, site=site, **kw)
        gop, _ = gemm_train(p_, c["A"], c["W"], M, N, K, dt, act=ACT_MISH_GRAD, resid=c["U"], p=p, site=site, out_op=True, **kw)
        # ---- (2) MISH with bias, aux_out, dropout and a residual; and its pieces
        zb32, _ = gemm_train(p_, c["A"], c["W"], M, N, K, dt, bias=c["B"], **kw)
        y32, _ = gemm_train(p_, c["A"], c["W"], M, N, K, dt, act=ACT_MISH, bias=c["B"], **kw)
        f32_, aux = gemm_train(p_, c["A"], c["W"], M, N, K, dt, act=ACT_MISH, bias=c["B"], resid=c["RES"], aux=True, p=p, site=site, **kw)
        f32b, auxb = gemm_train(p_, c["A"], c["W"], M, N, K, dt, act=ACT_MISH, bias=c["B"], resid=c["RES"], aux=True, p=p, site=site, **kw)
        fop, aux_o = gemm_train(p_, c["A"], c["W"], M, N, K, dt, act=ACT_MISH, bias=c["B"], resid=c["RES"], aux=True, p=p, site=site, out_op=True, **kw)
    contracts(z32, g32, gop, zb32, y32, f32_, aux, fop, aux_o)
    assert same_bits(g32, g32b) and same_bits(f32_, f32b) and same_bits(aux, auxb), "two calls, two results"
    # the plain product against float64: K fp32 additions in any order
    a64, w64 = c["a"].astype(np.float64), c["w"].astype(np.float64)
    z = z32[:live].double().cpu().numpy()
    assert (np.abs(z - a64 @ w64.T) <= (K + 3) * U32 * (np.abs(a64) @ np.abs(w64).T)).all()
    # (1) dropout on the accumulator, THEN x mish'(resid)
    ref = z * m64 * R.mish_grad(c["u"].astype(np.float64))
    err = np.abs(g32[:live].double().cpu().numpy() - ref)
    bound = np.abs(z * m64) * MISH_ERR + 3 * U32 * np.abs(ref)
    print(f"COMPOSITE mish_grad {name} {dt} worst err/bound={np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    assert bool(((g32[:live] == 0) == (mask == 0) | (z32[:live] == 0)).all()), "zeros exactly where the mask drops"
    assert same_bits(gop[:live], g32[:live].to(TD[dt])), "operand-type output != cast(fp32 output)"
    # (2) aux_out is the pre-activation; out = mish(aux) . mask + resid with the kernel's own mish (y32): a product and a sum, fused or not
    assert same_bits(aux[:live], zb32[:live]) and same_bits(aux_o[:live], zb32[:live]), "aux_out != act NONE output with the same bias"
    y = y32[:live].double().cpu().numpy()
    want = y * m64 + c["res"].astype(np.float64)
    got = f32_[:live].double().cpu().numpy()
    assert (np.abs(got - want) <= (U32 * np.abs(y * m64) + U32 * np.abs(got)) * (1 + 2.0 ** -20)).all(), "out != mish(aux) . mask + resid"
    assert np.abs(y - R.mish(zb32[:live].double().cpu().numpy())).max() <= 2.0 ** -14 * max(1.0, float(np.abs(y).max()))
    assert same_bits(fop[:live], f32_[:live].to(TD[dt])), "operand-type output != cast(fp32 output)"


# ------------------------------------------------------------------------------------------------ rejections
def test_rejected_calls_launch_nothing():
    """NULL required pointers and misaligned ones are OFX_EINVAL, unsupported shapes OFX_ESHAPE, a short workspace OFX_EWORKSPACE - at every
    new entry point; the poisoned outputs keep their bits."""
    lib = L.load()
    D, M = 512, 8
    f = lambda *s: torch.ones(s, dtype=torch.float32, device="cuda")
    dy, x, stats, gamma = f(M, D), f(M, D), f(M, 2), f(D)
    dx, dxo, sums = poison32(M, D), poison_op(M, D, "bf16"), sum_sheet(3, 3 * D)
    ws = torch.empty(lib.ofx_layernorm_bwd_ws(1024) // 4 + 4, dtype=torch.float32, device="cuda")
    outs = [dx, dxo, sums]
    snap = lambda: [bits(o).clone() for o in outs]
    before = snap()

    def ln(dy_=dy.data_ptr(), dx_=dx.data_ptr(), dxo_=dxo.data_ptr(), D_=D, M_=M, ws_=ws.data_ptr(), wsb=None, p=0.0, dt=1, add=None, amap=None):
        wsb = lib.ofx_layernorm_bwd_ws(D_) if wsb is None else wsb
        return lib.ofx_layernorm_bwd(dy_, x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), add, amap, dx_, dxo_, sums[0].data_ptr(), sums[1].data_ptr(),
                                     sums[2].data_ptr(), M_, None, D_, p, SEED, 1, 0, dt, ws_, wsb, stream())

    assert lib.ofx_layernorm_bwd_ws(640) == 0 and lib.ofx_colsum_ws(6) == 0 and lib.ofx_colsum_ws(0) == 0
    for kw in (dict(dy_=None), dict(dx_=None), dict(dxo_=None), dict(ws_=None), dict(p=1.0), dict(p=-0.5), dict(dt=0), dict(amap=stats.data_ptr()),
               dict(dy_=dy.data_ptr() + 4), dict(dx_=dx.data_ptr() + 8), dict(dxo_=dxo.data_ptr() + 2), dict(ws_=ws.data_ptr() + 4)):
        assert ln(**kw) == OFX_EINVAL, kw
    assert ln(D_=640, wsb=1 << 30) == OFX_ESHAPE and ln(D_=256, wsb=1 << 30) == OFX_ESHAPE and ln(M_=0) == OFX_ESHAPE
    assert ln(wsb=lib.ofx_layernorm_bwd_ws(D) - 4) == OFX_EWORKSPACE and b"workspace" in lib.ofx_last_error()

    C = 1024
    xs = f(M, C)

    def cs(x_=xs.data_ptr(), kind=0, ld=C, o0=sums[0].data_ptr(), seg=C, C_=C, valid=0, M_=M, ws_=ws.data_ptr(), wsb=None, dt=1):
        wsb = lib.ofx_colsum_ws(C_) if wsb is None else wsb
        return lib.ofx_colsum(x_, kind, ld, None, None, o0, None, None, seg, C_, valid, M_, None, 0, dt, ws_, wsb, stream())

    for kw in (dict(x_=None), dict(o0=None), dict(ws_=None), dict(kind=2), dict(kind=1, dt=0), dict(x_=xs.data_ptr() + 4), dict(kind=1, x_=xs.data_ptr() + 4),
               dict(ws_=ws.data_ptr() + 8)):
        assert cs(**kw) == OFX_EINVAL, kw
    for kw in (dict(C_=1022, wsb=1 << 30), dict(ld=C - 4), dict(ld=C + 2), dict(M_=0), dict(seg=0), dict(seg=C // 4), dict(valid=C + 1), dict(valid=-1)):
        assert cs(**kw) == OFX_ESHAPE, kw
    assert cs(wsb=lib.ofx_colsum_ws(C) - 4) == OFX_EWORKSPACE

    dl, w = f(M), f(M, D)

    def head(dl_=dl.data_ptr(), w_=w.data_ptr(), dX=dx.data_ptr(), dXb=dxo.data_ptr(), db=sums[0].data_ptr(), B=M, D_=D, p=0.1, dt=1):
        return lib.ofx_head_bwd(dl_, w_, None, dX, dXb, db, B, D_, p, SEED, 1, 2, 0, dt, stream())

    for kw in (dict(w_=None), dict(dX=None), dict(dXb=None), dict(dl_=None), dict(p=1.0), dict(dt=3), dict(w_=w.data_ptr() + 4), dict(dX=dx.data_ptr() + 4),
               dict(dXb=dxo.data_ptr() + 2)):
        assert head(**kw) == OFX_EINVAL, kw                     # dl_=None with db given: the CIR mode has no bias gradient
    for kw in (dict(B=0), dict(D_=0), dict(D_=510)):
        assert head(**kw) == OFX_ESHAPE, kw

    a16 = torch.ones((256, 256), dtype=torch.bfloat16, device="cuda")
    cc = poison32(256, 256)
    outs.append(cc)
    before.append(bits(cc).clone())

    def gt(A=a16.data_ptr(), W=a16.data_ptr(), C_=cc.data_ptr(), bias=None, resid=None, aux=None, N=256, K=256, act=0, p=0.0, slab=None, sb=0, dt=1):
        return lib.ofx_gemm_train(A, W, C_, bias, resid, aux, 256, None, N, K, K, N, N, act, 0, p, SEED, 0, dt, slab, sb, stream())

    for kw in (dict(A=None), dict(W=None), dict(C_=None), dict(p=1.0), dict(act=ACT_MISH_GRAD), dict(bias=dy.data_ptr() + 4), dict(resid=dy.data_ptr() + 8),
               dict(aux=dx.data_ptr() + 4), dict(A=a16.data_ptr() + 2), dict(dt=0)):
        assert gt(**kw) == OFX_EINVAL, kw
    assert gt(N=200) == OFX_ESHAPE and gt(K=72) == OFX_ESHAPE
    try:
        L.check(lib.ofx_tune(2, 1), "tune"); L.check(lib.ofx_tune(5, 2), "tune")
        assert gt(slab=ws.data_ptr(), sb=lib.ofx_gemm_splitk_ws(256, 256, 256) - 4) == OFX_EWORKSPACE
    finally:
        lib.ofx_tune(2, 0); lib.ofx_tune(5, 1)

    def tn(A=a16.data_ptr(), B=a16.data_ptr(), C_=cc.data_ptr(), ldc=256, M_=256, mv=0, nv=0, slab=None, sb=0, dt=1):
        return lib.ofx_gemm_tn_into(A, 256, B, 256, C_, ldc, M_, 256, 256, None, mv, nv, 0, slab, sb, dt, stream())

    for kw in (dict(A=None), dict(B=None), dict(C_=None), dict(mv=-1), dict(nv=-4), dict(A=a16.data_ptr() + 2), dict(C_=cc.data_ptr() + 4), dict(dt=0),
               dict(slab=ws.data_ptr() + 4, sb=1 << 20)):
        assert tn(**kw) == OFX_EINVAL, kw
    for kw in (dict(M_=128), dict(ldc=200), dict(nv=250), dict(mv=300), dict(nv=248, ldc=244)):
        assert tn(**kw) == OFX_ESHAPE, kw
    assert tn(slab=ws.data_ptr(), sb=16) == OFX_EWORKSPACE

    def tc(src=dy.data_ptr(), dst=dxo.data_ptr(), R_=M, C_=D, ldd=M, rd=None, ldr=0, dt=1):
        return lib.ofx_transpose_cast(src, dst, R_, C_, ldd, rd, ldr, dt, stream())

    for kw in (dict(src=None), dict(dst=None), dict(dt=0), dict(src=dy.data_ptr() + 2), dict(dst=dxo.data_ptr() + 1)):
        assert tc(**kw) == OFX_EINVAL, kw
    for kw in (dict(R_=0), dict(C_=0), dict(ldd=M - 1), dict(rd=dxo.data_ptr(), ldr=D - 1)):
        assert tc(**kw) == OFX_ESHAPE, kw
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(bits(o), b), "a refused call wrote something"
