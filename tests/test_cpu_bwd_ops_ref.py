"""CPU-only: oracle/bwd_ops.py, the float64 reference of tests/test_gpu_bwd_ops.py, against float64 torch autograd (<= 1e-12 relative),
and - from the references alone - the input conditions the GPU file relies on: every sum case is SHARP (each live row owns a stored
column where its term exceeds 16 x that column's error bound (h + 3) 2^-24 sum |terms|, so a dropped or doubled row cannot hide), and
the mish' sweep reaches the points it names."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import bwd_ops as R


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("D,add_kind,p", [(512, "none", 0.0), (768, "full", 0.1), (1024, "map", 0.3)])
def test_layernorm_backward_matches_autograd(D, add_kind, p):
    """y = layer_norm(x) with statistics of the same float64 x; upstream dy; the addend and the dropped copy are linear extras."""
    g = np.random.default_rng(D)
    M, eps = 37, 1e-5
    x = 3.0 * g.standard_normal((M, D)) + 1.5
    x[::5] += 100.0
    dy, gamma, beta = g.standard_normal((M, D)), 1.0 + 0.25 * g.standard_normal(D), g.standard_normal(D)
    add = add_map = None
    if add_kind == "full":
        add = g.standard_normal((M, D))
    elif add_kind == "map":
        add, add_map = g.standard_normal((4, D)), np.full(M, -1)
        add_map[[30, 2, 17, 9]] = np.arange(4)
    mask = R.drop_mask(p, 5, 3, M, D)
    xt, gt, bt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, gamma, beta))
    (F.layer_norm(xt, (D,), gt, bt, eps) * torch.tensor(dy)).sum().backward()
    mean, rstd = x.mean(-1), 1.0 / np.sqrt(x.var(-1) + eps)
    r = R.ln_bwd_ref(dy, x, mean, rstd, gamma, add, add_map, mask)
    extra = 0.0 if add is None else R.gathered_add(add, add_map, M)
    assert rel(r["dx"], xt.grad.numpy() + extra) <= 1e-12
    assert rel(r["dgamma"], gt.grad.numpy()) <= 1e-12 and rel(r["dbeta"], bt.grad.numpy()) <= 1e-12
    assert rel(r["dx_drop"], (xt.grad.numpy() + extra) * mask) <= 1e-12 and rel(r["dcols"], ((xt.grad.numpy() + extra) * mask).sum(0)) <= 1e-12
    if add_kind == "map":
        assert not extra[add_map < 0].any() and np.array_equal(extra[30], add[0])
    # the fp32 emulation is the same function: it agrees with float64 to fp32 accuracy, row by row
    e = R.ln_bwd_dx_emul(*(a.astype(np.float32) for a in (dy, x, mean, rstd, gamma)), None if add is None else add.astype(np.float32), add_map)
    r32 = R.ln_bwd_ref(*(a.astype(np.float32) for a in (dy, x, mean, rstd, gamma)), None if add is None else add.astype(np.float32), add_map)
    err = np.linalg.norm(e - r32["dx"], axis=1) / np.linalg.norm(r32["dx"], axis=1)
    assert e.dtype == np.float32 and err.max() < 64 * R.U32 and err.max() > 0


def test_mish_grad_matches_autograd():
    u = np.concatenate([np.linspace(-30, 30, 4001), [0.0, 1e-30, -1e-30, 19.0, 20.0, -1.1924, 88.0, -88.0]])
    ut = torch.tensor(u, dtype=torch.float64, requires_grad=True)
    F.mish(ut).sum().backward()
    ref = ut.grad.numpy()
    got = R.mish_grad(u)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert abs(R.mish_grad(0.0) - 0.6) < 1e-15 and R.mish_grad(400.0) == 1.0 and R.mish_grad(-400.0) == 0.0
    assert rel(R.mish(u), F.mish(ut).detach().numpy()) <= 1e-12


@pytest.mark.parametrize("mode", ["cp", "cir"])
def test_head_backward_matches_autograd(mode):
    g = np.random.default_rng(11)
    B, D = 9, 24
    row0 = torch.tensor(g.standard_normal((B, D)), requires_grad=True)
    m = R.drop_mask(0.3, 9, 2, B, D)
    up = g.standard_normal(B if mode == "cp" else (B, D))
    if mode == "cp":
        w, b = torch.tensor(g.standard_normal(D), requires_grad=True), torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
        (((row0 * torch.tensor(m, dtype=torch.float64)) @ w + b) * torch.tensor(up)).sum().backward()
        d_row0, d_b = R.head_bwd_ref(up, w.detach().numpy(), m)
        assert rel(d_b, b.grad.numpy()) <= 1e-12
    else:       # the CIR head hands over ready row gradients of the dropped-out rows
        ((row0 * torch.tensor(m, dtype=torch.float64)) * torch.tensor(up)).sum().backward()
        d_row0, d_b = R.head_bwd_ref(None, up, m)
        assert d_b is None
    assert rel(d_row0, row0.grad.numpy()) <= 1e-12


def test_drop_mask_values_and_rate():
    m = R.drop_mask(0.1, R.SEED, 7, 300, 1024)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))
    assert m.dtype == np.float32 and set(np.unique(m)) == {np.float32(0.0), keep}
    assert abs((m == 0).mean() - 0.1) < 0.005
    assert np.array_equal(R.drop_mask(0.1, R.SEED, 7, np.array([5, 299]), 1024), m[[5, 299]])       # rows by index
    assert not np.array_equal(m, R.drop_mask(0.1, R.SEED, 8, 300, 1024)) and (R.drop_mask(0.0, 1, 1, 3, 8) == 1).all()


def test_colsum_reference():
    g = np.random.default_rng(3)
    x, gi, sc = g.standard_normal((20, 12)), g.permutation(20)[:7], g.standard_normal(7)
    s, t = R.colsum_ref(x, gi, sc)
    want = (torch.tensor(x)[torch.tensor(gi)] * torch.tensor(sc)[:, None]).sum(0).numpy()
    assert rel(s, want) <= 1e-12 and t.shape == (7, 12) and rel(t.sum(0), s) <= 1e-15


# ---- the conditions the GPU file relies on
def test_mish_sweep_reaches_its_points():
    u = R.mish_sweep()
    f = np.float32
    assert u.shape == (256, 256) and u.dtype == f and np.isfinite(u).all()
    flat = set(u.ravel().tolist())
    for v in (0.0, 1e-30, -1e-30, 88.0, -88.0, 19.0, 20.0, -30.0, 30.0):
        assert float(f(v)) in flat, v
    for v in (19.0, 20.0, R.mish_grad_zero()):
        assert float(np.nextafter(f(v), f(np.inf))) in flat and float(np.nextafter(f(v), f(-np.inf))) in flat, v
    z = R.mish_grad_zero()
    assert abs(z + 1.1924) < 1e-4 and abs(R.mish_grad(z)) < 1e-15
    dense = np.sort(u.ravel()[:65000])
    assert np.diff(dense).max() < 1e-3                      # [-30, 30] at a spacing of 9.2e-4
    fp32_formula_err = np.abs(R.mish_grad(u.astype(np.float64))).max()
    assert 1.0 < fp32_formula_err < 1.1                     # mish' peaks at 1.0888: absolute and relative error agree to 9 %


# ---- sharpness
@pytest.mark.parametrize("i", range(len(R.LN_CASES)))
def test_layernorm_cases_are_sharp(i):
    case = R.LN_CASES[i]
    n, h = R.ln_live(case), R.ln_h(case)
    inp, ref = R.ln_inputs(i), R.ln_reference(i)
    assert inp["stats"].shape == (n, 2) and ref["dx"].shape == (n, case[0])
    assert h == -(-n // 1024) + 27
    if n:
        a = np.abs(inp["dy"])
        assert a.min() >= 0.5 and a.max() < 2.0
        assert np.abs(inp["x"][::7].mean(-1)).min() > 90                 # the shifted rows
    names = ["dgamma", "dbeta"] + (["dcols"] if case[6] else [])
    for name in names:
        t = ref["t_" + name]
        assert R.sharp(t, R.sum_bound(t, h + 1)), name                   # + 1: also under the accumulate addition
    if case[4] == "map" and n:
        assert (inp["add_map"] >= 0).sum() == min(n, 9) and sorted(inp["add_map"][inp["add_map"] >= 0]) == list(range(min(n, 9)))
        live = np.nonzero(inp["add_map"] >= 0)[0]
        assert n < 9 or not np.array_equal(inp["add_map"][live], np.arange(9))       # scattered AND out of order


@pytest.mark.parametrize("i", range(len(R.CS_CASES)))
def test_colsum_cases_are_sharp(i):
    case = R.CS_CASES[i]
    kind, C, ld, M, live, gather, scale, outs, valid, acc = case
    n, h = R.cs_live(case), R.cs_h(case)
    nchunk, per = R.cs_plan(case)
    assert nchunk == min(max(M // 16, 1), 256) and (n == 0 or (per - 1) * nchunk < n <= per * nchunk)
    s, t = R.cs_reference(i)
    assert t.shape == (n, C) and C % len(outs) == 0
    seg = C // len(outs)
    stored = np.zeros(C, bool)
    for k, on in enumerate(outs):
        if on:
            stored[k * seg:k * seg + (valid or seg)] = True
    assert stored.any()
    b = R.sum_bound(t, h + 1)
    assert R.sharp(t[:, stored], b[stored])
    inp = R.cs_inputs(i)
    if gather:
        gi = inp["gather"]
        assert len(np.unique(gi)) == n and (np.diff(gi) < 0).any() and inp["table"].shape[0] > n


@pytest.mark.parametrize("i", range(len(R.HEAD_CASES)))
def test_head_cases_are_sharp(i):
    mode, B, D, cu, hs, bs, acc, alias, dt = R.HEAD_CASES[i]
    inp = R.head_inputs(i)
    if mode == "cp":
        t = inp["dlogits"].astype(np.float64)[:, None]
        assert R.sharp(t, R.sum_bound(t, R.head_h(B) + 1))
    if cu:
        c = inp["cu"]
        assert (np.diff(c) >= 2).all() and (c != np.arange(B)).all() and c[-1] < inp["rows"]
    assert not alias or (mode == "cir" and not cu)
