"""oracle/fold_ops.py, the float64 reference of the towers' LayerNorm-fold chain, checked WITHOUT a GPU:
  1. pinned to an independent formulation - torch float64 layer_norm followed by linear equals the folded form
     rstd (x Wf^T - mean col_sum) + bias_f on unrounded operands; every single op against torch float64;
  2. SHARP - on the inputs of every bounded case of tests/test_gpu_fold_ops.py a planted mistake exceeds the bound: a statistic taken from
     the next row, from the next 64-column segment, a sum missing one of its 64 columns, a col_sum taken from unrounded weights, a stale
     (h0, l0);
  3. the exact-lattice cases are exactly representable (fp32 accumulation, every v, every 64-term sum of v and v^2, the (hi, lo) pair);
  4. the one-pass envelope of stats_finalize: the emulated kernel formula sits inside the derived bound, and the project's own fixtures sit
     where c 2^-24 max E[x^2] / Var is a tenth of the 1e-3 budget.
"""
import numpy as np
import pytest
import torch

from oracle import fold_ops as R

U32 = R.U32


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ 1. the pin
def test_folded_form_equals_layernorm_then_linear():
    g = np.random.default_rng(5)
    M, K, N = 37, 192, 128
    x = g.standard_normal((M, K)) * 1.7 + g.standard_normal((M, 1)) * 3
    w, gamma, beta, bias = g.standard_normal((N, K)), g.uniform(0.5, 2, K), g.standard_normal(K), g.standard_normal(N)
    want = torch.nn.functional.linear(torch.nn.functional.layer_norm(t64(x), (K,), t64(gamma), t64(beta), 1e-5), t64(w), t64(bias)).numpy()
    wf = w * gamma[None, :]
    st = R.row_stats_ref(x, 1e-5)
    # row_stats_ref rounds eps to fp32 as the kernels take it; the pin runs at that eps
    e32 = float(np.float32(1e-5))
    want = torch.nn.functional.linear(torch.nn.functional.layer_norm(t64(x), (K,), t64(gamma), t64(beta), e32), t64(w), t64(bias)).numpy()
    got = R.consumer_ref(x, wf, wf.sum(1), st[:, 0], st[:, 1], bias + w @ beta)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the statistics from per-segment partials are the same statistics
    st2 = R.finalize_ref(R.seg_sums(x), K)
    assert np.abs(st2 - st).max() <= 1e-12 * np.abs(st).max()
    # the activation
    z = g.standard_normal(100) * 3
    assert np.allclose(R.quick_gelu(z), (t64(z) * torch.sigmoid(1.702 * t64(z))).numpy(), rtol=1e-14, atol=0)


def test_single_ops_against_torch():
    g = np.random.default_rng(6)
    x = R.stream_rows(9, 512, 1)
    gamma, beta = g.uniform(0.5, 2, 512), g.standard_normal(512)
    e32 = float(np.float32(1e-5))
    want = torch.nn.functional.layer_norm(t64(x), (512,), t64(gamma), t64(beta), e32).numpy()
    assert np.abs(R.ln_ref(x, gamma, beta) - want).max() <= 1e-12 * np.abs(want).max()
    emul = R.ln_emul(x, gamma.astype(np.float32), beta.astype(np.float32))
    assert R.rel_rows(emul, want).max() < 8 * U32
    st, se = R.row_stats_ref(x), R.row_stats_emul(x)
    assert np.abs(st[:, 0] - x.astype(np.float64).mean(1)).max() == 0 and np.abs(se - st).max() <= 8 * U32 * np.abs(st).max()
    # the (hi, lo) split: torch's casts, |lo| <= ulp(hi) / 2, and the pair resolves v to pair_res
    for dt, td in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        hi, lo = R.split_op(x, dt)
        assert np.array_equal(hi, torch.from_numpy(x).to(td).float().numpy())
        assert np.array_equal(lo, (torch.from_numpy(x) - torch.from_numpy(hi)).to(td).float().numpy())
        assert (np.abs(lo) <= R.ulp_op(hi, dt) / 2).all()
        assert (np.abs(hi.astype(np.float64) + lo - x) <= R.pair_res(x, dt)).all()
        # fold_pack: hi / lo expectations are torch casts of fp32(w gamma)
        w = g.standard_normal((5, 512)).astype(np.float32)
        fp = R.fold_pack_ref(w, gamma.astype(np.float32), beta.astype(np.float32), np.ones(5, np.float32), dt, 1)
        wg = torch.from_numpy(w) * torch.from_numpy(gamma.astype(np.float32))
        assert np.array_equal(fp["hi"], wg.to(td).float().numpy()) and np.array_equal(fp["lo"], (wg - wg.to(td).float()).to(td).float().numpy())
        assert np.allclose(fp["bias_terms"].sum(0), 1.0 + w.astype(np.float64) @ beta.astype(np.float32).astype(np.float64), rtol=1e-13)
    # embed_rows: the CLS row and per-position pos
    po, cls, pos = g.standard_normal((2 * 3, 8)), g.standard_normal(8), g.standard_normal((4, 8))
    rows = R.embed_rows(po, cls, pos, 2, 4)
    assert np.array_equal(rows[4], cls + pos[0]) and np.array_equal(rows[6], po[4] + pos[2])


# ------------------------------------------------------------------------------------------------ 2. sharpness, 3. exact lattice
PRODUCER_SHARP = [(17, 256, 128, "bf16", 0), (257, 768, 128, "f16", 0), (600, 768, 768, "f16", 1), (65, 256, 128, "bf16", 1)]


@pytest.mark.parametrize("M,N,K,dt,form", PRODUCER_SHARP)
def test_producer_random_case_is_sharp(M, N, K, dt, form):
    c = R.producer_random(M, N, K, dt, form)
    kk = 2 * K if form else K
    v, mag = R.producer_ref(c["a"], c["w"], c["bias"], c["h0"], c["l0"], w_lo=c["w_lo"])
    vb = R.value_bound(mag, kk, v, dt)
    # a stale (h0, l0): the pair of a row 1, 8 or 16 further on (another slot of the prefetch ring, another half-pass)
    for d in (1, 8, 16):
        if M > d:
            stale, _ = R.producer_ref(c["a"], c["w"], c["bias"], np.roll(c["h0"], -d, 0), np.roll(c["l0"], -d, 0), w_lo=c["w_lo"])
            assert ((np.abs(stale - v) > vb).mean(1) > 0.9).all(), d
    # a stale lo alone, the smaller half (2^-9 / 2^-12 of v): above the accumulation allowance at K = 128; at the bench's K it is the
    # exact-lattice case that catches it
    if M > 1 and kk <= 256:
        stale, _ = R.producer_ref(c["a"], c["w"], c["bias"], c["h0"], np.roll(c["l0"], -1, 0), w_lo=c["w_lo"])
        assert ((np.abs(stale - v) > vb).mean(1) > 0.5).all()
    hi, lo = R.split_op(v.astype(np.float32), dt)
    t = hi.astype(np.float64) + lo
    part, pb = R.seg_sums(t), R.part_bound(t, dt)
    if M > 1:       # a statistic taken from the next row
        assert (np.abs(np.roll(part, -1, 0) - part) > pb).all()
    assert (np.abs(np.roll(part, -1, 1) - part) > pb).all()                                       # ... from the next segment
    # a sum missing one of its 64 columns: for every column position, the dropped term exceeds the bound in most (row, segment)s
    a = np.abs(t).reshape(M, -1, R.SEG)
    assert ((a > pb[..., 0:1]).mean((0, 1)) > 0.8).all() and ((a * a > pb[..., 1:2]).mean((0, 1)) > 0.8).all()
    # and the bound leaves room for correct fp32 arithmetic: the pair itself is inside value_bound
    assert (np.abs(t - v) <= vb).all()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("M,N,K", [(17, 256, 128), (600, 768, 768), (129, 256, 128)])
def test_lattice_cases_are_exact(M, N, K, form, dt):
    c = R.producer_lattice(M, N, K, dt, form)
    assert R.lattice_is_exact(c, dt)
    v, _ = R.producer_ref(c["a"], c["w"], c["bias"], c["h0"], c["l0"], w_lo=c["w_lo"])
    # the fp32 accumulation in two very different orders gives the float64 result
    a32, w32 = c["a"], c["w"] if not form else np.concatenate([c["w"], c["w_lo"]], 1)
    aa = a32 if not form else np.concatenate([a32, a32], 1)
    acc = np.zeros((M, N), np.float32)
    for k in range(aa.shape[1] - 1, -1, -1):
        acc += aa[:, k:k + 1] * w32[None, :, k]
    v32 = ((acc + c["bias"][None, :]) + (c["h0"] + c["l0"])).astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)
    # and it is sharp in the strictest sense: neighbouring rows and segments differ, so does a stale pair
    part = R.seg_sums(v)
    assert (np.roll(part, -1, 1) != part).any(-1).all() and (M == 1 or (np.roll(part, -1, 0) != part).any(-1).all())
    assert (v != 0).mean() > 0.9


@pytest.mark.parametrize("route", list(R.ROUTES))
def test_every_lattice_case_of_the_gpu_test_is_exact(route):
    _, _, form = R.ROUTES[route]
    for dt in (("f16",) if form == 2 else ("bf16", "f16")):
        for (M, N, K) in R.producer_shapes(route):
            assert R.lattice_is_exact(R.producer_lattice(M, N, K, dt, form), dt), (M, N, K, dt)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,N,K", R.CONSUMER_SHAPES)
def test_consumer_case_is_sharp(M, N, K, act, dt):
    """against the LARGEST allowance the GPU test grants an element: 1e-3 of the largest output in f16, 2^-9 + (1e-3 - 2^-11) in bf16"""
    c = R.consumer_case(M, N, K, dt, 0, act)
    ref = R.consumer_ref(c["a"], c["w"], c["col_sum"], c["mean"], c["rstd"], c["bias"], act)
    scale = np.abs(ref).max() * (1.0 if dt == "f16" else (2.0 ** -9 + 1e-3 - 2.0 ** -11) / 1e-3)

    def off(**kw):
        d = dict(c); d.update(kw)
        return np.abs(R.consumer_ref(d["a"], d["w"], d["col_sum"], d["mean"], d["rstd"], d["bias"], act) - ref) / scale

    if M > 1:       # the statistics of the next row: every row moves beyond the bound
        assert (off(mean=np.roll(c["mean"], -1)).max(1) > R.CONSUMER_BOUND).all()
        assert (off(rstd=np.roll(c["rstd"], -1)).max(1) > R.CONSUMER_BOUND).mean() > 0.95
    # the constants of the next 4-column group (one lane over), and of the next tile
    # (QuickGELU flattens the columns whose z is far below 0: with one row a quarter of the columns cannot show a wrong constant)
    most = 0.9 if act == 0 or M > 1 else 0.6
    for d in (4, 64, 128):
        assert (off(bias=np.roll(c["bias"], -d)).max(0) > R.CONSUMER_BOUND).mean() > most
        assert (off(col_sum=np.roll(c["col_sum"], -d)).max(0) > R.CONSUMER_BOUND).mean() > most


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("N,K", [(5, 512), (768, 768)])
def test_fold_pack_col_sum_of_unrounded_weights_shows(N, K, dt):
    g = np.random.default_rng(N + K)
    w = (g.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    gamma = g.uniform(0.5, 2, K).astype(np.float32)
    fp = R.fold_pack_ref(w, gamma, np.zeros(K, np.float32), np.zeros(N, np.float32), dt, 0)
    terms = fp["hi"].astype(np.float64).T
    bound = R.sum_bound(terms, R.fold_pack_h(K, 0))
    unrounded = (w.astype(np.float64) * gamma).sum(1)
    assert (np.abs(unrounded - terms.sum(0)) > bound).mean() > 0.6          # the sum of 2^-9 / 2^-12 roundings against (h + 3) 2^-24 sum |w|
    # one column dropped from the sum
    assert (np.abs(terms) > bound[None, :]).mean() > 0.9
    # under split the pair resolves the weights to 2^-16 / 2^-22 and the two sums agree to less than the bound: there the mistake is
    # smaller than correct fp32 arithmetic and no test can or need see it
    fp2 = R.fold_pack_ref(w, gamma, np.zeros(K, np.float32), np.zeros(N, np.float32), dt, 1)
    t2 = np.concatenate([fp2["hi"], fp2["lo"]], 1).astype(np.float64).T
    assert (np.abs(unrounded - t2.sum(0)) <= R.sum_bound(t2, R.fold_pack_h(K, 1))).all()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_chain_case_shows_a_col_sum_of_unrounded_weights(dt):
    """The chain case (row_stats_cast -> fold_pack -> gemm_fold), single-product weights: with col_sum taken from the unrounded w gamma the
    rows of mean / std = 16 move by more than the consumer's bound (a sum of K roundings of 2^-9 or 2^-12, times 16): 1.5e-2 of the
    largest output in bf16, 2.2e-3 in f16."""
    c = R.chain_case(dt, 0)
    hi, _ = R.split_op(c["x"], dt)
    st = R.row_stats_ref(c["x"])
    fp = R.fold_pack_ref(c["w"], c["gamma"], c["beta"], c["bias"], dt, 0)
    bias_f = fp["bias_terms"].sum(0)
    ref = R.consumer_ref(hi, fp["hi"], fp["hi"].astype(np.float64).sum(1), st[:, 0], st[:, 1], bias_f)
    bad = R.consumer_ref(hi, fp["hi"], (c["w"].astype(np.float64) * c["gamma"]).sum(1), st[:, 0], st[:, 1], bias_f)
    moved = np.abs(bad - ref).max() / np.abs(ref).max()
    print(f"chain {dt}: col_sum of unrounded weights moves the output by {moved:.2e} of its maximum")
    assert moved > R.CONSUMER_BOUND
    # and the folded form on the rounded operands is LayerNorm + Linear of the hi rows with the full rows' statistics
    xn = (hi.astype(np.float64) - st[:, :1]) * st[:, 1:]
    want = xn @ fp["hi"].astype(np.float64).T + bias_f[None, :]
    assert np.abs(ref - want).max() <= 1e-10 * np.abs(want).max()


def test_finalize_emulation_sits_inside_the_derived_bound():
    """The np.float32 emulation of the kernel's formula against float64 on the partials it is fed: inside c 2^-24 cond + 3 2^-24 for every
    case of the GPU test, with c = (3 slots + 1) / 2 <= 32; and a statistic of the next row exceeds the bound."""
    worst = 0.0
    for slots in R.FINALIZE_SLOTS:
        assert R.finalize_c(slots) <= 32
        for ratio in R.FINALIZE_RATIOS:
            x = R.finalize_rows(257, slots, ratio)
            part = R.seg_sums(x).astype(np.float32)
            ref, em = R.finalize_ref(part, slots * 64), R.finalize_emul(part, slots * 64)
            bound = R.finalize_bound(R.cond_of(x), slots)
            e = np.abs(em[:, 1] - ref[:, 1]) / ref[:, 1]
            worst = max(worst, float((e / bound).max()))
            assert (e <= bound).all(), (slots, ratio, (e / bound).max())
            assert (np.abs(em[:, 0] - ref[:, 0]) <= (slots + 1) * U32 * np.abs(part[..., 0]).sum(-1) / (slots * 64)).all()
            nxt = np.abs(np.roll(ref[:, 1], -1) - ref[:, 1]) / ref[:, 1]
            assert (nxt > bound).mean() > (0.9 if ratio <= 16 else 0.5), (slots, ratio)
    print(f"finalize emulation: worst err / bound = {worst:.3f}")
    # constant rows: variance 0, the clamp; exact mean
    part = np.zeros((4, 12, 2), np.float32)
    for r, cval in enumerate((0.0, 3.0, -0.625, 100.5)):
        part[r, :, 0], part[r, :, 1] = 64 * cval, 64 * cval * cval
    em = R.finalize_emul(part, 768)
    assert np.array_equal(em[:, 0], np.array([0.0, 3.0, -0.625, 100.5], np.float32)) and (em[:, 1] <= (1 + 3 * U32) / np.sqrt(np.float64(np.float32(1e-5)))).all()


# ------------------------------------------------------------------------------------------------ 4. the fixtures' envelope
_COND = {}


def fixture_cond(key, seed):
    if key not in _COND:
        from oracle import np_oracle as O
        from outfitx_amd import synth
        W = {k[len(synth.IMG_PREFIX):]: v for k, v in synth.variant_state_dict(key).items() if k.startswith(synth.IMG_PREFIX)}
        px = synth.smooth_pixel_values(seed, 2)
        worst, emb = R.vit_stream_cond(px, W)
        want = O.vit_forward(px, W, dt=np.float64)
        assert np.abs(emb - want).max() <= 1e-9 * np.abs(want).max(), "the tapped forward is np_oracle's"
        _COND[key] = worst
    return _COND[key]


@pytest.mark.parametrize("key,seed", [("3", 11), ("3o3", 12)])
def test_fixture_streams_sit_inside_a_tenth_of_the_budget(key, seed):
    """max E[x^2] / Var over the rows that feed stats_finalize (the stream after out-proj and after fc2, every layer), on smooth images,
    plain and level-3 outlier weights: c 2^-24 max cond < 1e-4 with c = 18.5 (W = 768: 12 slots).  Measured: see the print."""
    cond = fixture_cond(key, seed)
    c = R.finalize_c(768 // 64)
    print(f"fixture {key}: max E[x^2] / Var = {cond:.3f}; c 2^-24 cond = {c * U32 * cond:.3e}")
    assert c * U32 * cond < 1e-4
