"""Dynamic loss scaling fused into the AdamW boundary (ofx_adamw_step_scaled, outfitx_amd/csrc/optim.hip), optim.FlatAdamW(loss_scaling=True)
and the trainers' `loss_scaling` on the HIP optimizer.

References: the plain call ofx_adamw_step itself (bit identity, derived below), tests/loss_scale_ref.py (the float64 restatement of
unscale_ + clip + AdamW + GradScaler.update, held to torch on the CPU by tests/test_cpu_loss_scale.py) under the bounds of
tests/test_gpu_flat_adamw.py, and torch.amp.GradScaler('cpu') for the (scale, tracker) trajectory.

Bit identity is derived, not measured: for a power of two S, (g S) * (grad_scale / S) and g * grad_scale are the same real number -
g S is exact in fp32, and so is the fp32 factor grad_scale * (float)(1 / S) - so both round to the same float, and everything after that
first product is the same arithmetic in both calls.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import flat_adamw_ref as R
import loss_scale_ref as S
import test_gpu_flat_adamw as T
from conftest import golden
from outfitx_amd import synth

warnings.simplefilter("ignore")
pytestmark = pytest.mark.gpu
OFX_EINVAL, OFX_ESHAPE, OFX_EWORKSPACE = -1, -2, -4
cu = T.cu


def bits(t):
    return t.view(torch.int32)


class ScaledArena(T.Arena):
    """tests/test_gpu_flat_adamw.py's arena (sentinel-guarded parameters, the three arenas, the call's scalars) + the scaler's state."""

    def __init__(self, sizes, p0, scale=S.INIT_SCALE, tracker=0, growth=S.GROWTH, backoff=S.BACKOFF, interval=S.INTERVAL):
        super().__init__(sizes, p0)
        self.scale = torch.full((), float(scale), device="cuda")
        self.tracker = torch.full((), int(tracker), dtype=torch.int32, device="cuda")
        self.growth, self.backoff, self.interval = growth, backoff, interval

    def call_scaled(self, lr, beta1, grad_scale=1.0):
        from outfitx_amd.engine import adamw_step_scaled
        adamw_step_scaled(self.seg, self.grad, self.m, self.v, self.step, lr, beta1, R.BETA2, R.EPS, R.WD, R.MAX_NORM, grad_scale, self.scale,
                          self.tracker, self.growth, self.backoff, self.interval, self.norm, self.skipped, self.ws)

    def state(self):
        """Every output of a call, as bit patterns."""
        return [bits(t).clone() for t in (self.buf, self.m, self.v, self.step.reshape(1), self.norm.reshape(1), self.grad)] + [self.skipped.clone()]


# ------------------------------------------------------------------------------------------------ 1. bit identity
@functools.lru_cache(maxsize=None)
def plain_schedule(seed, grad_scale):
    """The four-step schedule through the PLAIN call -> per-step states (computed once per seed and grad_scale)."""
    T.need_gpu()
    p0, grads = R.make_problem(seed)
    A = T.Arena(R.SIZES, p0)
    out = []
    for k, (lr, b1, _) in enumerate(R.SCHEDULE):
        A.set_grad(grads[k])
        A.call(lr, b1, grad_scale=grad_scale)
        out.append([bits(t).clone() for t in (A.buf, A.m, A.v, A.step.reshape(1), A.norm.reshape(1), A.grad)] + [A.skipped.clone()])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -3, 2.0 ** 16, 2.0 ** 24])
def test_scaled_call_on_a_scaled_arena_returns_the_plain_calls_bits(scale, grad_scale, seed):
    """1. ofx_adamw_step_scaled on S x G with *loss_scale = S against ofx_adamw_step on G, every step of the schedule: parameters (and
    the sentinels around them), both moments, *step, *grad_norm and *skipped bit for bit, and an all-zero arena."""
    want = plain_schedule(seed, grad_scale)
    p0, grads = R.make_problem(seed)
    A = ScaledArena(R.SIZES, p0, scale=scale)
    for k, (lr, b1, _) in enumerate(R.SCHEDULE):
        gs = grads[k] * np.float32(scale)
        assert np.isfinite(gs).all() and np.array_equal(gs / np.float32(scale), grads[k])          # S x G is exact in fp32
        A.set_grad(gs)
        A.call_scaled(lr, b1, grad_scale=grad_scale)
        got = A.state()
        for name, x, y in zip(("p", "m", "v", "step", "grad_norm", "arena", "skipped"), got, want[k]):
            assert torch.equal(x, y), (k, name, int((x != y).sum()))
        assert int((got[5] != 0).sum()) == 0 and int(A.skipped) == 0 and float(A.step) == k + 1
    assert float(A.scale) == scale and int(A.tracker) == len(R.SCHEDULE)


# ------------------------------------------------------------------------------------------------ 2. non-finite gradients
OFF_4097 = 64 + 64 + 64 + 1024                 # arena offset of the 4097-element tensor (sizes 1, 5, 64, 1000 before it)
POSITIONS = {"first float": 0, "last float": -1, "padding gap": 70, "straddling float4, live": OFF_4097 + 4096, "straddling float4, padding": OFF_4097 + 4098}


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("where", sorted(POSITIONS))
def test_a_non_finite_arena_element_skips_the_step_and_backs_the_scale_off(where, bad):
    """2. One non-finite float anywhere in the arena - live, padding, or in the float4 that straddles the end of a tensor whose numel is
    no multiple of 4: p, m, v, *step bit-identical, arena zero, *skipped = 1, scale x backoff, tracker 0."""
    T.need_gpu()
    p0, grads = R.make_problem(1)
    lr, b1, _ = R.SCHEDULE[2]
    A = ScaledArena(R.SIZES, p0, scale=1024.0, tracker=2, backoff=0.25)
    assert A.offsets[4] == OFF_4097 and A.sizes[4] == 4097 and bool(A.pad[70]) and bool(A.pad[OFF_4097 + 4098]) and not bool(A.pad[OFF_4097 + 4096])
    assert not bool(A.pad[0]) and not bool(A.pad[A.n - 1])
    g = np.random.default_rng(5)
    A.m[A.idx] = cu((g.standard_normal(len(p0)) * 0.1).astype(np.float32))          # non-trivial moments, so "untouched" says something
    A.v[A.idx] = cu((g.random(len(p0)) * 0.01).astype(np.float32))
    A.step.fill_(3.0)
    A.set_grad(grads[2] * np.float32(1024.0))
    A.grad[POSITIONS[where]] = bad
    before = [t.clone() for t in (A.buf, A.m, A.v, A.step)]
    A.call_scaled(lr, b1)
    torch.cuda.synchronize()
    assert int(A.skipped) == 1 and not np.isfinite(float(A.norm))
    for x, y in zip(before, (A.buf, A.m, A.v, A.step)):
        assert torch.equal(bits(x), bits(y))
    assert int((bits(A.grad) != 0).sum()) == 0
    assert float(A.scale) == 256.0 and int(A.tracker) == 0


def test_scaled_gradients_whose_fp32_squares_overflow_are_not_skipped():
    """2b. Arena elements around 1e30 under a scale of 65536: squared in fp32 they (and the unscaled 1.5e25 too) would be inf; the norm is
    taken in double, is finite, and the step runs and meets the restatement."""
    T.need_gpu()
    p0, grads = R.make_problem(2, scales=[1e30])
    lr, b1, _ = R.SCHEDULE[2]
    with np.errstate(over="ignore"):
        assert np.isfinite(grads[0]).all() and np.isinf((grads[0] / np.float32(65536.0)) ** 2).any()
    A = ScaledArena(R.SIZES, p0)
    A.set_grad(grads[0])
    rec = {"p_in": A.p(), "m_in": A.live(A.m), "v_in": A.live(A.v), "g_in": grads[0], "t_old": 0, "lr": lr, "beta1": b1, "grad_scale": 1.0 / 65536.0}
    A.call_scaled(lr, b1)
    torch.cuda.synchronize()
    assert int(A.skipped) == 0 and np.isfinite(float(A.norm)) and float(A.step) == 1 and int(A.tracker) == 1 and float(A.scale) == 65536.0
    rec.update(p=A.p(), m=A.live(A.m), v=A.live(A.v), norm=float(A.norm))
    T.check_step("1e30 gradients", rec, *T.bounds_of(R.standard_bounds()))
    assert A.side_effects() == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ 3. trajectory
INFS = [False, True, False, False, False, True, False]        # infs on calls 2 and 6; growth_interval 3: the scale grows on call 5


def test_seven_calls_follow_the_cpu_grad_scaler_and_the_restatement():
    """3. Every call's arena is G_t x the scale TENSOR, formed on the device.  (scale, tracker, skipped) after every call are the CPU
    GradScaler's; every step that ran meets the restatement of that step (from the kernel's own inputs) under the bounds of
    tests/test_gpu_flat_adamw.py for inputs off the schedule."""
    T.need_gpu()
    scales = [1.0, 0.01, 50.0, 0.001, 1.0, 0.01, 0.001]
    p0, grads = R.make_problem(0, steps=7, scales=scales)
    want = S.torch_scaler_trajectory(INFS, interval=3)
    assert [s for s, _ in want] == [65536.0, 32768.0, 32768.0, 32768.0, 65536.0, 32768.0, 32768.0] and [t for _, t in want] == [1, 0, 1, 2, 0, 0, 1]
    bound, norm_tol = T.bounds_of(R.standard_bounds())
    A = ScaledArena(R.SIZES, p0, interval=3)
    t_old = 0
    for k, inf in enumerate(INFS):
        lr, b1, _ = R.SCHEDULE[k % 4]
        g = grads[k].copy()
        if inf:
            g[12345] = np.inf
        A.grad.zero_()
        A.grad[A.idx] = cu(g) * A.scale
        scale_in, tracker_in = float(A.scale), int(A.tracker)
        rec = {"p_in": A.p(), "m_in": A.live(A.m), "v_in": A.live(A.v), "g_in": A.live(A.grad), "t_old": t_old, "lr": lr, "beta1": b1}
        A.call_scaled(lr, b1)
        torch.cuda.synchronize()
        assert (float(A.scale), int(A.tracker), int(A.skipped)) == (*want[k], int(inf)), (k, float(A.scale), int(A.tracker), int(A.skipped))
        r = S.ref_step_scaled(rec["p_in"], rec["m_in"], rec["v_in"], rec["g_in"], t_old, lr, b1, scale_in, tracker_in, norm=float(A.norm), interval=3)
        assert (r["scale"], r["tracker"], r["skipped"]) == (*want[k], int(inf))
        assert A.side_effects() == (0, 0, 0)
        if inf:
            assert np.array_equal(A.p(), rec["p_in"]) and np.array_equal(A.live(A.m), rec["m_in"]) and float(A.step) == t_old
            continue
        t_old += 1
        rec.update(p=A.p(), m=A.live(A.m), v=A.live(A.v), norm=float(A.norm), grad_scale=1.0 / scale_in)
        T.check_step(f"call {k + 1}, scale {scale_in:g}", rec, bound, norm_tol)
        assert float(A.step) == t_old


# ------------------------------------------------------------------------------------------------ 4. capture
def test_a_captured_scaled_step_replays_to_the_eager_sequences_bits():
    """4. One single-stream graph of the call, replayed three times with a fresh arena before each (an inf in the second): parameters,
    moments, step, norm, skipped, scale and tracker equal the eager sequence bit for bit after every replay."""
    T.need_gpu()
    p0, grads = R.make_problem(1)
    lr, b1, _ = R.SCHEDULE[2]
    fills = []
    for k in range(3):
        g = grads[k].copy()
        if k == 1:
            g[777] = np.inf
        fills.append(cu(g))

    def run(step_fn, A):
        out = []
        for k in range(3):
            A.grad.zero_()
            A.grad[A.idx] = fills[k] * A.scale
            step_fn()
            torch.cuda.synchronize()
            out.append(A.state() + [bits(A.scale.reshape(1)).clone(), A.tracker.clone()])
        return out

    E = ScaledArena(R.SIZES, p0, interval=2)
    eager = run(lambda: E.call_scaled(lr, b1), E)
    assert [int(s[6]) for s in eager] == [0, 1, 0] and float(E.scale) == 32768.0 and int(E.tracker) == 1
    G = ScaledArena(R.SIZES, p0, interval=2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        G.call_scaled(lr, b1)
    torch.cuda.synchronize()
    assert float(G.step) == 0 and float(G.scale) == 65536.0                       # capturing ran nothing
    replayed = run(graph.replay, G)
    for k in range(3):
        for i, (x, y) in enumerate(zip(replayed[k], eager[k])):
            assert torch.equal(x, y), (k, i)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_scaled_refusals_launch_nothing():
    """5. What ofx_adamw_step refuses, and: NULL or misaligned loss_scale / growth_tracker, growth_factor < 1, backoff_factor outside
    (0, 1], growth_interval < 1 -> OFX_EINVAL; every buffer, the scale and the tracker bit-identical after each."""
    T.need_gpu()
    from outfitx_amd import _lib as L
    lib = L.load()
    p0, grads = R.make_problem(2)
    A = ScaledArena(R.SIZES, p0, tracker=5)
    A.set_grad(grads[2])
    watched = lambda: (A.buf, A.m, A.v, A.step, A.grad, A.scale, A.tracker, A.norm, A.skipped)
    before = [t.clone() for t in watched()]
    pair = torch.zeros(4, device="cuda")                                           # for a misaligned (odd-byte) address
    good = {"segments": A.seg.data_ptr(), "n_segments": len(R.SIZES), "grad": A.grad.data_ptr(), "exp_avg": A.m.data_ptr(), "exp_avg_sq": A.v.data_ptr(),
            "n_arena": A.n, "step": A.step.data_ptr(), "loss_scale": A.scale.data_ptr(), "growth_tracker": A.tracker.data_ptr(), "growth_factor": 2.0,
            "backoff_factor": 0.5, "growth_interval": 2000, "grad_norm": A.norm.data_ptr(), "skipped": A.skipped.data_ptr(), "ws": A.ws.data_ptr(),
            "ws_bytes": lib.ofx_adamw_step_ws_bytes(A.n)}

    def call(**over):
        a = dict(good, **over)
        rc = lib.ofx_adamw_step_scaled(a["segments"], a["n_segments"], a["grad"], a["exp_avg"], a["exp_avg_sq"], a["n_arena"], a["step"], 2e-5, 0.9, 0.999,
                                       1e-8, 0.01, 1.0, 1.0, a["loss_scale"], a["growth_tracker"], a["growth_factor"], a["backoff_factor"],
                                       a["growth_interval"], a["grad_norm"], a["skipped"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for x, y in zip(before, watched()):
            assert torch.equal(bits(x), bits(y)), over
        return rc

    for name in ("segments", "grad", "exp_avg", "exp_avg_sq", "step", "grad_norm", "skipped", "ws", "loss_scale", "growth_tracker"):
        assert call(**{name: None}) == OFX_EINVAL and b"adamw_step_scaled" in lib.ofx_last_error(), name
    for name in ("loss_scale", "growth_tracker"):
        assert call(**{name: pair.data_ptr() + 2}) == OFX_EINVAL, name
    for over in ({"growth_factor": 0.999}, {"growth_factor": float("nan")}, {"backoff_factor": 0.0}, {"backoff_factor": -0.5}, {"backoff_factor": 1.001},
                 {"backoff_factor": float("nan")}, {"growth_interval": 0}, {"growth_interval": -3}):
        assert call(**over) == OFX_EINVAL, over
    for n_seg in (0, 1025):
        assert call(n_segments=n_seg) == OFX_ESHAPE, n_seg
    for n_arena in (0, 100):
        assert call(n_arena=n_arena) == OFX_ESHAPE, n_arena
    assert call(ws_bytes=good["ws_bytes"] - 1) == OFX_EWORKSPACE
    assert call(grad=A.grad.data_ptr() + 4) == OFX_EINVAL
    # the edges that ARE allowed run: growth 1, backoff 1, interval 1 (a tracker of 0 reaches it at once)
    A.tracker.zero_()
    rc = lib.ofx_adamw_step_scaled(good["segments"], good["n_segments"], good["grad"], good["exp_avg"], good["exp_avg_sq"], good["n_arena"], good["step"],
                                   2e-5, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, good["loss_scale"], good["growth_tracker"], 1.0, 1.0, 1, good["grad_norm"],
                                   good["skipped"], good["ws"], good["ws_bytes"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and int(A.skipped) == 0 and float(A.step) == 1 and float(A.scale) == 65536.0 and int(A.tracker) == 0


# ------------------------------------------------------------------------------------------------ 6. the model
K_SMALL = 12                  # loss x 2^-12: see the test


def test_scaling_the_loss_costs_the_f16_backward_nothing_and_keeps_what_a_small_upstream_loses():
    """6. The f16 model, three backwards into one arena:
        a0       loss                      the step tests/test_gpu_train.py holds to 5e-3 per parameter
        a_small  loss x 2^-k               what an unscaled f16 step sees when the upstream is small (batch 3072, mean, / 4)
        a_scaled loss x 2^-k x 2^16, the arena then x 2^-16 (exact)
    k = 12 puts upstream x |cp_w| (the first f16 value of the backward, dX of the head) below f16's smallest normal 6.1e-5; asserted.
    a0 x 2^-k is exact in fp32, so it is what both should equal.  Distances are ||x - y|| / ||y|| over the elements the train_step
    fixture pins (small gradients whole, the big ones' strided samples), all of them at once:
        e_scaled <= e_f16 := distance of a0 from the fixture's reference gradients    (asserted: scaling costs nothing beyond f16 itself)
        e_small                                                                      (printed; the parent's behaviour, not asserted)
    The fixture's reference gradients are those of ITS batch, 12 outfits, so e_f16 is taken there; e_scaled and e_small are taken on
    that batch and on B = 5 (five outfits of its first five lengths), and both e_scaled are held to e_f16.  Measured on an MI355X: DESIGN.md section 6."""
    T.need_gpu()
    from outfitx_amd.trainer import FlatGrads
    from src.losses import FocalLoss
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    g = golden("train_step")
    n = g["n_items"]
    m = T_train_model()
    params = {k: v for k, v in m.named_parameters() if not k.startswith("item_encoder.")}
    names = [str(k) for k in g["grad_names"]]
    fg = FlatGrads([params[k] for k in names])
    loss_fn = FocalLoss(alpha=0.75, gamma=2, reduction="mean")
    w_max = float(params["cp_ffn.1.weight"].abs().max())
    ref = np.concatenate([np.asarray(g["grad/" + k] if "grad/" + k in g.files else g["gsample/" + k], np.float64).ravel() for k in names])

    def pinned(a):
        """The fixture's elements of an arena, concatenated (float64)."""
        out = []
        for k, o in zip(names, fg.offsets):
            t = a[o:o + params[k].numel()].cpu().numpy().astype(np.float64)
            out.append(t if "grad/" + k in g.files else t[::1009])
        return np.concatenate(out)

    e_f16 = None
    for B in (len(n), 5):
        emb, mask = synth.outfit_batch(int(g["seed"]), B, 16, n[:B])
        x, km, labels = cu(emb), cu(mask), cu(g["labels"][:B])

        def arena(factor):
            fg.zero_()
            y_hat = m(task=CP, outfit_embedding=x, outfit_mask=km).squeeze(-1)
            y_hat.retain_grad()
            (loss_fn(y_hat=y_hat, y_true=labels) * factor).backward()
            return fg.flat.clone(), float(y_hat.grad.abs().max())

        a0, up0 = arena(1.0)
        a_small, up_small = arena(2.0 ** -K_SMALL)
        a_scaled, _ = arena(2.0 ** (16 - K_SMALL))
        a_scaled = a_scaled * 2.0 ** -16
        print(f"B = {B}: upstream max {up0:.3e} (x 2^-{K_SMALL}: {up_small:.3e}), |cp_w| max {w_max:.3e}, product {up_small * w_max:.3e}")
        assert abs(up_small - up0 * 2.0 ** -K_SMALL) <= 1e-6 * up_small and 0 < up_small * w_max < 6.1e-5
        if e_f16 is None:                                    # the fixture's own batch comes first
            e_f16 = T_nrm(pinned(a0) - ref) / T_nrm(ref)
            assert e_f16 <= 5e-3, e_f16
        want = pinned(a0) * 2.0 ** -K_SMALL
        e_scaled = T_nrm(pinned(a_scaled) - want) / T_nrm(want)
        e_small = T_nrm(pinned(a_small) - want) / T_nrm(want)
        whole = lambda a: float((a.double() - a0.double() * 2.0 ** -K_SMALL).norm() / (a0.double() * 2.0 ** -K_SMALL).norm())
        print(f"B = {B}: e_f16 {e_f16:.3e}  e_scaled {e_scaled:.3e}  e_small {e_small:.3e}   (whole arena: e_scaled {whole(a_scaled):.3e}  "
              f"e_small {whole(a_small):.3e})")
        assert np.isfinite(e_small)
        assert e_scaled <= e_f16, (B, e_scaled, e_f16)


@functools.lru_cache(maxsize=None)
def T_train_model():
    import test_gpu_train as TT
    return TT.make_model("f16")


def T_nrm(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))


# ------------------------------------------------------------------------------------------------ 7. the trainers
def cp_batches():
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    out = []
    for i in range(4):
        emb, mask = synth.outfit_batch(40 + i, 8, 16, 4)
        out.append({"input_dict": {"task": CP, "outfit_embedding": torch.from_numpy(emb).cuda(), "outfit_mask": torch.from_numpy(mask).cuda()},
                    "label": (torch.arange(8) % 2).float().cuda()})
    return out


def cir_batches(B=8, K=3):
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    out = []
    for i in range(4):
        emb, mask = synth.outfit_batch(50 + i, B, 16, 4)
        out.append({"input_dict": {"task": CIR, "outfit_embedding": torch.from_numpy(emb).cuda(), "outfit_mask": torch.from_numpy(mask).cuda(),
                                   "target_item_text_embedding": torch.from_numpy(synth.unit_rows(50 + i, "target_text", B, 512)).cuda()},
                    "pos_item_embedding": torch.from_numpy(synth.item_embeddings(50 + i, "pos", B) * 3.0).cuda(),
                    "neg_items_embedding": torch.from_numpy(synth.item_embeddings(50 + i, "neg", B * K).reshape(B, K, 1024) * 3.0).cuda(),
                    "neg_items_mask": torch.zeros(B, K, dtype=torch.bool).cuda()})
    return out


@pytest.mark.parametrize("kind", ["cp", "cir"])
def test_trainers_with_the_hip_optimizer_and_loss_scaling_on_the_f16_model(kind):
    """7. train_precision f16, hip_optimizer, loss_scaling, two windows of two micro-batches: finite parameters, no skipped step, tracker
    2, the scale still 65536, an unscaled norm; then, from the same start, the second window with an inf in the arena: parameters are those
    after window one, the scale is halved, the tracker 0.  The scaling multiply and the whole boundary run under
    torch.cuda.set_sync_debug_mode("error"): nothing reads anything back."""
    T.need_gpu()
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer, CPTrainConfig, CPTrainer
    m = T_train_model()
    named = {k: v for k, v in m.named_parameters() if not k.startswith("item_encoder.")}
    start = {k: v.detach().clone() for k, v in named.items()}
    batches = cp_batches() if kind == "cp" else cir_batches()

    def trainer():
        with torch.no_grad():
            for k, v in named.items():
                v.copy_(start[k])
        m.mark_weights_changed()
        kw = dict(learning_rate=1e-3, accumulation_steps=2, n_epochs=1, hip_optimizer=True, loss_scaling=True)
        if kind == "cp":
            return CPTrainer(m, steps_per_epoch=200, cfg=CPTrainConfig(**kw), params=list(named.values()))
        on_path = [p for p in CIRTrainer._default_params(m) if any(p is q for q in named.values())]
        return CIRTrainer(m, steps_per_epoch=200, cfg=CIRTrainConfig(**kw), params=on_path)

    def last_micro_step_checked(tr, batch, plant):
        """The window's last micro-batch written out, its scaling multiply and its boundary under the sync checker."""
        if kind == "cp":
            loss = tr.loss_fn(y_hat=tr.model(**tr._inputs(batch)).squeeze(dim=-1), y_true=batch["label"])
        else:
            loss = tr._loss(batch, tr.model(**tr._inputs(batch)))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            scaled = tr.optimizer.scale(loss / tr.cfg.accumulation_steps)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        scaled.backward()
        pre = tr.grads.flat.double().norm() / tr.optimizer.loss_scale            # the unscaled norm the boundary should report
        if plant:
            tr.grads.flat[1000:1001].fill_(float("inf"))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            tr._boundary_step(False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return loss.detach(), float(pre)

    try:
        # ---- two clean windows
        tr = trainer()
        opt = tr.optimizer
        assert isinstance(opt, FlatAdamW) and opt.loss_scaling and tr.scaler is None and float(opt.loss_scale) == 65536.0
        losses = [float(tr.micro_step(b, i)[0]) for i, b in enumerate(batches[:3])]
        last, want_norm = last_micro_step_checked(tr, batches[3], plant=False)
        losses.append(float(last))
        assert all(np.isfinite(losses)) and all(0 < l < 1e3 for l in losses), losses           # reported unscaled
        assert int(tr.last_step_skipped) == 0 and int(opt.growth_tracker) == 2 and float(opt.loss_scale) == 65536.0 and float(opt.step_t) == 2
        norm = float(tr.last_grad_norm)
        assert np.isfinite(norm) and norm > 0 and abs(norm - want_norm) <= 1e-5 * want_norm, (norm, want_norm)      # the UNSCALED norm
        assert all(bool(torch.isfinite(v).all()) for v in named.values())
        assert int((bits(tr.grads.flat) != 0).sum()) == 0
        moved = [k for k, v in named.items() if any(v is p for p in tr.grads.params) and not torch.equal(v, start[k])]
        assert len(moved) == len(tr.grads.params)
        sd = opt.state_dict()
        assert sd["scale"] == 65536.0 and sd["growth_tracker"] == 2
        print(kind, "losses", losses, "unscaled norm", norm)
        # ---- the same start, an inf in the second window
        tr = trainer()
        opt = tr.optimizer
        for i in range(2):
            tr.micro_step(batches[i], i)
        torch.cuda.synchronize()
        after_one = {k: v.detach().clone() for k, v in named.items()}
        assert int(opt.growth_tracker) == 1 and int(tr.last_step_skipped) == 0
        tr.micro_step(batches[2], 2)
        last_micro_step_checked(tr, batches[3], plant=True)
        assert int(tr.last_step_skipped) == 1 and float(opt.loss_scale) == 32768.0 and int(opt.growth_tracker) == 0 and float(opt.step_t) == 1
        for k, v in named.items():
            assert torch.equal(bits(v), bits(after_one[k])), k
        assert int((bits(tr.grads.flat) != 0).sum()) == 0
        # old state dicts (no scaler keys) still load, and the scaler's survive a round trip
        sd = opt.state_dict()
        assert sd["scale"] == 32768.0 and sd["growth_tracker"] == 0
        old = {k: v for k, v in sd.items() if k not in ("scale", "growth_tracker")}
        opt.loss_scale.fill_(4.0); opt.growth_tracker.fill_(7)
        opt.load_state_dict(old)
        assert float(opt.loss_scale) == 4.0 and int(opt.growth_tracker) == 7
        opt.load_state_dict(sd)
        assert float(opt.loss_scale) == 32768.0 and int(opt.growth_tracker) == 0 and float(opt.step_t) == 1
    finally:
        torch.cuda.set_sync_debug_mode("default")
        with torch.no_grad():
            for k, v in named.items():
                v.copy_(start[k])
        m.mark_weights_changed()
