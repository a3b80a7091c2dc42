"""Fused clip + AdamW + zero over the gradient arena (ofx_adamw_step, outfitx_amd/csrc/optim.hip), optim.FlatAdamW and the trainers'
hip_optimizer path.

Reference for every comparison: tests/flat_adamw_ref.py, the float64 restatement of clip_grad_norm_ + torch.optim.AdamW that
tests/test_cpu_flat_adamw_ref.py pins against torch.  A step of the kernel is compared to the restatement of THAT step, taken from the
kernel's own fp32 inputs and with the clip coefficient defined from the fp32 norm the kernel reported (the norm is held separately,
against the float64 norm).  Bounds, in the restatement's error scales E_p, E_m, E_v, on EVERY element:
  * the four-step schedule: 4 x the worst ratio torch's own fp32 CPU step shows on the same inputs (same seed, worst over the four
    steps); the factor 4 is for a different but valid fp32 evaluation order (fma contraction, reciprocal forms);
  * other inputs (stub modules): 4 x the worst such ratio over the schedule's three seeds (`R.standard_bounds()`);
  * the norm: max(1e-6, 2 x torch's fp32 deviation) relative.
torch's own steps on the device (fused / foreach AdamW) are held to the yardstick test's bounds: below 4 units, norm below 1e-5.
"""
import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import flat_adamw_ref as R
from conftest import W_SEED
from outfitx_amd import synth

warnings.simplefilter("ignore")
pytestmark = pytest.mark.gpu
OFX_EINVAL, OFX_ESHAPE, OFX_EWORKSPACE = -1, -2, -4
SENTINEL = -7777.25


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Arena:
    """Parameters as views into ONE buffer filled with a sentinel (16-byte-aligned positions, >= 64 sentinel floats after each), the
    three arenas in FlatGrads' layout, and the call's scalars."""

    def __init__(self, sizes, p0):
        from outfitx_amd.engine import adamw_step_ws_bytes
        from outfitx_amd.optim import segment_table
        self.sizes = list(sizes)
        pos, self.pos = 64, []
        for n in sizes:
            self.pos.append(pos)
            pos = (pos + n + 64 + 3) // 4 * 4
        self.buf = torch.full((pos,), SENTINEL, dtype=torch.float32, device="cuda")
        self.params = [self.buf[q:q + n] for q, n in zip(self.pos, sizes)]
        assert all(p.data_ptr() % 16 == 0 for p in self.params)
        self.offsets, n_arena = [], 0
        for n in sizes:
            self.offsets.append(n_arena)
            n_arena += (n + 63) // 64 * 64
        self.n = n_arena
        self.idx = torch.from_numpy(np.concatenate([o + np.arange(n) for o, n in zip(self.offsets, sizes)])).cuda()      # arena index of every live float
        pad = np.ones(n_arena, bool); pad[self.idx.cpu().numpy()] = False
        self.pad = torch.from_numpy(pad).cuda()
        sent = np.ones(pos, bool)
        for q, n in zip(self.pos, sizes):
            sent[q:q + n] = False
        self.sent = torch.from_numpy(sent).cuda()
        self.grad, self.m, self.v = (torch.zeros(n_arena, device="cuda") for _ in range(3))
        self.step = torch.zeros((), device="cuda")
        self.norm = torch.full((), float("nan"), device="cuda")
        self.skipped = torch.full((), -1, dtype=torch.int32, device="cuda")
        self.seg = segment_table(self.params, self.offsets).cuda()
        self.ws = torch.empty(adamw_step_ws_bytes(n_arena), dtype=torch.uint8, device="cuda")
        self.set_p(p0)

    def set_p(self, flat):
        o = 0
        for p, n in zip(self.params, self.sizes):
            p.copy_(cu(flat[o:o + n])); o += n

    def set_grad(self, flat):
        self.grad.zero_()
        self.grad[self.idx] = cu(flat)

    def p(self):
        return torch.cat(self.params).cpu().numpy()

    def live(self, arena):
        return arena[self.idx].cpu().numpy()

    def call(self, lr, beta1, grad_scale=1.0):
        from outfitx_amd.engine import adamw_step
        adamw_step(self.seg, self.grad, self.m, self.v, self.step, lr, beta1, R.BETA2, R.EPS, R.WD, R.MAX_NORM, grad_scale, self.norm, self.skipped, self.ws)

    def side_effects(self):
        """-> (non-zero words of the gradient arena, non-zero padding words of m and v, changed sentinel floats)."""
        return (int((self.grad.view(torch.int32) != 0).sum()), int((self.m.view(torch.int32)[self.pad] != 0).sum()) + int((self.v.view(torch.int32)[self.pad] != 0).sum()),
                int((self.buf[self.sent] != SENTINEL).sum()))


def run_schedule(seed):
    """The four-step schedule through engine.adamw_step -> (arena, per-step records)."""
    need_gpu()
    from outfitx_amd.engine import ADAMW_WG_FLOATS
    p0, grads = R.make_problem(seed)
    A = Arena(R.SIZES, p0)
    assert A.n > 2 * ADAMW_WG_FLOATS and -(-A.n // ADAMW_WG_FLOATS) > 2        # more than two workgroups: the norm crosses workgroups
    recs = []
    for k, (lr, b1, _) in enumerate(R.SCHEDULE):
        A.set_grad(grads[k])
        rec = {"p_in": A.p(), "m_in": A.live(A.m), "v_in": A.live(A.v), "g_in": grads[k], "t_old": k, "lr": lr, "beta1": b1}
        A.call(lr, b1)
        torch.cuda.synchronize()
        rec.update(p=A.p(), m=A.live(A.m), v=A.live(A.v), norm=float(A.norm), step=float(A.step), skipped=int(A.skipped), side=A.side_effects())
        recs.append(rec)
    return A, recs


@functools.lru_cache(maxsize=None)
def schedule_records(seed):
    return run_schedule(seed)[1]


def check_step(tag, rec, bound, norm_tol):
    """Print every figure of one recorded step, then assert the module's bounds on it."""
    r = R.ref_step(rec["p_in"], rec["m_in"], rec["v_in"], rec["g_in"], rec["t_old"], rec["lr"], rec["beta1"], grad_scale=rec.get("grad_scale", 1.0),
                   norm=rec["norm"])
    e = R.error_ratios(rec["p"], rec["m"], rec["v"], r)
    dn = abs(rec["norm"] - r["norm64"]) / r["norm64"]
    print(f"{tag}: norm {rec['norm']:.7g} rel {dn:.2e} (tol {norm_tol:.2e}); ratios p {e['p']:.2f} m {e['m']:.2f} v {e['v']:.2f} "
          f"(bounds {bound['p']:.2f} {bound['m']:.2f} {bound['v']:.2f})")
    assert dn <= norm_tol, (tag, dn)
    assert e["p"] <= bound["p"] and e["m"] <= bound["m"] and e["v"] <= bound["v"], (tag, e, bound)
    return e


def bounds_of(worst):
    return {k: 4 * worst[k] for k in ("p", "m", "v")}, max(1e-6, 2 * worst["norm"])


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("seed", R.SEEDS)
def test_parity_with_the_restatement_over_the_schedule(seed):
    """1. Four steps (three clipped, one not; lr and beta1 change every step), weight decay 0.01.  Worst ratios observed on an MI355X over
    the three seeds: see DESIGN.md section 6."""
    recs = schedule_records(seed)
    bound, norm_tol = bounds_of(R.torch_worst(seed))
    for k, rec in enumerate(recs):
        check_step(f"seed {seed} step {k + 1}", rec, bound, norm_tol)
        assert rec["step"] == k + 1 and rec["skipped"] == 0


@pytest.mark.parametrize("seed", R.SEEDS)
def test_side_effects(seed):
    """2. After every step: the whole gradient arena is all-zero bits, the moments' padding still is, every sentinel float is unchanged."""
    for k, rec in enumerate(schedule_records(seed)):
        assert rec["side"] == (0, 0, 0), (k, rec["side"])
        assert np.abs(rec["m"]).max() > 0 and np.abs(rec["v"]).max() > 0


def test_two_runs_from_the_same_state_give_the_same_bits():
    """3."""
    (a, _), (b, _) = run_schedule(0), run_schedule(0)
    assert torch.equal(a.buf, b.buf) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.norm, b.norm)


def test_grad_scale_is_applied_to_the_gradient_before_the_norm():
    """4. (g, grad_scale = 0.5) and (0.5 g, grad_scale = 1) are bit-identical in every output."""
    need_gpu()
    p0, grads = R.make_problem(0)
    lr, b1, _ = R.SCHEDULE[2]
    a, b = Arena(R.SIZES, p0), Arena(R.SIZES, p0)
    a.set_grad(grads[2]); b.set_grad(grads[2] * np.float32(0.5))
    rec = {"p_in": a.p(), "m_in": a.live(a.m), "v_in": a.live(a.v), "g_in": grads[2], "t_old": 0, "lr": lr, "beta1": b1, "grad_scale": 0.5}
    a.call(lr, b1, grad_scale=0.5); b.call(lr, b1, grad_scale=1.0)
    torch.cuda.synchronize()
    for x, y in ((a.buf, b.buf), (a.m, b.m), (a.v, b.v), (a.norm, b.norm), (a.step, b.step), (a.skipped, b.skipped), (a.grad, b.grad)):
        assert torch.equal(x, y)
    rec.update(p=a.p(), m=a.live(a.m), v=a.live(a.v), norm=float(a.norm))
    check_step("grad_scale 0.5", rec, *bounds_of(R.torch_worst(0)))
    assert a.side_effects() == (0, 0, 0)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_is_dropped_and_nothing_else_moves(bad):
    """5. One non-finite gradient element: p, m, v, *step bit-identical, gradient zero, *skipped == 1; the next finite step runs with
    t = 1 and matches the restatement."""
    need_gpu()
    p0, grads = R.make_problem(1)
    lr, b1, _ = R.SCHEDULE[2]
    A = Arena(R.SIZES, p0)
    g = np.random.default_rng(5)
    A.m[A.idx] = cu((g.standard_normal(len(p0)) * 0.1).astype(np.float32))          # non-trivial moments, so "untouched" says something
    A.v[A.idx] = cu((g.random(len(p0)) * 0.01).astype(np.float32))
    gbad = grads[2].copy(); gbad[70 + 4096 + 17] = bad                                # inside the 4097-element tensor
    A.set_grad(gbad)
    before = [t.clone() for t in (A.buf, A.m, A.v, A.step)]
    A.call(lr, b1)
    torch.cuda.synchronize()
    assert int(A.skipped) == 1 and not np.isfinite(float(A.norm))
    for x, y in zip(before, (A.buf, A.m, A.v, A.step)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert A.side_effects() == (0, 0, 0) and float(A.step) == 0
    A.set_grad(grads[2])
    rec = {"p_in": A.p(), "m_in": A.live(A.m), "v_in": A.live(A.v), "g_in": grads[2], "t_old": 0, "lr": lr, "beta1": b1}
    A.call(lr, b1)
    torch.cuda.synchronize()
    rec.update(p=A.p(), m=A.live(A.m), v=A.live(A.v), norm=float(A.norm))
    assert int(A.skipped) == 0 and float(A.step) == 1
    check_step(f"after a skipped {bad} step", rec, *bounds_of(R.torch_worst(1)))
    assert A.side_effects() == (0, 0, 0)


def test_refusals_launch_nothing():
    """6. NULL pointers -> OFX_EINVAL; n_segments 0 / 1025 and n_arena 0 / 100 -> OFX_ESHAPE; a workspace one byte short ->
    OFX_EWORKSPACE; p (and everything else) bit-identical after each.  FlatAdamW: OfxError on a CPU arena, ValueError on a misaligned view."""
    need_gpu()
    from outfitx_amd import _lib as L
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import FlatGrads
    lib = L.load()
    p0, grads = R.make_problem(2)
    A = Arena(R.SIZES, p0)
    A.set_grad(grads[2])
    before = [t.clone() for t in (A.buf, A.m, A.v, A.step, A.grad)]
    good = {"segments": A.seg.data_ptr(), "n_segments": len(R.SIZES), "grad": A.grad.data_ptr(), "exp_avg": A.m.data_ptr(), "exp_avg_sq": A.v.data_ptr(),
            "n_arena": A.n, "step": A.step.data_ptr(), "grad_norm": A.norm.data_ptr(), "skipped": A.skipped.data_ptr(), "ws": A.ws.data_ptr(),
            "ws_bytes": lib.ofx_adamw_step_ws_bytes(A.n)}

    def call(**over):
        a = dict(good, **over)
        rc = lib.ofx_adamw_step(a["segments"], a["n_segments"], a["grad"], a["exp_avg"], a["exp_avg_sq"], a["n_arena"], a["step"], 2e-5, 0.9, 0.999, 1e-8,
                                0.01, 1.0, 1.0, a["grad_norm"], a["skipped"], a["ws"], a["ws_bytes"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for x, y in zip(before, (A.buf, A.m, A.v, A.step, A.grad)):
            assert torch.equal(x, y), over
        return rc

    for name in ("segments", "grad", "exp_avg", "exp_avg_sq", "step", "grad_norm", "skipped", "ws"):
        assert call(**{name: None}) == OFX_EINVAL and b"adamw_step" in lib.ofx_last_error(), name
    for n_seg in (0, 1025):
        assert call(n_segments=n_seg) == OFX_ESHAPE, n_seg
    for n_arena in (0, 100):
        assert call(n_arena=n_arena) == OFX_ESHAPE, n_arena
        assert lib.ofx_adamw_step_ws_bytes(n_arena) == 0
    assert good["ws_bytes"] > 0 and call(ws_bytes=good["ws_bytes"] - 1) == OFX_EWORKSPACE
    with pytest.raises(L.OfxError):
        FlatAdamW(FlatGrads([torch.nn.Parameter(torch.zeros(8))]), lr=1e-3)
    base = torch.zeros(200, device="cuda")
    with pytest.raises(ValueError):
        FlatAdamW(FlatGrads([torch.nn.Parameter(base[1:65])]), lr=1e-3)
    from outfitx_amd.engine import adamw_step
    with pytest.raises(L.OfxError):
        adamw_step(A.seg.cpu(), A.grad.cpu(), A.m.cpu(), A.v.cpu(), A.step.cpu(), 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0, A.norm.cpu(), A.skipped.cpu())


# ------------------------------------------------------------------------------------------------ the optimizer object
class Stub(torch.nn.Module):
    """A few Linear layers of odd sizes: tensors of 693, 21, 147, 7, 7 and 1 elements (tails that are no multiple of 4)."""

    def __init__(self):
        super().__init__()
        self.a, self.b, self.c = torch.nn.Linear(33, 21), torch.nn.Linear(21, 7), torch.nn.Linear(7, 1)


def make_stub(seed=0):
    need_gpu()
    torch.manual_seed(seed)
    return Stub().cuda()


def stub_grads(model, seed, scale):
    g = np.random.default_rng(seed)
    return [cu((g.standard_normal(tuple(p.shape)) * scale).astype(np.float32)) for p in model.parameters()]


def flat_np(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def opt_state(opt, params, key):
    return flat_np([opt.state[p][key] if p in opt.state and key in opt.state[p] else torch.zeros_like(p) for p in params])


def one_step(model, opt, grads, flat: bool):
    """One clip + AdamW step of `opt` (FlatAdamW, or torch.optim.AdamW behind clip_grad_norm_) on `grads` -> the recorded step."""
    ps = list(model.parameters())
    for p, g in zip(ps, grads):
        if flat:
            p.grad.copy_(g)
        else:
            p.grad = g.clone()
    grp = opt.param_groups[0]
    t_old = float(opt.step_t) if flat else (float(opt.state[ps[0]]["step"]) if opt.state else 0.0)
    rec = {"p_in": flat_np(ps), "m_in": opt_state(opt, ps, "exp_avg"), "v_in": opt_state(opt, ps, "exp_avg_sq"), "g_in": flat_np(grads), "t_old": t_old,
           "lr": grp["lr"], "beta1": grp["betas"][0]}
    norm = None if flat else torch.nn.utils.clip_grad_norm_(ps, R.MAX_NORM)
    opt.step()
    torch.cuda.synchronize()
    rec.update(p=flat_np(ps), m=opt_state(opt, ps, "exp_avg"), v=opt_state(opt, ps, "exp_avg_sq"), norm=float(opt.grad_norm if flat else norm))
    return rec


YARDSTICK = ({"p": 4.0, "m": 4.0, "v": 4.0}, 1e-5)        # what tests/test_cpu_flat_adamw_ref.py asserts of torch's own fp32 step


def test_state_dict_round_trips_with_torch_adamw():
    """7. torch.optim.AdamW's state_dict after two torch steps loads into FlatAdamW (into its arenas, which stay where they are) and one
    more step in each agrees through the restatement; FlatAdamW's state_dict loads into a torch.optim.AdamW likewise; unequal per-parameter
    step values raise."""
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import FlatGrads
    bound, norm_tol = bounds_of(R.standard_bounds())
    ma = make_stub()
    oa = torch.optim.AdamW(ma.parameters(), lr=1e-3, weight_decay=R.WD)
    for k in range(2):
        one_step(ma, oa, stub_grads(ma, 10 + k, 1.0), flat=False)
    sd = oa.state_dict()
    mb = copy.deepcopy(ma)
    ob = FlatAdamW(FlatGrads(list(mb.parameters())), lr=1e-3)
    arenas = (ob.exp_avg.data_ptr(), ob.exp_avg_sq.data_ptr())
    ob.load_state_dict(sd)
    assert (ob.exp_avg.data_ptr(), ob.exp_avg_sq.data_ptr()) == arenas and float(ob.step_t) == 2
    assert np.array_equal(opt_state(ob, list(mb.parameters()), "exp_avg"), opt_state(oa, list(ma.parameters()), "exp_avg"))
    g3 = stub_grads(ma, 12, 1.0)
    ra, rb = one_step(ma, oa, g3, flat=False), one_step(mb, ob, g3, flat=True)
    check_step("torch after its own two steps", ra, *YARDSTICK)
    check_step("FlatAdamW from torch's state_dict", rb, bound, norm_tol)
    assert float(ob.step_t) == 3 and abs(ra["norm"] - rb["norm"]) <= norm_tol * rb["norm"]
    assert int((ob.flat_grads.flat.view(torch.int32) != 0).sum()) == 0
    # ... and back: FlatAdamW's state_dict has torch's layout and loads into torch.optim.AdamW
    sd_b, sd_a = ob.state_dict(), oa.state_dict()
    assert set(sd_b) == set(sd_a) and set(sd_b["param_groups"][0]) == set(sd_a["param_groups"][0]) and set(sd_b["state"]) == set(sd_a["state"])
    assert all(set(sd_b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd_b["state"][i]["step"]) == 3 for i in sd_b["state"])
    mc = copy.deepcopy(mb)
    oc = torch.optim.AdamW(mc.parameters(), lr=1e-3, weight_decay=R.WD)
    oc.load_state_dict(sd_b)
    g4 = stub_grads(ma, 13, 0.01)                                           # norm about 0.3: unclipped
    rb4, rc4 = one_step(mb, ob, g4, flat=True), one_step(mc, oc, g4, flat=False)
    assert rc4["t_old"] == 3 and rb4["norm"] < 1.0
    check_step("FlatAdamW, fourth step", rb4, bound, norm_tol)
    check_step("torch from FlatAdamW's state_dict", rc4, *YARDSTICK)
    bad = copy.deepcopy(sd)
    bad["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError):
        ob.load_state_dict(bad)


def test_a_torch_state_dict_without_state_for_some_parameters_loads():
    """7b. torch.optim.AdamW gives a parameter state at its first gradient, so the reference's checkpoints have no entry for tensors
    off the task's path.  Such a state_dict loads: the missing tensors get zero moments, the others their own, the step count is the
    stepped ones'; one more step then meets the bounds against the restatement from exactly that state."""
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import FlatGrads
    bound, norm_tol = bounds_of(R.standard_bounds())
    ma = make_stub(3)
    ps = list(ma.parameters())
    oa = torch.optim.AdamW(ps, lr=1e-3, weight_decay=R.WD)
    for k in range(2):
        for p, g in zip(ps[:4], stub_grads(ma, 40 + k, 1.0)[:4]):          # the last Linear never gets a gradient
            p.grad = g
        torch.nn.utils.clip_grad_norm_(ps[:4], R.MAX_NORM)
        oa.step()
    sd = oa.state_dict()
    assert sorted(sd["state"]) == [0, 1, 2, 3] and len(sd["param_groups"][0]["params"]) == 6
    mb = copy.deepcopy(ma)
    for p in mb.parameters():
        p.grad = None
    ob = FlatAdamW(FlatGrads(list(mb.parameters())), lr=1e-3)
    ob.exp_avg.fill_(3.0); ob.exp_avg_sq.fill_(3.0)                          # stale contents must not survive the load
    ob.load_state_dict(sd)
    pb = list(mb.parameters())
    assert float(ob.step_t) == 2
    assert np.array_equal(opt_state(ob, pb[:4], "exp_avg"), opt_state(oa, ps[:4], "exp_avg"))
    assert not opt_state(ob, pb[4:], "exp_avg").any() and not opt_state(ob, pb[4:], "exp_avg_sq").any()
    torch.optim.AdamW(copy.deepcopy(ma).parameters(), lr=1e-3).load_state_dict(sd)      # what torch itself accepts
    ob.exp_avg.zero_(); ob.exp_avg_sq.zero_(); ob.load_state_dict(sd)        # padding back to zero (the fill above was the test's own)
    rec = one_step(mb, ob, stub_grads(mb, 42, 1.0), flat=True)
    assert rec["t_old"] == 2 and float(ob.step_t) == 3
    check_step("FlatAdamW from a partial torch state_dict", rec, bound, norm_tol)


def test_a_parameter_whose_storage_moved_is_found_again():
    """The segment table follows p.data = p.data.clone(): the step updates the new storage and leaves the old one alone."""
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import FlatGrads
    bound, norm_tol = bounds_of(R.standard_bounds())
    m = make_stub(4)
    opt = FlatAdamW(FlatGrads(list(m.parameters())), lr=1e-3)
    table = opt.segments.data_ptr()
    one_step(m, opt, stub_grads(m, 50, 1.0), flat=True)
    moved = list(m.parameters())[0]
    old = moved.data
    kept = old.clone()
    moved.data = old.clone()
    assert moved.data_ptr() != old.data_ptr()
    rec = one_step(m, opt, stub_grads(m, 51, 1.0), flat=True)
    check_step("after p.data moved", rec, bound, norm_tol)
    assert torch.equal(old, kept) and not torch.equal(moved.data, kept) and opt.segments.data_ptr() == table


def test_one_cycle_lr_drives_lr_and_beta1():
    """8. OneCycleLR (cycle_momentum left at its default) over FlatAdamW: the third step() ran with the scheduler's lr and beta1 - the
    restatement with those values meets the bounds, the one with the constructor's beta1 does not."""
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import FlatGrads
    bound, norm_tol = bounds_of(R.standard_bounds())
    m = make_stub(1)
    opt = FlatAdamW(FlatGrads(list(m.parameters())), lr=1e-3)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-3, total_steps=6)
    twin_opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    twin = torch.optim.lr_scheduler.OneCycleLR(twin_opt, max_lr=1e-3, total_steps=6)
    fired = []
    h = opt.register_step_post_hook(lambda *a: fired.append(1))
    for k in range(3):
        want_lr, want_b1 = twin_opt.param_groups[0]["lr"], twin_opt.param_groups[0]["betas"][0]
        rec = one_step(m, opt, stub_grads(m, 20 + k, 1.0), flat=True)
        assert rec["lr"] == want_lr and rec["beta1"] == want_b1
        sched.step(); twin_opt.step(); twin.step()
    h.remove()
    assert len(fired) == 3 and 0.85 <= want_b1 < 0.95 and want_lr > 1e-3 / 25
    rec.update(lr=want_lr, beta1=want_b1)
    check_step(f"third step, scheduler's lr {want_lr:.3e} beta1 {want_b1:.4f}", rec, bound, norm_tol)
    wrong = R.error_ratios(rec["p"], rec["m"], rec["v"], R.ref_step(rec["p_in"], rec["m_in"], rec["v_in"], rec["g_in"], 2, want_lr, 0.9, norm=rec["norm"]))
    assert wrong["m"] > 100 * bound["m"], wrong


# ------------------------------------------------------------------------------------------------ the trainers
def test_boundary_step_of_both_trainer_forms():
    """9. Two CPTrainers over identical stubs, hip_optimizer off and on, the same arena contents (first boundary clipped, second not):
    the HIP path meets the bounds against the restatement, torch's path the yardstick's; both arenas end zero and the norms agree."""
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import CPTrainConfig, CPTrainer
    bound, norm_tol = bounds_of(R.standard_bounds())
    m0 = make_stub(2)
    trs = []
    for hip in (False, True):
        m = copy.deepcopy(m0)
        trs.append((m, CPTrainer(m, steps_per_epoch=4, cfg=CPTrainConfig(learning_rate=1e-3, accumulation_steps=1, n_epochs=1, hip_optimizer=hip))))
    assert isinstance(trs[1][1].optimizer, FlatAdamW) and not isinstance(trs[0][1].optimizer, FlatAdamW)
    assert trs[0][1].last_step_skipped is None
    for k, scale in enumerate((1.0, 0.01)):
        recs = []
        for hip, (m, tr) in zip((False, True), trs):
            ps, opt = list(m.parameters()), tr.optimizer
            gs = stub_grads(m, 30 + k, scale)
            for p, g in zip(ps, gs):
                p.grad.copy_(g)
            assert all(p.grad.data_ptr() == tr.grads.flat.data_ptr() + 4 * o for p, o in zip(tr.grads.params, tr.grads.offsets))
            grp = opt.param_groups[0]
            rec = {"p_in": flat_np(ps), "m_in": opt_state(opt, ps, "exp_avg"), "v_in": opt_state(opt, ps, "exp_avg_sq"), "g_in": flat_np(gs), "t_old": k,
                   "lr": grp["lr"], "beta1": grp["betas"][0]}
            tr._boundary_step(False)
            torch.cuda.synchronize()
            rec.update(p=flat_np(ps), m=opt_state(opt, ps, "exp_avg"), v=opt_state(opt, ps, "exp_avg_sq"), norm=float(tr.last_grad_norm))
            assert int((tr.grads.flat.view(torch.int32) != 0).sum()) == 0
            recs.append(rec)
        assert (recs[0]["norm"] > 1.0) == (k == 0)
        check_step(f"boundary {k + 1}, torch path", recs[0], *YARDSTICK)
        check_step(f"boundary {k + 1}, hip_optimizer", recs[1], bound, norm_tol)
        assert abs(recs[0]["norm"] - recs[1]["norm"]) <= norm_tol * recs[1]["norm"]
        assert recs[0]["lr"] == recs[1]["lr"] and recs[0]["beta1"] == recs[1]["beta1"]       # the two schedulers walk together
    tr = trs[1][1]
    assert int(tr.last_step_skipped) == 0 and tr.last_grad_norm is tr.optimizer.grad_norm and float(tr.optimizer.step_t) == 2


@functools.lru_cache(maxsize=None)
def real_model():
    need_gpu()
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    cfg = OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip"))
    cfg.transformer.dropout = 0.0
    m = OutfitX(cfg, train_precision="bf16")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.full_state_dict(W_SEED).items()}, strict=True)
    return m.cuda().train()


def trainable(m):
    return {k: v for k, v in m.named_parameters() if not k.startswith("item_encoder.")}


def scoring_forward(m, inp):
    m.eval()
    with torch.no_grad():
        y = m(**inp).clone()
    m.train()
    return y


def test_cp_trainer_with_the_hip_optimizer_on_the_real_model():
    """10. OutfitX, CPTrainer(hip_optimizer=True), accumulation 2, two micro-batches of 8 outfits x 4 items: finite loss, every trainable
    parameter changed, the arena is zero, and a forward after the step differs from one before it (the packed copies were refreshed).
    100 optimizer steps are scheduled so that OneCycleLR starts at lr = 1e-3 / 25: tensors off the CP path move by weight decay alone,
    and 1 - lr * 0.01 must not round to 1 in fp32."""
    from outfitx_amd.trainer import CPTrainConfig, CPTrainer
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    m = real_model()
    batches = []
    for i in range(2):
        emb, mask = synth.outfit_batch(40 + i, 8, 16, 4)
        batches.append({"input_dict": {"task": CP, "outfit_embedding": torch.from_numpy(emb), "outfit_mask": torch.from_numpy(mask)},
                        "label": (torch.arange(8) % 2).float()})
    inp = {k: (v if k == "task" else v.cuda()) for k, v in batches[0]["input_dict"].items()}
    y0 = scoring_forward(m, inp)
    before = {k: v.detach().clone() for k, v in trainable(m).items()}
    tr = CPTrainer(m, steps_per_epoch=200, cfg=CPTrainConfig(learning_rate=1e-3, accumulation_steps=2, n_epochs=1, hip_optimizer=True),
                   params=list(trainable(m).values()))
    losses = [float(tr.micro_step(b, i)[0]) for i, b in enumerate(batches)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    assert int(tr.last_step_skipped) == 0 and np.isfinite(float(tr.last_grad_norm)) and float(tr.last_grad_norm) > 0 and float(tr.optimizer.step_t) == 1
    same = [k for k, v in trainable(m).items() if torch.equal(v, before[k])]
    assert not same, same
    assert int((tr.grads.flat.view(torch.int32) != 0).sum()) == 0
    y1 = scoring_forward(m, inp)
    print("CP losses", losses, "norm", float(tr.last_grad_norm), "logit change", float((y1 - y0).abs().max()))
    assert torch.isfinite(y1).all() and not torch.equal(y0, y1)


def test_cir_trainer_with_the_hip_optimizer_on_the_real_model():
    """10, CIR: K = 3 negatives; outfit_token and the CP head are outside the arena and must stay bit-unchanged."""
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer
    from src.models.datatypes import OutfitComplementaryItemRetrievalTask as CIR
    m = real_model()
    B, K = 8, 3
    batches = []
    for i in range(2):
        emb, mask = synth.outfit_batch(50 + i, B, 16, 4)
        batches.append({"input_dict": {"task": CIR, "outfit_embedding": torch.from_numpy(emb), "outfit_mask": torch.from_numpy(mask),
                                       "target_item_text_embedding": torch.from_numpy(synth.unit_rows(50 + i, "target_text", B, 512))},
                        "pos_item_embedding": torch.from_numpy(synth.item_embeddings(50 + i, "pos", B) * 3.0),
                        "neg_items_embedding": torch.from_numpy(synth.item_embeddings(50 + i, "neg", B * K).reshape(B, K, 1024) * 3.0),
                        "neg_items_mask": torch.zeros(B, K, dtype=torch.bool)})
    inp = {k: (v if k == "task" else v.cuda()) for k, v in batches[0]["input_dict"].items()}
    y0 = scoring_forward(m, inp)
    before = {k: v.detach().clone() for k, v in trainable(m).items()}
    on_path = [p for p in CIRTrainer._default_params(m) if any(p is q for q in trainable(m).values())]
    tr = CIRTrainer(m, steps_per_epoch=200, cfg=CIRTrainConfig(learning_rate=1e-3, accumulation_steps=2, n_epochs=1, hip_optimizer=True), params=on_path)
    assert tr.optimizer.segments.shape[0] == len(on_path) == len(before) - 3
    losses = [float(tr.micro_step(b, i)[0]) for i, b in enumerate(batches)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    assert int(tr.last_step_skipped) == 0 and np.isfinite(float(tr.last_grad_norm)) and float(tr.last_grad_norm) > 0
    for k, v in trainable(m).items():
        if k in ("outfit_token", "cp_ffn.1.weight", "cp_ffn.1.bias"):
            assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), k
        else:
            assert not torch.equal(v, before[k]), k
    assert int((tr.grads.flat.view(torch.int32) != 0).sum()) == 0
    y1 = scoring_forward(m, inp)
    print("CIR losses", losses, "norm", float(tr.last_grad_norm), "embedding change", float((y1 - y0).abs().max()))
    assert torch.isfinite(y1).all() and not torch.equal(y0, y1)
