"""CPU checks of dynamic loss scaling (trainer.py's `loss_scaling`, optim.FlatAdamW(loss_scaling=True), ofx_adamw_step_scaled): the numpy
restatement of GradScaler's state machine (tests/loss_scale_ref.py) against torch.amp.GradScaler('cpu'), the trainers' torch-optimizer
form on plain-torch stand-in modules against a hand-written GradScaler loop, and the new C entry in header, ctypes table and library.
(The fused call only runs on a HIP device: tests/test_gpu_loss_scale.py.)"""
import copy
import os
import re

import numpy as np
import pytest
import torch

import loss_scale_ref as S
from conftest import ROOT

I, F = True, False
PATTERNS = {
    "backoff": (2000, [F, I, F, F]),
    "growth at interval 1": (1, [F, F, F, I, F]),
    "growth at interval 2": (2, [F, F, F, F, F, I, F, F]),
    "growth at interval 3": (3, [F, F, F, F, F, F, F]),
    "inf on the step that would have grown": (3, [F, F, I, F, F, F, F]),
    "consecutive infs": (2, [I, I, I, F, F, I, I, F, F, F]),
    "the GPU trajectory test's pattern": (3, [F, I, F, F, F, I, F]),
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_the_restated_state_machine_is_torchs_grad_scaler(name):
    interval, infs = PATTERNS[name]
    for init, growth, backoff in ((65536.0, 2.0, 0.5), (1000.0, 1.7, 0.3)):
        got = S.scaler_trajectory(infs, init, growth, backoff, interval)
        want = S.torch_scaler_trajectory(infs, init, growth, backoff, interval)
        assert got == want, (name, init, got, want)
    scales = [65536.0] + [s for s, _ in S.scaler_trajectory(infs, interval=interval)]                 # the pattern does what its name says
    assert any(b < a for a, b in zip(scales, scales[1:])) == any(infs) and ("growth" not in name or any(b > a for a, b in zip(scales, scales[1:])))


def test_growth_that_would_overflow_keeps_the_scale():
    big = float(np.float32(3e38))
    assert S.scaler_trajectory([F], big, interval=1) == S.torch_scaler_trajectory([F], big, interval=1) == [(big, 0)]


# ------------------------------------------------------------------------------------------------ the trainers, torch optimizer
class CPStub(torch.nn.Module):               # stands in for OutfitX on the CP path: same call signature, plain torch, CPU
    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.a = torch.nn.Linear(16, 8); self.b = torch.nn.Linear(8, 1)

    def forward(self, task, outfit_embedding, outfit_mask):
        keep = (~outfit_mask).float().unsqueeze(-1)
        pooled = (outfit_embedding * keep).sum(1) / keep.sum(1).clamp(min=1)
        return self.b(torch.nn.functional.mish(self.a(pooled)))


class CIRStub(torch.nn.Module):              # ... and on the CIR path; outfit_token and cp_ffn are off it, as in OutfitX
    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.a = torch.nn.Linear(16 + 8, 12, bias=False)
        self.outfit_token = torch.nn.Parameter(torch.randn(16))
        self.cp_ffn = torch.nn.Sequential(torch.nn.Dropout(0.0), torch.nn.Linear(16, 1))
        self.l = torch.nn.Linear(16, 16)

    def forward(self, task, outfit_embedding, outfit_mask, target_item_text_embedding):
        keep = (~outfit_mask).float().unsqueeze(-1)
        x = outfit_embedding + torch.tanh(self.l(outfit_embedding))
        pooled = (x * keep).sum(1) / keep.sum(1).clamp(min=1)
        return self.a(torch.cat([pooled, target_item_text_embedding], -1))


def focal(y_hat, y_true):                    # src/losses/focal_loss.py:26-41 in torch ops (the fused kernel needs a HIP device)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(y_hat, y_true, reduction="none")
    p = torch.sigmoid(y_hat); pt = p * y_true + (1 - p) * (1 - y_true)
    return ((0.75 * y_true + 0.25 * (1 - y_true)) * ce * (1 - pt) ** 2).mean()


def make_batches(kind, n_steps, bsz=8, K=5):
    g = np.random.default_rng(5)
    out = []
    for _ in range(n_steps):
        emb = torch.from_numpy(g.standard_normal((bsz, 6, 16)).astype(np.float32))
        mask = torch.from_numpy(np.arange(6)[None, :] >= g.integers(1, 7, bsz)[:, None])
        if kind == "cp":
            out.append({"input_dict": {"task": None, "outfit_embedding": emb, "outfit_mask": mask},
                        "label": torch.from_numpy((g.random(bsz) < 0.5).astype(np.float32))})
        else:
            f = lambda *shape: torch.from_numpy(g.standard_normal(shape).astype(np.float32))
            out.append({"input_dict": {"task": None, "outfit_embedding": emb, "outfit_mask": mask, "target_item_text_embedding": f(bsz, 8)},
                        "pos_item_embedding": f(bsz, 12), "neg_items_embedding": f(bsz, K, 12),
                        "neg_items_mask": torch.from_numpy(g.random((bsz, K)) < 0.3)})
    return out


def setup(kind, **cfg):
    """-> (model, trainer, loss(model, batch), the parameters the trainer steps)."""
    from outfitx_amd.losses import SetWiseRankingLoss
    from outfitx_amd.trainer import CIRTrainConfig, CIRTrainer, CPTrainConfig, CPTrainer
    if kind == "cp":
        m = CPStub()
        tr = CPTrainer(m, steps_per_epoch=STEPS, cfg=CPTrainConfig(learning_rate=LR, accumulation_steps=ACC, n_epochs=2, **cfg), loss_fn=focal)
        loss = lambda model, b: focal(model(**b["input_dict"]).squeeze(dim=-1), b["label"])
    else:
        m = CIRStub()
        fn = SetWiseRankingLoss(margin=2.0)
        tr = CIRTrainer(m, steps_per_epoch=STEPS, cfg=CIRTrainConfig(learning_rate=LR, accumulation_steps=ACC, n_epochs=2, **cfg), loss_fn=fn)
        loss = lambda model, b: fn(batch_y=b["pos_item_embedding"], batch_y_hat=model(**b["input_dict"]),
                                   batch_negative_samples=b["neg_items_embedding"], batch_negative_mask=b["neg_items_mask"])
    return m, tr, loss


STEPS, ACC, LR = 5, 2, 1e-2                  # three windows; the last one is short
SCALER = dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)


def on_path(model):
    off = {id(p) for p in [getattr(model, "outfit_token", None), *getattr(model, "cp_ffn", torch.nn.Module()).parameters()]}
    return [p for p in model.parameters() if id(p) not in off]


def grad_scaler_loop(ref, loss, batches, inf_at=None):
    """The reference's step (compatibility_prediction_trainer.py:63-77) written out: scaler.scale(loss).backward() -> unscale_ ->
    clip_grad_norm_ -> scaler.step -> scaler.update -> zero_grad -> scheduler step.  inf_at: the micro-step after whose backward one
    gradient element is overwritten with inf.  -> (scaler, per-step unscaled losses, per-window clip norms)."""
    ps = on_path(ref)
    opt = torch.optim.AdamW(ps, lr=LR)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, epochs=2, steps_per_epoch=-(-STEPS // ACC), pct_start=0.3, anneal_strategy="cos",
                                              div_factor=25, final_div_factor=1e4)
    sc = torch.amp.GradScaler("cpu", **SCALER)
    losses, norms = [], []
    for step, b in enumerate(batches):
        l = loss(ref, b)
        sc.scale(l / ACC).backward()
        losses.append(float(l.detach()))
        if step == inf_at:
            ps[0].grad.view(-1)[3] = float("inf")
        if (step + 1) % ACC == 0 or step + 1 == STEPS:
            sc.unscale_(opt)
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm=1.0)))
            sc.step(opt); sc.update(); opt.zero_grad(); sch.step()
    return sc, losses, norms


@pytest.mark.parametrize("kind", ["cp", "cir"])
def test_trainer_with_loss_scaling_equals_a_hand_written_grad_scaler_loop(kind):
    """Three windows, growth_interval 2: the scale doubles after the second.  Parameters, reported (unscaled) losses, the unscaled clip
    norm and the scaler's state equal the loop's (the tolerance of tests/test_cpu_cir_trainer.py: the arena's one norm against
    clip_grad_norm_'s norm of norms)."""
    m, tr, loss = setup(kind, loss_scaling=True, **SCALER)
    assert isinstance(tr.scaler, torch.amp.GradScaler) and tr.loss_scaling
    ref = copy.deepcopy(m)
    batches = make_batches(kind, STEPS)
    sc, want_losses, want_norms = grad_scaler_loop(ref, loss, batches)
    m.train(); tr.grads.zero_()
    norms = []
    for step, b in enumerate(batches):
        got = tr.micro_step(b, step)[0]
        assert abs(float(got) - want_losses[step]) <= 2e-5 * abs(want_losses[step]) + 1e-6, (step, float(got), want_losses[step])
        if (step + 1) % ACC == 0 or step + 1 == STEPS:
            norms.append(float(tr.last_grad_norm))
            assert not tr.grads.flat.any()
    assert np.allclose(norms, want_norms, rtol=2e-5) and all(0 < n < 100 for n in norms), (norms, want_norms)       # unscaled: not x 1024
    for a, w in zip(m.parameters(), ref.parameters()):
        assert torch.allclose(a, w, rtol=2e-5, atol=1e-6), (a - w).abs().max()
    assert not torch.equal(on_path(m)[0], on_path(type(m)())[0])                                   # it trained
    sd = tr.scaler.state_dict()
    assert (sd["scale"], sd["_growth_tracker"]) == (sc.state_dict()["scale"], sc.state_dict()["_growth_tracker"]) == (2048.0, 1)


@pytest.mark.parametrize("kind", ["cp", "cir"])
def test_a_planted_inf_skips_the_window_and_halves_the_scale(kind):
    m, tr, loss = setup(kind, loss_scaling=True, **SCALER)
    batches = make_batches(kind, STEPS)
    m.train(); tr.grads.zero_()
    tr.micro_step(batches[0], 0); tr.micro_step(batches[1], 1)
    after_one = [p.detach().clone() for p in m.parameters()]
    lr_before = tr.scheduler.get_last_lr()[0]
    tr.micro_step(batches[2], 2)
    # the second window's last micro-batch, by hand, with an inf in the arena before the boundary
    l = loss(m, batches[3])
    tr.scaler.scale(l / ACC).backward()
    tr.grads.flat[3] = float("inf")
    tr._boundary_step(False)
    for a, w in zip(m.parameters(), after_one):
        assert torch.equal(a, w)
    sd = tr.scaler.state_dict()
    assert (sd["scale"], sd["_growth_tracker"]) == (512.0, 0)
    assert not tr.grads.flat.any() and tr.scheduler.get_last_lr()[0] != lr_before                   # zeroed; the schedule moved on
    # ... and the same through a hand-written loop with the inf at the same place
    ref = type(m)()
    sc, _, _ = grad_scaler_loop(ref, loss, batches[:4], inf_at=3)
    assert sc.state_dict()["scale"] == 512.0
    for a, w in zip(m.parameters(), ref.parameters()):
        assert torch.allclose(a, w, rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("kind", ["cp", "cir"])
def test_the_default_config_steps_exactly_as_before(kind):
    """loss_scaling is off by default: no scaler exists, and the parameters after an epoch are, bit for bit, those of the boundary the
    trainer has always run, written out here - (loss / accumulation_steps).backward() into the arena, the arena's norm and clip, AdamW,
    OneCycleLR, zero."""
    from outfitx_amd.trainer import CIRTrainConfig, CPTrainConfig, FlatGrads
    for c in (CPTrainConfig(), CIRTrainConfig()):
        assert (c.loss_scaling, c.init_scale, c.growth_factor, c.backoff_factor, c.growth_interval) == (False, 65536.0, 2.0, 0.5, 2000)
    sd = torch.amp.GradScaler("cpu").state_dict()                                                   # ... which are torch's own
    assert (sd["scale"], sd["growth_factor"], sd["backoff_factor"], sd["growth_interval"]) == (65536.0, 2.0, 0.5, 2000)
    m, tr, loss = setup(kind)
    assert tr.scaler is None and not tr.loss_scaling
    ref = copy.deepcopy(m)
    grads = FlatGrads(on_path(ref))
    opt = torch.optim.AdamW(grads.params, lr=LR)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, epochs=2, steps_per_epoch=-(-STEPS // ACC), pct_start=0.3, anneal_strategy="cos",
                                              div_factor=25, final_div_factor=1e4)
    batches = make_batches(kind, STEPS)
    m.train(); tr.grads.zero_()
    for step, b in enumerate(batches):
        got = tr.micro_step(b, step)[0]
        l = loss(ref, b)
        (l / ACC).backward()
        assert torch.equal(got, l.detach())
        if (step + 1) % ACC == 0 or step + 1 == STEPS:
            grads.clip_norm_(1.0); opt.step(); sch.step(); grads.zero_()
    for a, w in zip(m.parameters(), ref.parameters()):
        assert torch.equal(a, w)


# ------------------------------------------------------------------------------------------------ the C entry
def test_header_ctypes_table_and_library_agree_on_the_scaled_entry_at_abi_6():
    from outfitx_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ofx.h")).read()
    decl = re.search(r"\bint ofx_adamw_step_scaled\s*\(([^;]*)\);", hdr)
    assert decl, "include/ofx.h does not declare ofx_adamw_step_scaled"
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]
    plain = re.search(r"\bint ofx_adamw_step\s*\(([^;]*)\);", hdr)
    plain_names = [a.split()[-1].lstrip("*") for a in plain.group(1).replace("\n", " ").split(",")]
    added = ["loss_scale", "growth_tracker", "growth_factor", "backoff_factor", "growth_interval"]
    assert [n for n in names if n not in added] == plain_names and [n for n in names if n in added] == added
    res, args = _lib.SIGNATURES["ofx_adamw_step_scaled"]
    assert len(args) == len(names) == len(_lib.SIGNATURES["ofx_adamw_step"][1]) + 5
    import ctypes as C
    i = names.index("loss_scale")
    assert args[i:i + 5] == [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int] and res is C.c_int
    assert int(re.search(r"#define OFX_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    lib = _lib.load()
    assert hasattr(lib, "ofx_adamw_step_scaled") and lib.ofx_abi_version() == 6


def test_scaled_engine_wrapper_and_optimizer_have_no_cpu_path():
    from outfitx_amd import _lib as L
    from outfitx_amd.engine import adamw_step_scaled
    from outfitx_amd.optim import FlatAdamW
    from outfitx_amd.trainer import FlatGrads
    z = torch.zeros(64)
    one, zi = torch.ones(()), torch.zeros((), dtype=torch.int32)
    with pytest.raises(L.OfxError):
        adamw_step_scaled(torch.zeros(1, 3, dtype=torch.int64), z, z.clone(), z.clone(), torch.zeros(()), 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 1.0,
                          one, zi, 2.0, 0.5, 2000, torch.zeros(()), zi.clone())
    with pytest.raises(L.OfxError):
        FlatAdamW(FlatGrads([torch.nn.Parameter(torch.zeros(8))]), lr=1e-3, loss_scaling=True)
