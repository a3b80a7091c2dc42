"""Yardstick of the fused optimizer step (ofx_adamw_step): a float64 numpy restatement of torch.nn.utils.clip_grad_norm_ followed by
torch.optim.AdamW (amsgrad off, maximize off), the error scales its results are measured in, and torch's own fp32 distance from it.
Tests only: nothing under outfitx_amd/ imports this file.

    g = grad_scale * grad;  norm = ||g||_2;  norm not finite -> skipped, gradient dropped, nothing else moves
    t = t_old + 1;  g_c = g * min(max_norm / (norm + 1e-6), 1);  p *= 1 - lr wd
    m = m + (g_c - m)(1 - b1);  v = b2 v + (1 - b2) g_c g_c;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Error scales (one fp32 evaluation of the step loses a few of these whatever its order of operations):
    E_p = ulp32(p_ref) + 2^-22 lr (|m_old| + |g_c|) / ((1 - b1^t) denom_ref)      the stored parameter's own rounding + the update's
    E_m = 2^-23 (|m_old| + |g_c|)                                                 the roundings of g_c, of g_c - m and of the sum
    E_v = 2^-22 v_ref + 4e-9 g_c^2                                                beta2's fp32 image and the sum + (1 - b2) g_c^2's roundings
"""
import functools

import numpy as np
import torch

SIZES = (1, 5, 64, 1000, 4097, 196608)
# (lr, beta1, scale of the standard-normal gradient): the norm is scale * sqrt(201775) = 449 * scale, so only the last step is unclipped
SCHEDULE = ((8e-7, .95, 50.), (1.3e-5, .87, .01), (2e-5, .85, 1.), (1e-5, .9, .001))
BETA2, EPS, WD, MAX_NORM = 0.999, 1e-8, 0.01, 1.0
SEEDS = (0, 1, 2)


def make_problem(seed, sizes=SIZES, steps=len(SCHEDULE), scales=None):
    """-> (p0 fp32 [sum(sizes)], [steps] fp32 gradients): the tensors of `sizes` laid end to end, no padding."""
    g = np.random.default_rng(1000 + seed)
    n = int(sum(sizes))
    scales = [s[2] for s in SCHEDULE] if scales is None else scales
    p0 = (g.standard_normal(n) * 0.05).astype(np.float32)
    return p0, [(g.standard_normal(n) * sc).astype(np.float32) for sc in scales[:steps]]


def ref_step(p, m, v, g, t_old, lr, beta1, beta2=BETA2, eps=EPS, wd=WD, max_norm=MAX_NORM, grad_scale=1.0, norm=None):
    """One step in float64 from the given inputs (any float dtype).  norm: the value the clip coefficient is defined from (None: the
    float64 norm of grad_scale * g).  -> dict p, m, v, norm64, t, skipped and the pieces the error scales need."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    g = g * np.float64(grad_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        norm64 = float(np.sqrt((g * g).sum()))
    nrm = norm64 if norm is None else float(norm)
    if not np.isfinite(nrm):
        return {"p": p, "m": m, "v": v, "norm64": norm64, "t": t_old, "skipped": 1}
    t = int(t_old) + 1
    gc = g * min(max_norm / (nrm + 1e-6), 1.0)
    p1 = p * (1.0 - lr * wd)
    m1 = m + (gc - m) * (1.0 - beta1)
    v1 = beta2 * v + (1.0 - beta2) * gc * gc
    denom = np.sqrt(v1) / np.sqrt(1.0 - beta2 ** t) + eps
    p1 = p1 - (lr / (1.0 - beta1 ** t)) * m1 / denom
    return {"p": p1, "m": m1, "v": v1, "norm64": norm64, "t": t, "skipped": 0, "gc": gc, "m_old": m, "denom": denom, "lr": lr, "bc1": 1.0 - beta1 ** t}


def error_ratios(p, m, v, ref):
    """max over ALL elements of |got - ref| / E for p, m, v (the module docstring's scales) -> dict."""
    a = np.abs(ref["m_old"]) + np.abs(ref["gc"])
    e_p = np.spacing(np.abs(ref["p"]).astype(np.float32)).astype(np.float64) + 2.0 ** -22 * ref["lr"] * a / (ref["bc1"] * ref["denom"])
    e_m = 2.0 ** -23 * a
    e_v = 2.0 ** -22 * ref["v"] + 4e-9 * ref["gc"] ** 2
    out = {}
    for k, got, e in (("p", p, e_p), ("m", m, e_m), ("v", v, e_v)):
        d = np.abs(np.asarray(got, np.float64) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0, 0.0, d / e)
        out[k] = float(r.max())
    return out


def _split(flat, sizes, dtype):
    o, out = 0, []
    for n in sizes:
        out.append(torch.from_numpy(np.array(flat[o:o + n], dtype)))
        o += n
    return out


def _cat(ts):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ts])


def torch_trajectory(seed, dtype, sizes=SIZES):
    """clip_grad_norm_ + torch.optim.AdamW on the CPU in `dtype` over the schedule.  Yields, per step, (inputs p, m, v, g as torch saw
    them, t_old, hyper-parameters, the norm clip_grad_norm_ returned, outputs p, m, v)."""
    p0, grads = make_problem(seed, sizes)
    params = [torch.nn.Parameter(t) for t in _split(p0, sizes, dtype)]
    opt = torch.optim.AdamW(params, lr=SCHEDULE[0][0], betas=(SCHEDULE[0][1], BETA2), eps=EPS, weight_decay=WD)
    out = []
    for k, (lr, b1, _) in enumerate(SCHEDULE):
        opt.param_groups[0]["lr"], opt.param_groups[0]["betas"] = lr, (b1, BETA2)
        for q, gq in zip(params, _split(grads[k], sizes, dtype)):
            q.grad = gq
        zeros = np.zeros_like(p0, dtype)
        m_in = _cat([opt.state[q]["exp_avg"] for q in params]) if k else zeros
        v_in = _cat([opt.state[q]["exp_avg_sq"] for q in params]) if k else zeros
        p_in, g_in = _cat(params), _cat([q.grad for q in params])
        norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
        out.append({"p_in": p_in, "m_in": m_in, "v_in": v_in, "g_in": g_in, "t_old": k, "lr": lr, "beta1": b1, "norm": norm.item(),
                    "p": _cat(params), "m": _cat([opt.state[q]["exp_avg"] for q in params]), "v": _cat([opt.state[q]["exp_avg_sq"] for q in params])})
    return out


def restatement_trajectory(seed, sizes=SIZES):
    """The restatement over the schedule in float64 from the same start -> per-step dicts of ref_step."""
    p0, grads = make_problem(seed, sizes)
    p, m, v = p0.astype(np.float64), np.zeros(len(p0)), np.zeros(len(p0))
    out = []
    for k, (lr, b1, _) in enumerate(SCHEDULE):
        r = ref_step(p, m, v, grads[k], k, lr, b1)
        p, m, v = r["p"], r["m"], r["v"]
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def torch_fp32_ratios(seed, sizes=SIZES):
    """(b): per step, how far torch's fp32 CPU clip_grad_norm_ + AdamW lands from the restatement of that same step taken from torch's
    own fp32 inputs and the fp32 norm it clipped with -> tuple of dicts {p, m, v (units of E), norm (relative deviation of the fp32
    norm from the float64 one)}."""
    out = []
    for s in torch_trajectory(seed, np.float32, sizes):
        r = ref_step(s["p_in"], s["m_in"], s["v_in"], s["g_in"], s["t_old"], s["lr"], s["beta1"], norm=s["norm"])
        e = error_ratios(s["p"], s["m"], s["v"], r)
        e["norm"] = abs(s["norm"] - r["norm64"]) / r["norm64"]
        out.append(e)
    return tuple(out)


def torch_worst(seed):
    """Worst of (b) over the schedule's steps for one seed -> dict p, m, v, norm."""
    rs = torch_fp32_ratios(seed)
    return {k: max(r[k] for r in rs) for k in ("p", "m", "v", "norm")}


def standard_bounds():
    """Worst of (b) over the three seeds -> dict; for checks on inputs other than the schedule's."""
    ws = [torch_worst(s) for s in SEEDS]
    return {k: max(w[k] for w in ws) for k in ("p", "m", "v", "norm")}
