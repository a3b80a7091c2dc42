"""Yardstick of the loss-scaled optimizer step (ofx_adamw_step_scaled): torch.amp.GradScaler's state machine and its unscale_ restated in
numpy on top of tests/flat_adamw_ref.py.  Tests only: nothing under outfitx_amd/ imports this file.

    arena = loss_scale * gradient  ->  g = arena * (grad_scale / loss_scale);  everything of flat_adamw_ref.ref_step on that g
    the step was skipped (norm not finite):  scale *= backoff;  tracker = 0
    otherwise:                               tracker += 1;  tracker == interval:  scale *= growth (if that is finite);  tracker = 0

The scale is a float32 and its products are formed in float64 and rounded once, as torch's _amp_update_scale_ forms them
(tests/test_cpu_loss_scale.py holds `scaler_update` to torch.amp.GradScaler('cpu') over found-inf patterns).
"""
import numpy as np
import torch

import flat_adamw_ref as R

INIT_SCALE, GROWTH, BACKOFF, INTERVAL = 65536.0, 2.0, 0.5, 2000          # torch.amp.GradScaler()'s defaults


def scaler_update(scale, tracker, found_inf, growth=GROWTH, backoff=BACKOFF, interval=INTERVAL):
    """GradScaler.update() -> (scale as a Python float holding a float32 value, tracker)."""
    scale = np.float32(scale)
    if found_inf:
        return float(np.float32(np.float64(scale) * backoff)), 0
    tracker = int(tracker) + 1
    if tracker == interval:
        with np.errstate(over="ignore"):
            up = np.float32(np.float64(scale) * growth)
        return float(up if np.isfinite(up) else scale), 0
    return float(scale), tracker


def scaler_trajectory(found_infs, init_scale=INIT_SCALE, growth=GROWTH, backoff=BACKOFF, interval=INTERVAL):
    """[(scale, tracker)] after every update of a scaler that starts at (init_scale, 0)."""
    s, t, out = float(np.float32(init_scale)), 0, []
    for f in found_infs:
        s, t = scaler_update(s, t, f, growth, backoff, interval)
        out.append((s, t))
    return out


def torch_scaler_trajectory(found_infs, init_scale=INIT_SCALE, growth=GROWTH, backoff=BACKOFF, interval=INTERVAL):
    """The same from a real torch.amp.GradScaler('cpu') driven through scale / unscale_ / step / update on one parameter, whose gradient is
    the scale itself (finite) or inf."""
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=0.1)
    sc = torch.amp.GradScaler("cpu", init_scale=init_scale, growth_factor=growth, backoff_factor=backoff, growth_interval=interval)
    out = []
    for f in found_infs:
        sc.scale((p * 1.0).sum()).backward()
        if f:
            p.grad[1] = float("inf")
        sc.unscale_(opt)
        sc.step(opt)
        sc.update()
        opt.zero_grad()
        sd = sc.state_dict()
        out.append((float(sd["scale"]), int(sd["_growth_tracker"])))
    return out


def ref_step_scaled(p, m, v, g_scaled, t_old, lr, beta1, scale, tracker, grad_scale=1.0, norm=None, growth=GROWTH, backoff=BACKOFF,
                    interval=INTERVAL, **kw):
    """One scaled step in float64: flat_adamw_ref.ref_step on g_scaled * (grad_scale / scale), then the scaler's update.  norm: the
    UNSCALED norm the clip coefficient is defined from (None: the float64 one).  -> ref_step's dict + 'scale', 'tracker'."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = R.ref_step(p, m, v, g_scaled, t_old, lr, beta1, grad_scale=np.float64(grad_scale) / np.float64(np.float32(scale)), norm=norm, **kw)
    r["scale"], r["tracker"] = scaler_update(scale, tracker, r["skipped"], growth, backoff, interval)
    return r
