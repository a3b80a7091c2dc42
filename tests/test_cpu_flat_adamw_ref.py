"""The yardstick of tests/test_gpu_flat_adamw.py, pinned on the CPU: the float64 restatement of clip_grad_norm_ + AdamW
(tests/flat_adamw_ref.py) against torch itself, and torch's own fp32 distance from it in the error scales the GPU test uses."""
import numpy as np

import flat_adamw_ref as R


def test_restatement_equals_torch_in_float64():
    """(a) clip_grad_norm_ + torch.optim.AdamW on float64 tensors, four steps of the schedule (lr, beta1 and the gradient's scale change
    every step; only the last step is unclipped), tensors of 1, 5, 64, 1000, 4097 and 196608 elements: p, m, v and the norm to 1e-12."""
    assert R.SIZES == (1, 5, 64, 1000, 4097, 196608)
    assert [s for s in R.SCHEDULE] == [(8e-7, .95, 50.), (1.3e-5, .87, .01), (2e-5, .85, 1.), (1e-5, .9, .001)]
    for seed in R.SEEDS:
        got, want = R.torch_trajectory(seed, np.float64), R.restatement_trajectory(seed)
        for k, (s, r) in enumerate(zip(got, want)):
            clipped = r["norm64"] > R.MAX_NORM
            assert clipped == (k < 3), (k, r["norm64"])
            d = {q: float(np.abs(s[q] - r[q]).max()) for q in ("p", "m", "v")}
            dn = abs(s["norm"] - r["norm64"]) / r["norm64"]
            print(f"seed {seed} step {k + 1}: norm {r['norm64']:.6g} (rel {dn:.1e}), max|d| p {d['p']:.1e} m {d['m']:.1e} v {d['v']:.1e}")
            assert dn <= 1e-12 and all(x <= 1e-12 for x in d.values()), (seed, k, d, dn)


def test_torch_fp32_distance_from_the_restatement_is_what_the_gpu_bounds_assume():
    """(b) torch's fp32 CPU step against the restatement of the same step from torch's fp32 inputs: a few units of E_p, E_m, E_v (measured
    here over the three seeds: p 1.3, m 1.8, v 0.8, norm 1.5e-6).  Below 4 and 1e-5, so the yardstick cannot drift silently."""
    for seed in R.SEEDS:
        for k, e in enumerate(R.torch_fp32_ratios(seed)):
            print(f"seed {seed} step {k + 1}: p {e['p']:.2f} m {e['m']:.2f} v {e['v']:.2f} norm {e['norm']:.2e}")
            assert e["p"] < 4 and e["m"] < 4 and e["v"] < 4 and e["norm"] < 1e-5, (seed, k, e)
    print("worst over the seeds:", R.standard_bounds())
