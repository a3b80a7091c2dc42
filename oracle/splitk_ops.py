"""Reference arithmetic of the split-K consumers (csrc/attention.hip set_attention_kernel's slab input, csrc/norm_act.hip
splitk_reduce_ln_kernel) - TEST INFRASTRUCTURE ONLY.

Both kernels promise a FIXED fp32 summation order, slab 0 + slab 1 + ... then the bias (then the residual): additions only, nothing a
compiler could contract, so numpy float32 reproduces them bit for bit (slab_sum).  The LayerNorm behind the reduce is judged against
float64 with a bound DERIVED from each row's float64 magnitudes (ln_bound), checked on the CPU against a float32 numpy LayerNorm
(ln_f32) by tests/test_cpu_attn_fwd_ref.py before any kernel meets it.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
U_OP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}          # unit roundoff of the operand types
ABS_OP = {"bf16": 0.0, "f16": 2.0 ** -25}              # half the spacing of f16's subnormals (bf16 shares fp32's exponent range)


def slab_sum(slabs, bias=None, resid=None):
    """(((s0 + s1) + ...) + bias) + resid in np.float32, one rounded addition after the other."""
    acc = np.array(slabs[0], np.float32, copy=True)
    for s in slabs[1:]:
        acc = acc + np.asarray(s, np.float32)
    if bias is not None:
        acc = acc + np.asarray(bias, np.float32)
    if resid is not None:
        acc = acc + np.asarray(resid, np.float32)
    assert acc.dtype == np.float32
    return acc


def cancelling_slabs(g, splits, shape, n_pairs=24):
    """Unit-normal fp32 slabs with a few pairs +a / -a of magnitude ~1e4 in two different slabs of the same element: any other summation
    order than the stated one leaves other bits there."""
    s = g.standard_normal((splits,) + tuple(shape), dtype=np.float32)
    if splits > 1:
        flat = s.reshape(splits, -1)
        for e in g.choice(flat.shape[1], n_pairs, replace=False):
            a, b = g.choice(splits, 2, replace=False)
            big = np.float32(1.0e4 * (1.0 + g.random()))
            flat[a, e] += big
            flat[b, e] -= big
    return s


def ln_ref(x, gamma, beta, eps):
    """float64 LayerNorm of the rows of x."""
    x, gamma, beta = (np.asarray(a, np.float64) for a in (x, gamma, beta))
    c = x - x.mean(-1, keepdims=True)
    return c / np.sqrt((c * c).mean(-1, keepdims=True) + eps) * gamma + beta


def ln_f32(x, gamma, beta, eps):
    """The same in np.float32, two passes (mean, then the variance of the centred row), numpy's own summation order."""
    x, gamma, beta = (np.asarray(a, np.float32) for a in (x, gamma, beta))
    D = np.float32(x.shape[-1])
    c = x - x.sum(-1, keepdims=True, dtype=np.float32) / D
    rstd = np.float32(1) / np.sqrt((c * c).sum(-1, keepdims=True, dtype=np.float32) / D + np.float32(eps))
    return c * rstd * gamma + beta


def ln_bound(x, gamma, beta, eps, out=None):
    """Per-element bound on |y_fp32 - ln_ref| of ANY two-pass fp32 LayerNorm of the fp32 rows x [rows, D], whatever its summation order, and
    with `out` = (dtype, kind) on the stored value as well (kind 1: y rounded to the operand type; kind 2: hi + lo).  u = 2^-24, first order
    in u with every constant rounded up, from the row's float64 quantities c = x - mean, sigma^2 = var + eps, y:
      mean    a sum of D terms in any order is off by <= (D - 1) u sum|x|; the multiplication by fl(1 / D) adds 2 u:
                  dmu = (D + 2) u mean|x|
      centre  t = fl(x - mu^) = c + d,  |d| <= dmu + u (|c| + dmu)
      var     sum t^2: the constant shift dmu enters the sum of squares only as D dmu^2 (sum c = 0), the roundings of t as 2 u; D positive
              terms summed in any order, products rounded or fused, <= (D + 1) u; / D, + eps: 3 u.  rsqrt halves the relative error and the
              device's rsqrtf adds <= 2 ulp:
                  rho = ((D + 6) u + dmu^2 / sigma^2) / 2 + 4 u
      y       fl(fl(fl(t rstd) g) + b), any of it fused: the product carries 2 u, the sum u |y|:
                  E32 = |g| / sigma (dmu + |c| (rho + 4 u)) + u (|y| + 2 |b|)          (|t rstd g| <= |y| + |b|)
      out     kind 1: + u_T (|y| + E32) + abs_T;   kind 2: lo = r(v - hi) with v - hi exact: + u_T^2 (|y| + E32) + abs_T,
              u_T = 2^-8 | 2^-11, abs_T = 2^-25 for f16's subnormals."""
    x, gamma, beta = (np.asarray(a, np.float64) for a in (x, gamma, beta))
    D = x.shape[-1]
    c = x - x.mean(-1, keepdims=True)
    sigma = np.sqrt((c * c).mean(-1, keepdims=True) + eps)
    y = c / sigma * gamma + beta
    dmu = (D + 2) * U32 * np.abs(x).mean(-1, keepdims=True)
    rho = ((D + 6) * U32 + (dmu / sigma) ** 2) / 2 + 4 * U32
    e32 = np.abs(gamma) / sigma * (dmu + np.abs(c) * (rho + 4 * U32)) + U32 * (np.abs(y) + 2 * np.abs(beta))
    if out is None:
        return e32
    dt, kind = out
    ut = U_OP[dt] if kind == 1 else U_OP[dt] ** 2
    return e32 + ut * (np.abs(y) + e32) + ABS_OP[dt]


def ln_inputs(D, splits, rows=37, seed=0):
    """Seeded inputs of the splitk_reduce_ln cases: slabs [splits, rows, D] (with cancelling pairs), bias, resid [rows, D], gamma, beta.  The
    rows have means up to a few standard deviations (row r is shifted by r / 8), so that the mean's error matters."""
    g = np.random.default_rng(4200 + D + 31 * splits + seed)
    slabs = cancelling_slabs(g, splits, (rows, D))
    slabs[0] += (np.arange(rows, dtype=np.float32) / np.float32(8))[:, None]
    bias = g.standard_normal(D, dtype=np.float32)
    resid = g.standard_normal((rows, D), dtype=np.float32)
    gamma = (1.0 + 0.25 * g.standard_normal(D)).astype(np.float32)
    beta = (0.5 * g.standard_normal(D)).astype(np.float32)
    return slabs, bias, resid, gamma, beta
