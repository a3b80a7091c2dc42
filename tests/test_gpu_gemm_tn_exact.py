"""The weight-gradient (TN) GEMM - gemm_tn_kernel's LDS image and transposed fragment reads, its two-stage rotation, the zero-filled
k-tail, the group_m walk with the split index peeled off the block id, the device-side k-partition of the live rows, the valid-extent
and accumulate stores of the direct epilogue and of the split-K reduce - on inputs for which every product and every partial sum is
exact in float32 (tests/gemm_tn_cases.py states the condition, tests/test_cpu_gemm_tn_exact.py checks it and that each case has the
plan and the partition it is in the table for).  The result then depends neither on the summation order nor on the split count, so
EVERY assertion here is bit equality: C[:m_valid, :n_valid] with the float64 product of the live rows (+ the prefill under
`accumulate`), the rest of C and its guard rows with what they held before, the sum of the slab planes with the same product, the
direct and the split launches of the same arrays - and the two entry points - with each other.  The slab is one plane longer than the
plan needs: the planes the plan owns come back finite, the extra one still NaN, which pins the split count that ran; and each plane
equals the product over the k-tiles that the documented partition of the live rows gives its split (an empty split: zeros), which pins
the partition that ran, not only its sum.

What stays with the tolerance tests (test_gpu_ops.py::test_gemm_tn_weight_gradient_kernel, test_gpu_bwd_ops.py::test_gemm_tn_into):
real-valued data."""
import numpy as np
import pytest
import torch

import gemm_tn_cases as T

pytestmark = pytest.mark.gpu

L = None
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
NAN32, GUARD32 = 0x7fc00000, 0x7fc0beef          # C's poison; the rows behind C (another NaN, so a read of them shows as well)
GUARD_ROWS = 2


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


def dev(a, td=None):
    t = torch.from_numpy(np.array(a)).cuda()                  # a copy: the case arrays are read-only
    return t if td is None else t.to(td).contiguous()


def bits(a):
    return a.view(np.int32)


def _mismatch(c, what, got, want):
    """None when got == want (as values: both are finite), else the message: count, first (m, n), the 256 x 256 tiles and the in-tile
    row / column box of the mismatches, and for a census case the digit strings (one binary digit per 32-deep k-step, step 0 first)."""
    bad = np.argwhere(got.astype(np.float64) != want)
    if bad.size == 0:
        return None
    m, n = bad[0]
    tiles = [tuple(int(x) for x in t) for t in np.unique(bad // 256, axis=0)]
    msg = (f"{c.name} [{what}; splits {c.splits}, k-tiles per split {c.parts}, partial tile {c.tail}]: {len(bad)} of {got.size} elements differ; "
           f"first at (m, n) = ({m}, {n}): got {got[m, n]!r}, want {want[m, n]!r}; tiles {tiles[:12]}{' ...' if len(tiles) > 12 else ''}; "
           f"in-tile rows {int((bad[:, 0] % 256).min())}..{int((bad[:, 0] % 256).max())}, columns {int((bad[:, 1] % 256).min())}..{int((bad[:, 1] % 256).max())}")
    if c.family == "census":
        msg += f"; census digits got {T.census_digits(float(got[m, n]), c)} want {T.census_digits(float(want[m, n]), c)}"
    return msg


def _launch(lib, c, d, t):
    """One launch of case c on the device operands t -> (C before, C after: int32 bits [m_valid + guard rows, ldc] on the host, errors)."""
    M, N, K = c.M, c.N, c.K
    mv = c.m_valid or M
    before = torch.empty((mv + GUARD_ROWS, c.ldc), dtype=torch.float32, device="cuda")
    before.view(torch.int32)[:mv] = NAN32
    before.view(torch.int32)[mv:] = GUARD32
    if c.accumulate:
        before[:mv] = dev(d["prefill"])
    out = before.clone()
    kd = None if c.kdev is None else torch.tensor([c.kdev], dtype=torch.int32, device="cuda")
    slab, nb = None, 0
    if c.slab:
        assert lib.ofx_gemm_tn_ws(M, N, K) == c.splits * M * N * 4, c.name                 # the plan the case names
        slab = torch.full((c.splits + 1, M, N), float("nan"), dtype=torch.float32, device="cuda")
        nb = slab.numel() * 4                                                              # the true size: one plane more than the plan needs
    args = (t["A"].data_ptr(), c.lda, t["B"].data_ptr(), c.ldb, out.data_ptr(), c.ldc, M, N, K, None if kd is None else kd.data_ptr())
    tail = (None if slab is None else slab.data_ptr(), nb, T.OP_DTYPE[c.dt], stream())
    if c.entry == "tn":
        rc = lib.ofx_gemm_tn(*args, *tail)
    else:
        rc = lib.ofx_gemm_tn_into(*args, c.m_valid, c.n_valid, c.accumulate, *tail)
    L.check(rc, c.name)
    torch.cuda.synchronize()
    errors = []
    if slab is not None:
        if not bool(torch.isfinite(slab[:c.splits]).all()):
            holes = [s for s in range(c.splits) if not bool(torch.isfinite(slab[s]).all())]
            errors.append(f"{c.name}: slab planes {holes} of {c.splits} were not written in full")
        if not bool(torch.isnan(slab[c.splits]).all()):
            errors.append(f"{c.name}: the plane behind the plan's {c.splits} was written")
        if not errors:
            planes = slab[:c.splits].cpu().numpy()
            total = planes.astype(np.float64).sum(0)
            msgs = [_mismatch(c, "sum of the slab planes", total, d["full"] if d["full"] is not None else d["want"])]
            # ... and each plane holds the k-tiles the kernel's partition of the LIVE rows gives its split, no others
            msgs += [_mismatch(c, f"slab plane {s}", planes[s], w) for s, w in enumerate(T.plane_wants(c, d))]
            errors += [m for m in msgs if m][:3]
    return bits(before.cpu().numpy()), bits(out.cpu().numpy()), errors


def _operands(c, d):
    return {"A": dev(d["A"], TD[c.dt]), "B": dev(d["B"], TD[c.dt])}


@pytest.mark.parametrize("group", list(T.GROUPS))
def test_gemm_tn_is_exact(group):
    lib = L.load()
    ops, first, errors = {}, {}, []
    for c in T.GROUPS[group]:
        d = T.build(c)
        mv, nv = c.m_valid or c.M, c.n_valid or c.N
        key = (c.family, c.M, c.N, c.K, d["live"], c.lda, c.ldb, c.dt)
        if key not in ops:
            ops.clear()                                       # one set of operands on the device at a time
            ops[key] = _operands(c, d)
        before, after, errs = _launch(lib, c, d, ops[key])
        errors += errs
        # nothing outside C[:m_valid, :n_valid] has changed: the columns from n_valid to ldc, the guard rows
        outside = np.ones(after.shape, bool)
        outside[:mv, :nv] = False
        if not np.array_equal(after[outside], before[outside]):
            r, col = np.argwhere(outside & (after != before))[0]
            errors.append(f"{c.name}: C was written outside [:{mv}, :{nv}], first at row {r}, column {col} (ldc {c.ldc})")
        got = after.view(np.float32)[:mv, :nv]
        if c.accumulate and d["live"] == 0 and not np.array_equal(after[:mv], before[:mv]):
            errors.append(f"{c.name}: no live row, yet C is not the prefill bit for bit")
        msg = _mismatch(c, "C", got, d["want"])
        if msg:
            errors.append(msg)
        # the same arrays: the same bits, direct or split, through either entry point
        same = first.setdefault(key + (mv, nv, c.ldc, c.accumulate), (c.name, after))
        if not np.array_equal(same[1], after):
            errors.append(f"{c.name}: not the bits of {same[0]}")
    assert not errors, "\n".join(errors)
