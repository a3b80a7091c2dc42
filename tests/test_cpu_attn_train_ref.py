"""The float64 reference of the training attention (oracle/attn_train.py) against float64 torch.autograd of the same
expression, on the CPU.  tests/test_gpu_attention_train.py holds the four training attention kernels to this reference,
block by block; the last test here shows on the emulation what that per-block criterion sees and a whole-tensor one does not."""
import numpy as np
import pytest
import torch

from oracle import attn_train as A

H, DH = 3, 64


def case(S, p, row0, seed=0):
    g = np.random.default_rng(1000 * S + 10 * int(p * 10) + row0 + seed)
    q, k, v, dO = (g.standard_normal((H, S, DH)) for _ in range(4))
    q[1] *= 4.0                                               # one peaked softmax
    mask = None if p == 0 else (g.random((H, S, S)) >= p) / (1.0 - p)
    if row0:
        dO[:, 1:] = 0.0
    return q, k, v, mask, dO


def autograd(q, k, v, mask, dO, scale):
    tq, tk, tv = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    P = torch.softmax(tq @ tk.transpose(-1, -2) * scale, -1)
    if mask is not None:
        P = P * torch.tensor(mask, dtype=torch.float64)
    O = P @ tv
    O.backward(torch.tensor(dO, dtype=torch.float64))
    return [t.detach().numpy() for t in (O, tq.grad, tk.grad, tv.grad)]


@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("S", [1, 2, 17, 32])
def test_reference_matches_float64_autograd(S, p, row0):
    q, k, v, mask, dO = case(S, p, row0)
    got = A.attn_train_ref(q, k, v, mask, dO, 0.125)
    want = autograd(q, k, v, mask, dO, 0.125)
    for name, a, b in zip("O dQ dK dV".split(), got, want):
        assert a.shape == b.shape == (H, S, DH) and a.dtype == np.float64
        scale = np.sqrt((b ** 2).sum((-1, -2)))
        err = np.sqrt(((a - b) ** 2).sum((-1, -2)))
        assert (err <= 1e-12 * scale).all(), (name, err, scale)         # per (head) block; a zero block must be zero
    if S == 1:                                                          # one key: the softmax is constant
        assert not got[1].any() and not got[2].any()
    if row0:
        assert not got[1][:, 1:].any()                                  # queries without an upstream gradient get no dQ


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("S", [1, 2, 17, 32])
def test_emulation_without_rounding_is_the_reference(S, p):
    q, k, v, mask, dO = case(S, p, 0, seed=5)
    for a, b in zip(A.attn_train_emul(q, k, v, mask, dO, 0.125, None), A.attn_train_ref(q, k, v, mask, dO, 0.125)):
        assert (A.block_err(a, b) <= 1e-14).all()


@pytest.mark.parametrize("dt,u", [("bf16", 2.0 ** -8), ("f16", 2.0 ** -11)])
def test_emulation_rounds_to_the_operand_type_and_stays_within_a_few_units_of_it(dt, u):
    q, k, v, mask, dO = case(17, 0.3, 0, seed=9)
    q, k, v = (A.round_to(a, dt) for a in (q, k, v))
    em = A.attn_train_emul(q, k, v, mask, dO, 0.125, dt)
    ref = A.attn_train_ref(q, k, v, mask, dO, 0.125)
    for a, b in zip(em, ref):
        assert np.array_equal(a, A.round_to(a, dt))
        e = A.block_err(a, b)
        assert (e > 0).all() and (e <= 4 * u).all(), e      # three roundings of relative size <= u / 2 .. u each on the way to an output
    assert A.block_err([[1.0]], [[0.0]]) == np.inf and A.block_err([[0.0]], [[0.0]]) == 0.0


@pytest.mark.parametrize("flaw,bad_set,whole_bound", [("tile", 0, None), ("row", 1, 5e-3)])
def test_per_block_criterion_sees_a_wrong_mask_index_that_a_whole_tensor_bound_does_not(flaw, bad_set, whole_bound):
    """The flaw the per-block test exists for, reproduced on the emulation (bf16, whose rounding error is the largest yardstick).  At
    NT = 2 the MFMA backward recomputes the dropout mask in its [query][key] orientation as query * 32 + key, query = 16u + 4q4 + r,
    key = 16t + r16.  Four 16-head sets of 32, 20, 31 and 17 rows; in ONE head of ONE set the tile (u = 0, t = 1) reads a wrong index:
      'tile': t and u swapped - the whole tile takes the mask of tile (u = 1, t = 0); set of 32 rows;
      'row' : the same swap for one (q4, r) only - one query row of the tile; set of 20 rows (4 live keys in the tile).
    dK and dV of that (set, head) are wrong, every other block is untouched.
      per block, e <= F max(e_emul, 1e-2 u) with the largest F the GPU test may use (3): exactly those two blocks fail - at 111x and
        134x the yardstick ('tile'), 4.0x and 7.2x ('row'), where 3x is allowed;
      whole tensor, ||dqkv - ref|| / ||ref|| over all sets, heads and the three gradients - the form of the whole-step criterion, which
        sees dqkv only summed into in_proj_weight.grad and asks 5e-3 (f16) or 3e-2 (bf16): 3.4e-2 ('tile': outside, but that test never
        ran NT = 2 with dropout), 3.3e-3 ('row': passes)."""
    Hh, lens, p, dt, u = 16, [32, 20, 31, 17], 0.3, "bf16", 2.0 ** -8
    g = np.random.default_rng(77)
    num = den = 0.0
    flagged = []
    for b, S in enumerate(lens):
        q, k, v = (A.round_to(g.standard_normal((Hh, S, DH)), dt) for _ in range(3))
        dO = g.standard_normal((Hh, S, DH))
        mask = (g.random((Hh, 32, 32)) >= p) / (1.0 - p)
        bad = mask.copy()
        if b == bad_set and flaw == "tile":
            bad[5, 0:16, 16:32] = mask[5, 16:32, 0:16]
        elif b == bad_set:
            bad[5, 7, 16:32] = mask[5, 23, 0:16]
        ref = A.attn_train_ref(q, k, v, mask[:, :S, :S], dO, 0.125)
        emul = A.attn_train_emul(q, k, v, mask[:, :S, :S], dO, 0.125, dt)
        got = A.attn_train_emul(q, k, v, mask[:, :S, :S], dO, 0.125, dt, mask_n=bad[:, :S, :S])
        for name, r_, e_, g_ in zip("O dQ dK dV".split(), ref, emul, got):
            ratio = A.block_err(g_, r_) / np.maximum(A.block_err(e_, r_), 1e-2 * u)
            for h in np.nonzero(ratio > 3.0)[0]:
                flagged.append((b, int(h), name))
                print(f"{flaw}: block {(b, int(h), name)} fails at {ratio[h]:.1f} x the yardstick")
            if name != "O":
                num += ((g_ - r_) ** 2).sum(); den += (r_ ** 2).sum()
    assert sorted(flagged) == [(bad_set, 5, "dK"), (bad_set, 5, "dV")]
    whole = np.sqrt(num / den)
    print(f"{flaw}: whole-tensor error {whole:.2e}")
    assert whole_bound is None or whole <= whole_bound
