"""What tests/test_gpu_preprocess.py rests on, checked without a GPU: the numpy reference (oracle/preprocess_ops.py over np_oracle's restatement
of PIL's resampler) equals the PIL + CLIPImageProcessor host pipeline bit for bit on every case of tests/preprocess_cases.py; the patch operand's
layout and casts are torch's; every case reaches the window bucket it claims, every "saturating" case drives both passes' accumulators outside
[0, 255], and no int32 accumulator can overflow."""
import numpy as np
import pytest
import torch
from PIL import Image

import preprocess_cases as PC
from oracle import np_oracle as O
from oracle import preprocess_ops as R
from outfitx_amd.encoders import clip_preprocess

TD = {"bf16": torch.bfloat16, "f16": torch.float16}


def torch_bits(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(TD[dt]).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("c", PC.CASES, ids=[c.name for c in PC.CASES])
def test_reference_equals_the_pil_pipeline(c):
    a = PC.image(c)
    want = clip_preprocess([Image.fromarray(a)], c.size).numpy()
    assert np.array_equal(R.pixels([a], c.size).view(np.uint32), want.view(np.uint32)), "oracle/preprocess_ops.pixels != PIL + CLIPImageProcessor"
    assert np.array_equal(R.resized_u8(a, c.size), PC.pil_u8(a, c.size)), "the uint8 crop window != PIL's"
    if max(R.geometry(c.h, c.w, c.size)[:2]) < 20000:     # np_oracle resizes the whole image in Python loops: not the 57344-long ones of 8 x 2048
        assert np.array_equal(O.clip_preprocess([a], c.size).view(np.uint32), want.view(np.uint32)), "np_oracle.clip_preprocess != PIL + CLIPImageProcessor"
    if c.channels == 1:                                   # grey == the same image replicated to RGB
        assert np.array_equal(R.pixels([np.repeat(a[:, :, None], 3, 2)], c.size), R.pixels([a], c.size))


def test_other_normalisations_are_numpy_arithmetic():
    """mean 0 / std 1 leaves float(u8) * f32(1 / 255); the CLIP constants give np_oracle's result; channels keep their own constants"""
    a = PC.image(PC.case(37, 53))
    u8 = R.resized_u8(a, 224)
    one = R.pixels([a], 224, (0, 0, 0), (1, 1, 1))[0]
    assert np.array_equal(one, u8.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0))
    assert np.array_equal(R.pixels([a], 224), O.clip_preprocess([a], 224))
    m, s = (0.1, 0.5, 0.9), (0.2, 0.3, 0.7)
    got = R.pixels([a], 224, m, s)[0]
    for ch in range(3):
        assert np.array_equal(got[ch], (u8[:, :, ch].astype(np.float32) * np.float32(1 / 255.0) - np.float32(m[ch])) / np.float32(s[ch]))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("size,patch", [(224, 32), (224, 16), (224, 7), (288, 32), (32, 8)])
def test_patch_operand_is_unfold_and_torch_cast(size, patch, dt):
    g = np.random.default_rng(size + patch)
    px = (g.standard_normal((2, 3, size, size)) * 1.5).astype(np.float32)
    cols = torch.nn.functional.unfold(torch.from_numpy(px), kernel_size=patch, stride=patch)          # [N, 3 p^2, g^2]: Conv2d's own im2col
    want = cols.transpose(1, 2).reshape(-1, 3 * patch * patch).to(TD[dt]).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.patch_operand(px, patch, dt), want)


def cast_sweep():
    """fp32 values around every rounding decision of the two casts: random bits, exact ties (both parities of the kept mantissa), their
    neighbours, results that are subnormal in f16, zero, and the values a normalised pixel can take"""
    g = np.random.default_rng(3)
    e = g.integers(100, 131, 6000).astype(np.uint32)                       # 2^-27 .. 2^3: f16 subnormal results lie below 2^-14
    sign = g.integers(0, 2, 6000).astype(np.uint32) << 31
    out = []
    for drop in (16, 13):                                                  # bits dropped: bf16, f16 normal
        kept = g.integers(0, 1 << (23 - drop), 6000).astype(np.uint32) << drop
        for low in (1 << (drop - 1), (1 << (drop - 1)) - 1, (1 << (drop - 1)) + 1, 0):
            out.append(sign | (e << 23) | kept | np.uint32(low))
    for ex in range(-27, -13):                                             # f16 subnormal results: ties sit at odd multiples of 2^-25
        out.append((np.arange(0, 2048, dtype=np.float64) * 2.0 ** -25 + 2.0 ** ex).astype(np.float32).view(np.uint32))
    out.append(g.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32))
    x = np.concatenate(out).view(np.float32)
    x = x[np.isfinite(x) & (np.abs(x) < 60000)]
    norm = ((np.arange(256, dtype=np.float32) * np.float32(1 / 255.0))[:, None] - np.asarray(O.CLIP_MEAN, np.float32)) / np.asarray(O.CLIP_STD, np.float32)
    return np.concatenate([x, -x, norm.ravel(), np.zeros(2, np.float32), -np.zeros(1, np.float32)])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_casts_are_torchs_on_ties_and_subnormals(dt):
    x = cast_sweep()
    got = R.cast_bits(x, dt)
    assert np.array_equal(got, torch_bits(x, dt))
    drop = 16 if dt == "bf16" else 13
    ties = (x.view(np.uint32) & np.uint32((1 << drop) - 1)) == np.uint32(1 << (drop - 1))
    assert ties.sum() > 5000, "the sweep holds exact ties"
    if dt == "f16":
        sub = (got & 0x7C00) == 0
        assert (sub & ((got & 0x3FF) != 0)).sum() > 5000, "the sweep holds subnormal f16 results"


def test_vectorised_coefficients_are_np_oracles():
    pairs = {(1, 224), (7, 224), (2, 336), (53, 317), (224, 225), (337, 224), (785, 224), (1100, 313), (2000, 570), (1030, 1024), (900, 288), (80, 32),
             (16384, 224), (8, 224), (2048, 1792)}
    pairs |= {(n, 224) for n in range(1, 1200, 37)}
    for a, b in sorted(pairs):
        (kk, bd), (kk0, bd0) = R.coeffs(a, b), O.pil_bicubic_coeffs(a, b)
        assert kk.shape == kk0.shape and np.array_equal(kk, kk0) and np.array_equal(bd, bd0), (a, b)


@pytest.mark.parametrize("c", [c for c in PC.CASES if c.bucket], ids=[c.name for c in PC.CASES if c.bucket])
def test_case_reaches_its_window_bucket(c):
    lo, hi = PC.BUCKETS[c.bucket]
    kh, kv = R.window_sizes(c.h, c.w, c.size)
    assert lo <= kh <= hi, (c.name, kh)
    if c.w <= c.h:                                        # w the shortest edge: the thresholds are 336 | 337 and 784 | 785 pixels
        assert (c.bucket == "8") == (c.w <= 336) and (c.bucket == "0") == (c.w >= 785)


def test_bucket_edges_and_geometry_claims():
    for edge, ksize in PC.BOUNDARY_WIDTHS.items():
        assert R.window_sizes(edge + 4, edge, 224)[0] == ksize and R.window_sizes(edge, edge, 224)[0] == ksize, edge
        # the planner's formula, restated: ksize = 2 ceil(2 max(in / out, 1)) + 1
        assert ksize == 2 * int(np.ceil(2.0 * max(edge / 224, 1.0))) + 1
    for (h, w), _, _ in PC.WINDOW_SHAPES:
        assert R.window_sizes(h, w, 224)[0] == R.coeffs(w, R.geometry(h, w, 224)[0])[0].shape[1]
    # w the long edge: its new length is truncated, the scale ends a little above h / 224, and an edge AT a threshold falls into the next bucket
    assert R.window_sizes(336, 400, 224)[0] == 9 and R.window_sizes(330, 400, 224)[0] == 7 and R.window_sizes(784, 790, 224)[0] == 17
    # identity plans: PIL skips the pass
    assert R.window_sizes(224, 224, 224) == (1, 1) and R.window_sizes(224, 500, 224)[1] == 1 and R.window_sizes(500, 224, 224)[0] == 1
    assert R.window_sizes(225, 224, 224) == (1, 1) and R.geometry(225, 224, 224) == (224, 225, 0, 0)      # 224 of 225 rows, nothing resampled
    # the mixed batch takes <0>; the early-return batch mixes 224 intermediate rows with several blocks more
    assert max(R.window_sizes(h, w, 224)[0] for (h, w) in [(340, 336), (340, 337), (790, 785), (224, 224)]) > 16
    (h, w) = PC.EARLY_RETURN_SHAPES[0]
    nw, nh, left, top = R.geometry(h, w, 224)
    b = R.coeffs(h, nh)[1]
    assert (b[top + 223].sum() - b[top][0] + 15) // 16 > 224 // 16 + 2
    # the crop windows of 8 x 2048 and 2048 x 8 start far from the origin
    assert R.geometry(8, 2048, 224)[2] > 20000 and R.geometry(2048, 8, 224)[3] > 20000
    # other sizes: 288 takes a second trip of the 256-column loops, 1024 four, 32 fills an eighth of a block
    assert [-(-s // 256) for s, _ in PC.OTHER_SIZES] == [1, 2, 2, 4]


@pytest.mark.parametrize("c", [c for c in PC.CASES if c.saturating], ids=[c.name for c in PC.CASES if c.saturating])
def test_saturating_cases_saturate_both_passes(c):
    (eh, th), (ev, tv) = R.clamp_events(PC.image(c), c.size)
    print(f"{c.name}: horizontal {eh / th:.3f}, vertical {ev / tv:.3f} of the accumulators leave [0, 255]")
    assert eh >= 0.01 * th and ev >= 0.01 * tv, (c.name, eh / th, ev / tv)
    u8 = R.resized_u8(PC.image(c), c.size)
    assert (u8 == 0).mean() > 0.05 and (u8 == 255).mean() > 0.05, "both clamp values are frequent in the result"


def test_accumulators_cannot_overflow():
    worst = 0
    for c in PC.CASES:
        nw, nh, _, _ = R.geometry(c.h, c.w, c.size)
        for a, b in ((c.w, nw), (c.h, nh)):
            if a != b:
                worst = max(worst, R.accumulator_bound(a, b))
                assert R.accumulator_bound(a, b) < 2 ** 31, (c.name, a, b)
    for n in list(range(1, 1200)) + [2048, 4000, 16384]:
        bound = R.accumulator_bound(n, 224)
        worst = max(worst, bound)
        assert bound < 2 ** 31, n
    print(f"worst 2^21 + 255 max_row sum |k| = {worst / 2 ** 31:.3f} * 2^31")
    assert worst <= 0.64 * 2 ** 31
