"""Plain numpy reference of the GPU image preprocessor's ops (outfitx_amd/csrc/preprocess.hip, patchify_kernel), on top of np_oracle's
restatement of PIL's ImagingResample: the uint8 crop window, the normalised fp32 pixels for any mean / std, the patch-embedding GEMM's im2col
operand with its bf16 / f16 cast, and the figures the tests' claims rest on (window sizes, clamp events, the accumulators' bound).
tests/test_cpu_preprocess_ref.py pins all of it to PIL + CLIPImageProcessor's arithmetic and to torch's casts; tests/test_gpu_preprocess.py holds
the kernels to it bit for bit."""
import functools

import numpy as np

from . import np_oracle as O

PBITS = 22


@functools.lru_cache(maxsize=None)
def coeffs(in_size, out_size):
    """np_oracle.pil_bicubic_coeffs with the loop over the outputs vectorised (an axis of 57344 outputs, a sweep over 1200 lengths): the same
    float64 operations in the same order per output - the window sum runs tap by tap - hence the same integers, which
    tests/test_cpu_preprocess_ref.py asserts.  -> (kk int64 [out, ksize], bounds [out, 2] = (xmin, count))"""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < n[:, None]
    w = np.where(live, O._bicubic_filter(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size)
    for t in range(ksize):                # sequential, like the C loop; the dead taps add 0.0
        ww = ww + w[:, t]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    kk = np.where(w < 0, (-0.5 + w * (1 << PBITS)).astype(np.int64), (0.5 + w * (1 << PBITS)).astype(np.int64))
    return np.where(live, kk, 0), np.stack([xmin, n], 1)


def geometry(h, w, size):
    """CLIPImageProcessor: shortest edge -> size, centre crop -> (nw, nh, left, top)"""
    short, long_ = (w, h) if w <= h else (h, w)
    new_long = int(size * long_ / short)
    nw, nh = (size, new_long) if w <= h else (new_long, size)
    return nw, nh, (nw - size) // 2, (nh - size) // 2


def window_sizes(h, w, size):
    """(ksize_h, ksize_v): the coefficient row lengths of the horizontal (w -> nw) and vertical (h -> nh) pass; an axis PIL skips (in == out) is
    one tap of 2^22.  The horizontal figure, its maximum over a batch, selects resample_h_kernel<8> (<= 8), <16> (9 .. 16) or <0> (> 16)."""
    nw, nh, _, _ = geometry(h, w, size)
    return (1 if nw == w else coeffs(w, nw)[0].shape[1]), (1 if nh == h else coeffs(h, nh)[0].shape[1])


def accumulator_bound(in_size, out_size):
    """2^21 + 255 max_row sum |k|: no accumulator of a pass from in_size to out_size can exceed it in magnitude"""
    kk, _ = coeffs(in_size, out_size)
    return (1 << (PBITS - 1)) + 255 * int(np.abs(kk).sum(1).max())


def _pass_axis0(img, in_size, out_size, lo, n_out):
    """outputs [lo, lo + n_out) of the pass along axis 0 -> (acc >> 22 before the clamp, int64; the input rows [y0, y1) they read)"""
    if in_size == out_size:
        return img[lo:lo + n_out].astype(np.int64), (lo, lo + n_out)
    kk, b = coeffs(in_size, out_size)
    out = np.empty((n_out,) + img.shape[1:], np.int64)
    for i in range(n_out):
        xmin, n = b[lo + i]
        k = kk[lo + i, :n].reshape((-1,) + (1,) * (img.ndim - 1))
        out[i] = ((1 << (PBITS - 1)) + (img[xmin:xmin + n].astype(np.int64) * k).sum(0)) >> PBITS
    return out, (int(b[lo][0]), int(b[lo + n_out - 1].sum()))


def _two_passes(image, size):
    """the crop window only, as the kernels compute it -> (unclamped horizontal values [rows, size(, C)], unclamped vertical values [size, size(, C)])"""
    a = np.asarray(image)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    h, w = a.shape[:2]
    nw, nh, left, top = geometry(h, w, size)
    if nh == h:
        y0, y1 = top, top + size
    else:
        b = coeffs(h, nh)[1]
        y0, y1 = int(b[top][0]), int(b[top + size - 1].sum())
    hacc, _ = _pass_axis0(np.swapaxes(a[y0:y1], 0, 1), w, nw, left, size)
    hacc = np.swapaxes(hacc, 0, 1)
    inter = np.zeros((h, size) + a.shape[2:], np.uint8)               # rows outside [y0, y1) are never read
    inter[y0:y1] = np.clip(hacc, 0, 255).astype(np.uint8)
    vacc, rows = _pass_axis0(inter, h, nh, top, size)
    assert rows == (y0, y1)
    return hacc, vacc


def resized_u8(image, size):
    """uint8 [H, W] or [H, W, C] -> the size x size crop of PIL's antialiased BICUBIC resize, uint8, same channels"""
    return np.clip(_two_passes(image, size)[1], 0, 255).astype(np.uint8)


def clamp_events(image, size):
    """(horizontal, vertical): how many accumulators (per channel) of the passes that make the crop window fall outside [0, 255] before the clamp,
    with the number of accumulators of each pass -> ((events_h, total_h), (events_v, total_v))"""
    hacc, vacc = _two_passes(image, size)
    return tuple((int(((t < 0) | (t > 255)).sum()), int(t.size)) for t in (hacc, vacc))


def normalise(u8, mean, std):
    """uint8 [size, size] or [size, size, 3] -> fp32 [3, size, size] = (u8 * f32(1 / 255) - mean) / std, every operation rounded to fp32"""
    r = u8.astype(np.float32)
    if r.ndim == 2:
        r = np.repeat(r[:, :, None], 3, 2)
    m, s = (np.asarray(t, np.float32).reshape(3, 1, 1) for t in (mean, std))
    return (r.transpose(2, 0, 1) * np.float32(1 / 255.0) - m) / s


def pixels(images, size=224, mean=O.CLIP_MEAN, std=O.CLIP_STD):
    """np_oracle.clip_preprocess for any mean / std -> [N, 3, size, size] fp32"""
    return np.stack([normalise(resized_u8(a, size), mean, std) for a in images])


def bf16_bits(x):
    """fp32 -> the bf16 bits of round-to-nearest-even, by integer arithmetic on the bits (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def f16_bits(x):
    return np.ascontiguousarray(x, np.float32).astype(np.float16).view(np.uint16)


def cast_bits(x, dtype):
    return {"bf16": bf16_bits, "f16": f16_bits}[dtype](x)


def patch_operand(pixels_f32, patch, dtype):
    """[N, 3, S, S] fp32 -> uint16 bits [N (S / patch)^2, 3 patch^2]: row n g^2 + py g + px, column c patch^2 + ky patch + kx (Conv2d's
    weight.reshape(out, -1) order), each value rounded to nearest even in `dtype` ("bf16" | "f16")"""
    p = O.patchify(np.asarray(pixels_f32, np.float32), patch)
    return cast_bits(p.reshape(-1, p.shape[-1]), dtype)
