"""The named inputs of the image preprocessor's op-level tests, with fixed seeds: tests/test_cpu_preprocess_ref.py checks on the reference what
each case claims (pipeline equality with PIL, its window bucket, that it saturates), tests/test_gpu_preprocess.py runs the same bytes through
the kernels.  Shapes are (h, w)."""
import collections
import functools
import zlib

import numpy as np

Case = collections.namedtuple("Case", "name h w channels size kind block bucket saturating")

# resample_h_kernel's instantiation is chosen by the widest horizontal window of the batch: "8" = ksize <= 8, "16" = 9 .. 16, "0" = wider
BUCKETS = {"8": (1, 8), "16": (9, 16), "0": (17, 1 << 30)}
# (h, w), bucket, block size of the saturating pattern: 5 px up to a shortest edge of 336, 8 px up to 784, 16 .. 24 px above
# The window is set by w / nw, and the LONG edge's new length is truncated to an integer: with w the shortest edge the scale is w / 224 exactly,
# with w the long edge it is a little above h / 224 - 336 x 400 resizes to 266 columns, 400 / 266 = 1.504 > 1.5, and takes 9 taps, not 7.
WINDOW_SHAPES = [((340, 336), "8", 5), ((330, 400), "8", 5), ((336, 400), "16", 5), ((340, 337), "16", 8), ((790, 784), "16", 8),
                 ((790, 785), "0", 16), ((785, 1100), "0", 20), ((2000, 785), "0", 24)]
BOUNDARY_WIDTHS = {336: 7, 337: 9, 784: 15, 785: 17}              # shortest edge at size 224 -> ksize_h
SMALL_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (37, 53),          # fewer pixels than taps, odd sizes
                (224, 224), (224, 500), (500, 224), (225, 224),    # the identity plan on both axes, on one, next to one
                (8, 2048), (2048, 8)]                              # crop windows far from the origin
EARLY_RETURN_SHAPES = [(2000, 300), (224, 224)]
GREY_SHAPES = [((300, 451), "8", 5), ((340, 337), "16", 8), ((790, 785), "0", 16)]
OTHER_SIZES = [(32, (100, 80)), (288, (400, 300)), (288, (900, 1000)), (1024, (1100, 1030))]
PATCH_SHAPES = [(37, 53), (340, 337), (224, 224), (100, 80), (500, 224)]     # the N = 5 batch of the patch-operand tests (N = 1: the second)
PATCH_GRIDS = [(224, 32), (224, 16), (224, 7), (288, 32), (32, 8)]           # (size, patch)


def _name(h, w, channels, size, kind):
    return f"{'rgb' if channels == 3 else 'grey'}-{h}x{w}-s{size}-{kind}"


def _cases():
    out = []
    for (h, w), bucket, block in WINDOW_SHAPES:
        out.append(Case(_name(h, w, 3, 224, "noise"), h, w, 3, 224, "noise", 0, bucket, False))
        out.append(Case(_name(h, w, 3, 224, "blocks"), h, w, 3, 224, "blocks", block, bucket, True))
    for (h, w) in SMALL_SHAPES + EARLY_RETURN_SHAPES[:1]:
        out.append(Case(_name(h, w, 3, 224, "noise"), h, w, 3, 224, "noise", 0, None, False))
    for (h, w), bucket, block in GREY_SHAPES:
        out.append(Case(_name(h, w, 1, 224, "noise"), h, w, 1, 224, "noise", 0, bucket, False))
        out.append(Case(_name(h, w, 1, 224, "blocks"), h, w, 1, 224, "blocks", block, bucket, True))
    for size, (h, w) in OTHER_SIZES:
        out.append(Case(_name(h, w, 3, size, "noise"), h, w, 3, size, "noise", 0, None, False))
    for size in sorted({s for s, _ in PATCH_GRIDS}):
        for (h, w) in PATCH_SHAPES:
            for ch in (3, 1):
                if not any(c.name == _name(h, w, ch, size, "noise") for c in out):
                    out.append(Case(_name(h, w, ch, size, "noise"), h, w, ch, size, "noise", 0, None, False))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def case(h, w, channels=3, size=224, kind="noise"):
    return BY_NAME[_name(h, w, channels, size, kind)]


def noise(h, w, channels, seed):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, channels), dtype=np.uint8)
    return a if channels == 3 else a[:, :, 0]


def blocks(h, w, channels, block):
    """hard edges in every channel: a black / white checkerboard in R, its inverse in G, column stripes in B (grey: the checkerboard)"""
    y, x = np.arange(h)[:, None] // block, np.arange(w)[None, :] // block
    r = (((y + x) & 1) * 255).astype(np.uint8)
    if channels == 1:
        return r
    return np.ascontiguousarray(np.stack([r, 255 - r, np.broadcast_to(((x & 1) * 255).astype(np.uint8), (h, w))], 2))


@functools.lru_cache(maxsize=None)
def _image(name):
    c = BY_NAME[name]
    a = noise(c.h, c.w, c.channels, zlib.crc32(name.encode())) if c.kind == "noise" else blocks(c.h, c.w, c.channels, c.block)
    a.setflags(write=False)
    return a


def image(c):
    """uint8 [h, w, 3] or [h, w] (grey), read-only; the same bytes on every call"""
    return _image(c.name)


def pil_u8(a, size):
    """PIL's own result for the resize + centre crop of CLIPImageProcessor: uint8 [size, size(, 3)]"""
    from PIL import Image
    im = Image.fromarray(np.asarray(a))
    w, h = im.size
    short, long_ = (w, h) if w <= h else (h, w)
    new_long = int(size * long_ / short)
    nw, nh = (size, new_long) if w <= h else (new_long, size)
    if (nw, nh) != (w, h):
        im = im.resize((nw, nh), resample=Image.BICUBIC)
    left, top = (nw - size) // 2, (nh - size) // 2
    return np.asarray(im.crop((left, top, left + size, top + size)))
