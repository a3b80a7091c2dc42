"""Op-level exact tests of the GPU image preprocessor on a real MI355X, through the C ABI (ctypes): ofx_clip_preprocess (fp32 pixels),
ofx_clip_preprocess_patches (the patch-embedding GEMM's im2col operand, written by the vertical pass) and ofx_patchify (the pixel route's
counterpart), outfitx_amd/csrc/preprocess.hip and patchify_kernel.

Reference: oracle/preprocess_ops.py (plain numpy over np_oracle's restatement of PIL's ImagingResample), pinned by
tests/test_cpu_preprocess_ref.py to PIL + CLIPImageProcessor's arithmetic bit for bit on every case of tests/preprocess_cases.py, which also asserts
each case's window bucket, that every "blocks" case drives >= 1 % of both passes' accumulators outside [0, 255], and that no int32 accumulator
can overflow.  EVERY comparison here is bit equality: there is no tolerance in this file.  Every output (fp32 pixels, patches, workspace) is
poisoned - a payload NaN, a byte pattern - and followed by guard bytes whose bits are checked; the workspace passed is exactly
ofx_clip_preprocess_ws bytes; every op is called twice and must return the same bits.  The source buffer ends 4 bytes past the last image (the
slack the header asks for), filled with 0xA5.

WHICH KERNEL EACH CASE REACHES.  The profile records carry no kernel kind for this op (category "other"), so the instantiation of the
horizontal pass rests on the ksize assertions of the CPU test: the batch's widest horizontal window picks resample_h_kernel<8> (ksize <= 8),
<16> (9 .. 16) or <0> (wider, and every grey batch).  Shapes are (h, w).
  test_window_buckets: RGB, size 224, single-image batches, noise and a saturating block pattern each: (340, 336), (330, 400) -> <8> (ksize 7);
    (336, 400), (340, 337) -> <16> (9), (790, 784) -> <16> (15); (790, 785), (785, 1100), (2000, 785) -> the RGB branch of <0> (17).  336 | 337 and
    784 | 785 are the bucket edges when w is the shortest edge; when w is the long edge its new length is truncated and 336 x 400 (266 columns,
    scale 1.504) already takes 9 taps; (330, 400) is the landscape <8> case.
  test_mixed_batch: one image per bucket + (224, 224) in one batch: all through <0>, each equal to its single-batch bits.
  test_small_shapes_and_geometry_edges: (1, 1) .. (37, 53) (fewer pixels than taps, clamped tap addresses of <8>), identity plans (one tap of 2^22)
    on one or both axes, (8, 2048) / (2048, 8) (crop windows 28560 outputs from the origin), (2000, 300) + (224, 224): blocks past the short
    image's rows take the early return.
  test_grey: channels = 1 -> the grey branch of <0> at ksize 7 / 9 / 17, against the 2-D oracle and against the channels = 3 run of the replicated image.
  test_other_sizes: size 32 (an eighth of a block), 288 (second trip of both passes' column loops), 1024 (four trips).
  test_patch_operand: resample_v_kernel<bf16_t> / <f16_t>, size / patch 224 / 32, 224 / 16, 224 / 7, 288 / 32, 32 / 8, N = 1 and 5, channels 3 and 1;
    test_patchify: patchify_kernel<bf16_t> / <f16_t> on values around every rounding decision, and once past the launcher's cap of 32768 blocks
    (the grid-stride loop's second trip).
  test_normalisation, test_input_contract, test_host_state, test_refused_calls: see their docstrings.

MEASURED on the MI355X.  First run: every comparison with the kernels exact, every guard intact, every pair of calls equal to the bit - all
three instantiations of the horizontal pass in both RGB and grey form, both operand casts, sizes 32 .. 1024, the six calls in flight and the
runs after the plan cache's eviction.  No kernel or planning bug was found; the two failures of the first runs were the tests' own (channels
compared after a per-channel normalisation; an offset rule that produced even offsets) and are fixed here.  The whole file takes 5 s.
That the tests can fail: six mutations of preprocess.hip, each built aside and run against the one test named: no rounding term in the RGB branch
of <0> -> test_window_buckets[rgb-790x785-s224-noise] (75,057 of 150,528 values differ); no zeroing of the taps past a column's count in the
register branch -> test_window_buckets[rgb-340x336-s224-noise] (133,282); no clamp in the horizontal pass -> test_window_buckets[rgb-340x336-s224-blocks]
(64,484); q[pp] and q[2 pp] swapped in the patch store -> test_patch_operand[224-32-3] (100,248); the grey branch's second channel from px[x + 1] ->
test_grey[grey-300x451-s224-noise] (49,796); mul_then_sub as one fma -> test_normalisation (79,724; mean 0 / std 1 alone does not see it, the
first non-CLIP pair does).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import preprocess_cases as PC
from oracle import np_oracle as O
from oracle import preprocess_ops as R

pytestmark = pytest.mark.gpu

OFX_EINVAL, OFX_ESHAPE, OFX_EWORKSPACE = -1, -2, -4
DT = {"bf16": 1, "f16": 2}
NAN32 = 0x7FC0BEEF
NANOP = {"bf16": 0x7FC5, "f16": 0x7E05}
GUARD32, GUARD16, GUARD8, WS_POISON, SLACK = 0x5AA55AA5, 0x5AA5, 0x5A, 0xCD, 0xA5
GUARD = 256                          # guard elements after every output, guard bytes after the workspace
I, LL = C.POINTER(C.c_int), C.POINTER(C.c_longlong)

L = None


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


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


def as_u16(t):
    return t.cpu().numpy().view(np.uint16)


def pack(images, offsets=None, fill=SLACK):
    """-> (device uint8 buffer: the images' bytes at `offsets` (default: back to back from 0, no alignment), `fill` between them and in the 4 bytes
    of slack after the last, offsets, heights, widths)"""
    flat = [np.ascontiguousarray(a).reshape(-1) for a in images]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([f.size for f in flat])[:-1]])
    offsets = np.asarray(offsets, np.int64)
    buf = np.full(int(max(o + f.size for o, f in zip(offsets, flat))) + 4, fill, np.uint8)
    for o, f in zip(offsets, flat):
        buf[o:o + f.size] = f
    hs = np.array([a.shape[0] for a in images], np.int32)
    ws = np.array([a.shape[1] for a in images], np.int32)
    return torch.from_numpy(buf).cuda(), offsets, hs, ws


class Call:
    """One ofx_clip_preprocess / ofx_clip_preprocess_patches call with poisoned, guarded buffers.  launch() only enqueues; check() synchronises,
    checks the guards and that nothing of the output kept its poison, and returns the output's bits (uint32 [N, 3, size, size] or uint16 rows)."""

    def __init__(self, images, size=224, mean=O.CLIP_MEAN, std=O.CLIP_STD, patch=0, dt=None, offsets=None, fill=SLACK):
        lib = L.load()
        self.channels = 3 if np.asarray(images[0]).ndim == 3 else 1
        self.src, self.offs, self.hs, self.ws_ = pack(images, offsets, fill)
        self.N, self.size, self.patch, self.dt = len(images), size, patch, dt
        self.mean, self.std = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        self.n_out = self.N * 3 * size * size
        self.ws_bytes = int(lib.ofx_clip_preprocess_ws(self.hs.ctypes.data_as(I), self.ws_.ctypes.data_as(I), self.N, self.channels, size))
        assert self.ws_bytes > 0
        self.ws = torch.full((self.ws_bytes + GUARD,), WS_POISON, dtype=torch.uint8, device="cuda")
        self.ws[self.ws_bytes:] = GUARD8
        if dt is None:
            self.out = torch.full((self.n_out + GUARD,), NAN32, dtype=torch.int32, device="cuda")
            self.out[self.n_out:] = GUARD32
        else:
            self.out = torch.full((self.n_out + GUARD,), NANOP[dt], dtype=torch.int16, device="cuda")
            self.out[self.n_out:] = GUARD16
        assert self.ws.data_ptr() % 256 == 0 and self.out.data_ptr() % 16 == 0

    def launch(self):
        lib = L.load()
        a = (self.src.data_ptr(), self.offs.ctypes.data_as(LL), self.hs.ctypes.data_as(I), self.ws_.ctypes.data_as(I), self.N, self.channels, self.size)
        if self.dt is None:
            rc = lib.ofx_clip_preprocess(*a, self.mean, self.std, self.out.data_ptr(), self.ws.data_ptr(), self.ws_bytes, stream())
        else:
            rc = lib.ofx_clip_preprocess_patches(*a, self.patch, self.mean, self.std, self.out.data_ptr(), DT[self.dt], self.ws.data_ptr(), self.ws_bytes, stream())
        L.check(rc, "ofx_clip_preprocess")
        return self

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.ws[self.ws_bytes:] == GUARD8).all()), "the workspace's guard bytes"
        if self.dt is None:
            assert bool((self.out[self.n_out:] == GUARD32).all()), "the output's guard"
            got = as_u32(self.out[:self.n_out]).reshape(self.N, 3, self.size, self.size)
            assert not (got == NAN32).any(), "an output element kept its poison"
            return got
        assert bool((self.out[self.n_out:] == GUARD16).all()), "the output's guard"
        got = as_u16(self.out[:self.n_out]).reshape(-1, 3 * self.patch * self.patch)
        assert not (got == NANOP[self.dt]).any(), "an output element kept its poison"
        return got


def run(images, **kw):
    """the op twice, on fresh poisoned buffers: the same bits -> the bits"""
    a, b = Call(images, **kw).launch().check(), Call(images, **kw).launch().check()
    assert np.array_equal(a, b), "two calls, two results"
    return a


@functools.lru_cache(maxsize=None)
def ref_bits(name, mean=O.CLIP_MEAN, std=O.CLIP_STD):
    """the oracle's pixels of one case, computed once: uint32 [3, size, size]"""
    c = PC.BY_NAME[name]
    r = R.pixels([PC.image(c)], c.size, mean, std)[0].view(np.uint32)
    r.setflags(write=False)
    return r


def mismatch(got, want):
    bad = got != want
    return f"{int(bad.sum())} of {bad.size} differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}" if bad.any() else "equal"


def check_case(c):
    got = run([PC.image(c)], size=c.size)
    assert np.array_equal(got[0], ref_bits(c.name)), (c.name, mismatch(got[0], ref_bits(c.name)))
    return got[0]


# ------------------------------------------------------------------------------------------------ window buckets
WINDOW_CASES = [PC.case(h, w, kind=k) for (h, w), _, _ in PC.WINDOW_SHAPES for k in ("noise", "blocks")]


@pytest.mark.parametrize("c", WINDOW_CASES, ids=[c.name for c in WINDOW_CASES])
def test_window_buckets(c):
    """resample_h_kernel<8>, <16> and the RGB branch of <0>, at both edges of each bucket; noise, and hard black / white edges that push both
    passes' accumulators through the clamps and the 8-bit intermediate."""
    got = check_case(c)
    if c.saturating:
        vals = got.view(np.float32)
        black = ((np.float32(0) * np.float32(1 / 255.0) - np.asarray(O.CLIP_MEAN, np.float32)) / np.asarray(O.CLIP_STD, np.float32)).reshape(3, 1, 1)
        white = ((np.float32(255) * np.float32(1 / 255.0) - np.asarray(O.CLIP_MEAN, np.float32)) / np.asarray(O.CLIP_STD, np.float32)).reshape(3, 1, 1)
        assert (vals == black).mean() > 0.05 and (vals == white).mean() > 0.05, "both clamp values are frequent in the result"


def test_mixed_batch():
    """One image of each bucket and (224, 224) in one batch: the whole batch runs <0> (taps from memory), and every image's bits equal its
    single-image run (<8>, <16>, <0>, identity) and the oracle."""
    cs = [PC.case(340, 336), PC.case(340, 337), PC.case(790, 785), PC.case(224, 224)]
    got = run([PC.image(c) for c in cs])
    for i, c in enumerate(cs):
        assert np.array_equal(got[i], ref_bits(c.name)), (c.name, mismatch(got[i], ref_bits(c.name)))
        assert np.array_equal(got[i], check_case(c)), c.name


# ------------------------------------------------------------------------------------------------ small shapes, geometry edges
SMALL_CASES = [PC.case(h, w) for (h, w) in PC.SMALL_SHAPES]


@pytest.mark.parametrize("c", SMALL_CASES, ids=[c.name for c in SMALL_CASES])
def test_small_shapes_and_geometry_edges(c):
    check_case(c)


def test_early_return_in_a_shared_grid():
    """(2000, 300) needs 307 intermediate rows, (224, 224) needs 224: the grid is sized by the first, the second's blocks past row 224 return."""
    cs = [PC.case(*s) for s in PC.EARLY_RETURN_SHAPES]
    for order in (cs, cs[::-1]):
        got = run([PC.image(c) for c in order])
        for i, c in enumerate(order):
            assert np.array_equal(got[i], ref_bits(c.name)), (c.name, mismatch(got[i], ref_bits(c.name)))


# ------------------------------------------------------------------------------------------------ grey
GREY_CASES = [PC.case(h, w, channels=1, kind=k) for (h, w), _, _ in PC.GREY_SHAPES for k in ("noise", "blocks")]


@pytest.mark.parametrize("c", GREY_CASES, ids=[c.name for c in GREY_CASES])
def test_grey(c):
    """channels = 1: the grey branch of resample_h_kernel<0> (byte loads, one accumulator copied to three), which the engine never takes - it
    replicates grey images on the host.  Equal to the oracle on the 2-D array and to the channels = 3 run of the replicated image."""
    a = PC.image(c)
    got = check_case(c)
    rgb = run([np.repeat(a[:, :, None], 3, 2)])
    assert np.array_equal(got, rgb[0]), mismatch(got, rgb[0])
    plain = run([a], mean=(0, 0, 0), std=(1, 1, 1))[0]                    # the three channels hold one value
    assert np.array_equal(plain[0], plain[1]) and np.array_equal(plain[0], plain[2])


# ------------------------------------------------------------------------------------------------ other sizes
SIZE_CASES = [PC.case(h, w, size=s) for s, (h, w) in PC.OTHER_SIZES]


@pytest.mark.parametrize("c", SIZE_CASES, ids=[c.name for c in SIZE_CASES])
def test_other_sizes(c):
    """size 32: 32 of a block's 256 threads have a column; 288: both passes' `col += 256` loops take a second trip of 32 columns; 1024: four."""
    check_case(c)


# ------------------------------------------------------------------------------------------------ patch operand
@functools.lru_cache(maxsize=None)
def patch_batch(size, channels):
    cs = [PC.case(h, w, channels=channels, size=size) for (h, w) in PC.PATCH_SHAPES]
    return cs, np.stack([ref_bits(c.name).view(np.float32) for c in cs])


def patchify_call(px_bits, N, img, patch, dt):
    """ofx_patchify on fp32 pixels (uint32 bits, [N, 3, img, img]) twice -> uint16 rows"""
    px = torch.from_numpy(np.ascontiguousarray(px_bits).view(np.int32)).cuda()
    n_out = N * 3 * img * img
    outs = []
    for _ in range(2):
        out = torch.full((n_out + GUARD,), NANOP[dt], dtype=torch.int16, device="cuda")
        out[n_out:] = GUARD16
        L.check(L.load().ofx_patchify(px.data_ptr(), out.data_ptr(), N, img, patch, DT[dt], stream()), "ofx_patchify")
        torch.cuda.synchronize()
        assert bool((out[n_out:] == GUARD16).all()), "the output's guard"
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), "two calls, two results"
    return outs[0][:n_out]


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("size,patch", PC.PATCH_GRIDS)
def test_patch_operand(size, patch, channels):
    """resample_v_kernel<bf16_t> and <f16_t>: row (py g + px), column c p^2 + ky p + kx and the cast, against patch_operand(oracle pixels) and,
    where ofx_patchify takes the shape (patch % 8 == 0), against ofx_patchify(ofx_clip_preprocess(...)) - the pixel route's bits."""
    cs, px = patch_batch(size, channels)
    for dt in ("bf16", "f16"):
        for sel in ([1], [0, 1, 2, 3, 4]):
            ims = [PC.image(cs[i]) for i in sel]
            got = run(ims, size=size, patch=patch, dt=dt)
            want = R.patch_operand(px[sel], patch, dt)
            assert got.shape == want.shape and np.array_equal(got, want), (dt, len(sel), mismatch(got, want))
            if patch % 8 == 0:
                pixels = run(ims, size=size)
                assert np.array_equal(pixels, px[sel].view(np.uint32))
                via = as_u16(patchify_call(pixels, len(sel), size, patch, dt)).reshape(want.shape)
                assert np.array_equal(got, via), (dt, len(sel), "fused != ofx_patchify(ofx_clip_preprocess)", mismatch(got, via))
            else:
                px0 = torch.zeros(3 * size * size, device="cuda")
                out = torch.zeros(3 * size * size, dtype=torch.int16, device="cuda")
                assert L.load().ofx_patchify(px0.data_ptr(), out.data_ptr(), 1, size, patch, DT[dt], stream()) == OFX_ESHAPE


def lattice_pixels(N, img, seed):
    """fp32 bits around every rounding decision of both casts: exact ties of either parity, their neighbours, f16-subnormal results, zeros"""
    g = np.random.default_rng(seed)
    n = N * 3 * img * img
    e = g.integers(100, 130, n).astype(np.uint32)
    sign = g.integers(0, 2, n).astype(np.uint32) << 31
    drop = np.where(g.integers(0, 2, n) == 0, 16, 13).astype(np.uint32)
    kept = (g.integers(0, 1 << 10, n).astype(np.uint32) >> (drop - np.uint32(13))) << drop
    half = np.uint32(1) << (drop - np.uint32(1))
    low = np.choose(g.integers(0, 4, n), [half, half - np.uint32(1), half + np.uint32(1), g.integers(0, 1 << 13, n).astype(np.uint32)])
    u = sign | (e << 23) | kept | low
    u[g.integers(0, n, n // 50)] = 0
    return u.reshape(N, 3, img, img)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("N,img,patch", [(1, 224, 32), (3, 224, 32), (1, 64, 16), (3, 64, 16), (1, 32, 8), (3, 32, 8)])
def test_patchify(N, img, patch, dt):
    """patchify_kernel alone: the layout, and the cast on ties, their neighbours and f16-subnormal results."""
    u = lattice_pixels(N, img, N + img)
    got = as_u16(patchify_call(u, N, img, patch, dt)).reshape(-1, 3 * patch * patch)
    want = R.patch_operand(u.view(np.float32), patch, dt)
    assert np.array_equal(got, want), mismatch(got, want)


def test_patchify_past_the_grid_cap():
    """ofx_launch_patchify caps its grid at 32768 blocks of 256 threads, one 8-pixel group each: 446 images of 224 x 224 are 8,391,936 groups,
    3,328 past the cap - the grid-stride loop's second trip.  Compared on the device."""
    N, img, patch = 446, 224, 32
    assert N * 3 * img * img // 8 > 32768 * 256 >= (N - 1) * 3 * img * img // 8
    px = np.random.default_rng(8).random((N, 3, img, img), dtype=np.float32) * np.float32(4) - np.float32(2)
    got = patchify_call(px.view(np.uint32), N, img, patch, "bf16")
    want = torch.from_numpy(R.patch_operand(px, patch, "bf16").view(np.int16).reshape(-1)).cuda()
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} differ"


# ------------------------------------------------------------------------------------------------ normalisation
def test_normalisation():
    """mean 0 / std 1 leaves float(u8) * f32(1 / 255): the integer resize alone, against PIL's own uint8 result; then three non-CLIP (mean, std)
    pairs of three distinct values each: a swapped channel or a multiply-subtract fused into one rounding changes bits."""
    r255 = np.float32(1 / 255.0)
    for c in (PC.case(340, 337), PC.case(790, 785, kind="blocks"), PC.case(37, 53)):
        a = PC.image(c)
        got = run([a], mean=(0, 0, 0), std=(1, 1, 1))[0]
        u8 = PC.pil_u8(a, 224)
        assert np.array_equal(got, (u8.transpose(2, 0, 1).astype(np.float32) * r255).view(np.uint32)), c.name
        for mean, std in (((0.1, 0.5, 0.9), (0.2, 0.3, 0.7)), ((0.7231, 0.013, 0.31), (1.9, 0.511, 0.083)), ((-0.3, 0.25, 1.0), (3.0, 0.9, 0.123))):
            got = run([a], mean=mean, std=std)[0]
            want = ref_bits(c.name, mean, std)
            assert np.array_equal(got, want), (c.name, mean, std, mismatch(got, want))
            assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])


# ------------------------------------------------------------------------------------------------ input contract
def test_input_contract_unaligned_offsets():
    """Images back to back at odd byte offsets (the first at 1): nothing needs alignment.  Two descriptors may name the same bytes."""
    cs = [PC.case(37, 53), PC.case(1, 7), PC.case(7, 1), PC.case(2, 3), PC.case(340, 337)]
    ims = [PC.image(c) for c in cs]
    offs, off = [], 1
    for a in ims:
        offs.append(off)
        off += a.size
        off += (off + 1) % 2                                  # the next odd offset: at most one byte between two images
    assert all(o % 2 == 1 for o in offs) and len({o % 16 for o in offs}) >= 4
    got = run(ims, offsets=offs)
    for i, c in enumerate(cs):
        assert np.array_equal(got[i], ref_bits(c.name)), (c.name, mismatch(got[i], ref_bits(c.name)))
    c = PC.case(340, 337)
    got = run([PC.image(c), PC.image(c)], offsets=[3, 3])
    assert np.array_equal(got[0], ref_bits(c.name)) and np.array_equal(got[1], ref_bits(c.name))


@pytest.mark.parametrize("h,w", [(340, 336), (340, 337), (790, 785)])
def test_input_contract_the_fourth_byte(h, w):
    """Each RGB tap is one dword load whose fourth byte belongs to the next pixel - or, at an image's end, to whatever follows.  An all-black
    image followed by one 0xFF byte and an all-white image, and the reverse with 0x00: exactly the black and the white value, in <8>, <16>, <0>."""
    black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    want = {0: R.pixels([black])[0].view(np.uint32), 255: R.pixels([white])[0].view(np.uint32)}
    const = lambda v: np.broadcast_to(((np.float32(v) * np.float32(1 / 255.0) - np.asarray(O.CLIP_MEAN, np.float32)) / np.asarray(O.CLIP_STD, np.float32))
                                      .reshape(3, 1, 1), (3, 224, 224)).view(np.uint32)
    assert np.array_equal(want[0], const(0)) and np.array_equal(want[255], const(255)), "PIL keeps a constant image constant"
    n = h * w * 3
    for first, second, between in ((black, white, 0xFF), (white, black, 0x00)):
        got = run([first, second], offsets=[0, n + 1], fill=between)
        assert np.array_equal(got[0], want[int(first[0, 0, 0])]), mismatch(got[0], want[int(first[0, 0, 0])])
        assert np.array_equal(got[1], want[int(second[0, 0, 0])]), mismatch(got[1], want[int(second[0, 0, 0])])


# ------------------------------------------------------------------------------------------------ host state
def test_host_state_ring_and_plan_cache():
    """The pinned staging ring has 4 slots per device: six calls in flight without a synchronisation reuse slots 0 and 1 (waiting on their events),
    and the fifth and sixth plans - 64 and 80 images of pairwise distinct geometry, 0.8 and 1 MB of coefficient tables - make those slots grow.
    Then more than 4096 cached axis plans: the next batch evicts the cache and plans afresh.  Every result exact."""
    tiny = [PC.noise(3 + i, 5 + 2 * i, 3, 1000 + i) for i in range(80)]
    batches = [[PC.image(PC.case(224, 224))], [PC.image(PC.case(340, 336)), PC.image(PC.case(37, 53))], tiny[:3], tiny[3:7], tiny[:64], tiny]
    calls = [Call(b).launch() for b in batches]
    want = R.pixels(tiny).view(np.uint32)
    named = {0: [PC.case(224, 224)], 1: [PC.case(340, 336), PC.case(37, 53)]}
    for k, (call, sel) in enumerate(zip(calls, (None, None, slice(0, 3), slice(3, 7), slice(0, 64), slice(0, 80)))):
        got = call.check()
        ref = np.stack([ref_bits(c.name) for c in named[k]]) if sel is None else want[sel]
        assert np.array_equal(got, ref), (k, mismatch(got, ref))
    n = 2100
    hs, ws_ = np.arange(1, n + 1, dtype=np.int32), np.arange(3001, 3001 + n, dtype=np.int32)
    assert int(L.load().ofx_clip_preprocess_ws(hs.ctypes.data_as(I), ws_.ctypes.data_as(I), n, 3, 224)) > 0          # 4200 distinct axis plans
    for c in (PC.case(340, 336), PC.case(340, 337), PC.case(790, 785, kind="blocks")):
        check_case(c)


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_calls():
    """Every refusal returns its documented code, names what it refuses in ofx_last_error, and launches nothing: the poisoned outputs keep
    their bits."""
    lib = L.load()
    a = PC.image(PC.case(37, 53))
    pix, pat = Call([a]), Call([a], patch=32, dt="f16")
    before = [t.clone() for t in (pix.out, pat.out, pix.ws, pat.ws)]
    hs1, ws1, offs = (C.c_int * 1)(37), (C.c_int * 1)(53), (C.c_longlong * 1)(0)

    def patches(src=pat.src.data_ptr(), offsets=offs, heights=hs1, widths=ws1, N=1, channels=3, size=224, patch=32, mean=pat.mean, stdv=pat.std,
                out=pat.out.data_ptr(), dt=2, ws=pat.ws.data_ptr(), ws_bytes=pat.ws_bytes):
        return lib.ofx_clip_preprocess_patches(src, offsets, heights, widths, N, channels, size, patch, mean, stdv, out, dt, ws, ws_bytes, stream())

    def pixels(src=pix.src.data_ptr(), offsets=offs, heights=hs1, widths=ws1, N=1, channels=3, size=224, mean=pix.mean, stdv=pix.std,
               out=pix.out.data_ptr(), ws=pix.ws.data_ptr(), ws_bytes=pix.ws_bytes):
        return lib.ofx_clip_preprocess(src, offsets, heights, widths, N, channels, size, mean, stdv, out, ws, ws_bytes, stream())

    def refused(fn, code, word, **kw):
        rc = fn(**kw)
        err = lib.ofx_last_error()
        assert rc == code and word in err, (fn.__name__, kw, rc, err)

    for fn, name in ((patches, b"clip_preprocess_patches"), (pixels, b"clip_preprocess")):
        for p in ("src", "offsets", "heights", "widths", "mean", "stdv", "out", "ws"):
            refused(fn, OFX_EINVAL, name if fn is patches or p != "out" else b"exactly one output", **{p: None})
    for fn in (patches, pixels):
        refused(fn, OFX_EINVAL, b"clip_preprocess", N=0)
        for ch in (0, 2, 4):
            refused(fn, OFX_ESHAPE, b"channels=%d" % ch, channels=ch)
        for (h, w) in ((0, 53), (37, 0), (16385, 53), (37, 16385)):
            refused(fn, OFX_ESHAPE, b"image 0 is %d x %d" % (h, w), heights=(C.c_int * 1)(h), widths=(C.c_int * 1)(w))
        refused(fn, OFX_EWORKSPACE, b"workspace", ws_bytes=pix.ws_bytes // 2)
    refused(pixels, OFX_ESHAPE, b"size=0", size=0)
    refused(pixels, OFX_ESHAPE, b"size=1025", size=1025)
    refused(patches, OFX_ESHAPE, b"size=0", size=0)
    refused(patches, OFX_ESHAPE, b"size=1025", size=1025, patch=25)
    refused(patches, OFX_ESHAPE, b"patch=48", patch=48)                      # 224 % 48 != 0
    refused(patches, OFX_ESHAPE, b"patch=0", patch=0)
    refused(patches, OFX_ESHAPE, b"patch=-7", patch=-7)
    for dt in (0, 3):
        refused(patches, OFX_EINVAL, b"op_dtype = %d" % dt, dt=dt)
    assert lib.ofx_clip_preprocess_ws(None, ws1, 1, 3, 224) == 0 and lib.ofx_clip_preprocess_ws(hs1, ws1, 0, 3, 224) == 0
    assert lib.ofx_clip_preprocess_ws((C.c_int * 1)(0), ws1, 1, 3, 224) == 0 and lib.ofx_clip_preprocess_ws(hs1, (C.c_int * 1)(16385), 1, 3, 224) == 0

    px = torch.zeros(3 * 64 * 64, device="cuda")

    def patchify(pixels_=px.data_ptr(), out=pat.out.data_ptr(), N=1, img=64, patch=16, dt=2):
        return lib.ofx_patchify(pixels_, out, N, img, patch, dt, stream())

    for kw in (dict(pixels_=None), dict(out=None), dict(dt=0), dict(dt=3), dict(pixels_=px.data_ptr() + 4), dict(out=pat.out.data_ptr() + 2)):
        refused(patchify, OFX_EINVAL, b"patchify", **kw)
    for kw in (dict(N=0), dict(img=0), dict(patch=0), dict(img=60, patch=12), dict(img=64, patch=24), dict(img=28, patch=7), dict(img=36, patch=12)):
        refused(patchify, OFX_ESHAPE, b"patchify", **kw)
    torch.cuda.synchronize()
    for t, b in zip((pix.out, pat.out, pix.ws, pat.ws), before):
        assert torch.equal(t, b), "a refused call wrote something"
