"""fused_qkv_attn_w2f8_kernel (csrc/fused_qkv_attn.hip; ofx_fused_qkv_attention_w2f8) on a real MI355X, through the C ABI.

The kernel gives every accumulator the instruction sequence gemm_w2f8_kernel gives it - per 128-deep super-step four f16 MFMAs in k order,
then one block-scaled fp8 MFMA of the e4m3 lo fragment against the e5m2 image of the activations - the epilogue is epi_value's chain rounded
once to f16, and the tail is the wave core ofx_attention runs.  So on ANY operands:

  A  the output EQUALS ofx_gemm_w2f8_fold (ofx_gemm_w2f8 without fold inputs) -> ofx_attention on the same operands, bit for bit (a -0 / +0
     difference is not a finding).  No tolerance: one would hide exactly the slips this kernel can have (a wrong scale byte, a k-step out of
     order, a fragment's image taken from another k-step, a stale constant of the previous tile).  The reference GEMM is forced onto the
     256 x 256 kernel (ofx_tune(2, 6)); its q | k | v are first compared with a second launch under ofx_tune(18, 0) (the other epilogue route).
  B  in every call the two guard rows behind `out` and the columns width .. ldo - 1 keep their bits, every written element is finite.
  C  refusals return the stated code and leave `out` untouched.
  D  the 12-layer ViT-B/32 encoder in 'f16w2x' on 160 and 163 images (>= 256 qkv tiles: the plan runs gemm_w2f8_kernel): the embeddings under
     ofx_tune(22, 1) and (22, 0) are np.array_equal, and the profile shows kind 7 records in the first run only.

Shapes (A, B): widths 256 (4 heads, two super-steps) and 768 (12 heads); S in {33, 50, 64}; n_img in {1, G, G + 1, 6 G + 1}, G = 256 // S; with
and without the fold inputs; the 6 G + 1 case again on a grid of 5 blocks (ofx_tune(11, 5): each block walks several tiles); and width 256,
S = 50, 11 images on 3 blocks: 12 tiles, a first, middle and last tile per walk and the prefetch under the tail.
Data: (i) standard normal X, weights N(0, 0.02^2) split by ofx_convert mode 3 and packed by ofx_pack_lo8; (ii) the same with two X columns
x 300 and single entries of +-60,000 (the e5m2 image's range and its clamp); (iii) weight rows scaled by 2^(n mod 7) - per-row scales differ
inside a head and between the two heads of a 128-row block - plus weight rows exactly representable in f16 (lo = 0, scale 2^0).

MEASURED (MI355X): A bit for bit in all 180 calls of the sweep (18 tests x 10) and all 6 of the three-block walk; the reference GEMM's two
epilogue routes agreed in every call; B held in every call; C every refusal returned its code with `out` untouched; D np.array_equal on 160 and
163 images with 11 kind-7 records in one run and 11 kind-8 qkv records in the other.  The file: 23 tests, 4.3 s, the slowest 1.0 s (D).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fused_qkv_cases as F
import test_gpu_fused_qkv_exact as E

pytestmark = pytest.mark.gpu

SCALE = F.SCALE
F16 = 2
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


def n_imgs(S):
    G = 256 // S
    return (1, G, G + 1, 6 * G + 1)


@functools.lru_cache(maxsize=4)
def operands(width, S, data):
    """Operands for the largest image count of (width, S); smaller counts use the leading rows.  X and out rows are width + 8 elements long
    (X's pad columns NaN)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * width + 10 * S + {"normal": 0, "outliers": 1, "rowscale": 2}[data])
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    M, N, st = max(n_imgs(S)) * S, 3 * width, stream()
    x = rnd(M, width)
    w = rnd(N, width) * 0.02
    if data == "outliers":
        x[:, 3] *= 300
        x[:, width - 5] *= 300
        x[0, 7], x[M - 1, width - 1], x[S + 1, 1], x[M // 2, width // 2] = 60000.0, -60000.0, 60000.0, -60000.0
    if data == "rowscale":
        w *= (2.0 ** (torch.arange(N, device="cuda") % 7))[:, None]
        for r in (5, 64 + 17, width + 64 + 3, 2 * width + 40):           # a q row of head 0, one of head 1, a k row of head 1, a v row of head 0
            w[r] = w[r].half().float()
    X = torch.full((M, width + 8), float("nan"), dtype=torch.float16, device="cuda")
    X[:, :width] = x.half()
    W2 = torch.empty(N, 2 * width, dtype=torch.float16, device="cuda")
    W8 = torch.empty(N, width, dtype=torch.uint8, device="cuda")
    s8 = torch.empty(N, dtype=torch.uint8, device="cuda")
    lib = L.load()
    L.check(lib.ofx_convert(w.contiguous().data_ptr(), W2.data_ptr(), N, width, 3, F16, st))
    L.check(lib.ofx_pack_lo8(W2.data_ptr(), W8.data_ptr(), s8.data_ptr(), N, width, st))
    torch.cuda.synchronize()
    if data == "rowscale":
        assert not W2[5, width:].any() and int(s8[((5 >> 7) * 16 + (5 & 15)) * 8 + ((5 >> 4) & 7)]) == 127      # lo = 0: scale 2^0
        assert len(set(s8[:64].tolist())) > 1
    stat = torch.stack([0.1 * rnd(M), 0.5 + 1.5 * torch.rand(M, generator=g, device="cuda")], 1).contiguous()
    return dict(X=X, W2=W2, W8=W8, s8=s8, bias=0.1 * rnd(N), stat=stat, cs=0.3 * rnd(N))


def fused(t, width, S, n_img, fold, label):
    M, ld = n_img * S, width + 8
    out, before = E.poisoned(M, ld, torch.float16)
    L.check(L.load().ofx_fused_qkv_attention_w2f8(t["X"].data_ptr(), t["W2"].data_ptr(), t["W8"].data_ptr(), t["s8"].data_ptr(), t["bias"].data_ptr(),
                                                  t["stat"].data_ptr() if fold else None, t["cs"].data_ptr() if fold else None, out.data_ptr(), n_img, S, width,
                                                  width // 64, ld, ld, SCALE, stream()), label)
    E.settle(out, before, width, label)
    return out[:M, :width].clone()


def reference(t, width, S, n_img, fold, label):
    """ofx_gemm_w2f8(_fold) on the 256 x 256 kernel -> ofx_attention; the GEMM's q | k | v are the same bits on both of its epilogue routes."""
    lib = L.load()
    M, N, ld = n_img * S, 3 * width, width + 8

    def gemm():
        q2, qb = E.poisoned(M, N, torch.float16)
        a = (t["X"].data_ptr(), t["W2"].data_ptr(), t["W8"].data_ptr(), t["s8"].data_ptr(), q2.data_ptr(), t["bias"].data_ptr())
        if fold:
            rc = lib.ofx_gemm_w2f8_fold(*a, t["stat"].data_ptr(), t["cs"].data_ptr(), M, N, width, ld, N, 0, stream())
        else:
            rc = lib.ofx_gemm_w2f8(*a, None, M, N, width, ld, N, 0, 0, 1, stream())
        L.check(rc, label + " reference GEMM")
        E.settle(q2, qb, N, label + " reference GEMM")
        return q2

    lib.ofx_tune(2, 6)
    try:
        lib.ofx_tune(18, 0)
        try:
            q_lds = gemm()
        finally:
            lib.ofx_tune(18, 1)
        q2 = gemm()
    finally:
        lib.ofx_tune(2, 0)
    assert torch.equal(E.bits(q2), E.bits(q_lds)), (label, "the reference GEMM's two epilogue routes disagree")
    o2, ob = E.poisoned(M, ld, torch.float16)
    L.check(lib.ofx_attention(q2.data_ptr(), o2.data_ptr(), None, n_img, S, width // 64, N, ld, width, 2 * width, 0, 0, SCALE, F16, stream()), label + " ofx_attention")
    E.settle(o2, ob, width, label + " ofx_attention")
    return o2[:M, :width].clone()


def mismatch(got, want, S, label):
    gb, wb = E.bits(got).int() & 0xFFFF, E.bits(want).int() & 0xFFFF
    bad = (gb != wb) & ~(((gb & 0x7FFF) == 0) & ((wb & 0x7FFF) == 0))
    if not bad.any():
        return None
    idx = bad.nonzero()
    r, c = idx[0].tolist()
    imgs, heads = sorted(set((idx[:, 0] // S).tolist())), sorted(set((idx[:, 1] // 64).tolist()))
    return (f"{label}: {int(bad.sum())} of {bad.numel()} elements differ; first at (row, column) = ({r}, {c}): got {got[r, c].item()!r}, want {want[r, c].item()!r}; "
            f"images {imgs[:12]}, heads {heads}")


@pytest.mark.parametrize("data", ["normal", "outliers", "rowscale"])
@pytest.mark.parametrize("S", [33, 50, 64])
@pytest.mark.parametrize("width", [256, 768])
def test_output_equals_the_gemm_attention_pair_bit_for_bit(width, S, data):
    t, lib, errors, calls = operands(width, S, data), L.load(), [], 0
    for n_img in n_imgs(S):
        for fold in (1, 0):
            label = f"w{width}-S{S}-{data}-n{n_img}{'' if fold else '-nofold'}"
            want = reference(t, width, S, n_img, fold, label)
            grids = (-1, 5) if n_img == max(n_imgs(S)) else (-1,)
            for grid in grids:
                lib.ofx_tune(11, grid)
                try:
                    got = fused(t, width, S, n_img, fold, label)
                finally:
                    lib.ofx_tune(11, -1)
                calls += 1
                msg = mismatch(got, want, S, label + (f" on {grid} blocks" if grid > 0 else ""))
                if msg:
                    errors.append(msg)
    print(f"EXACT w2f8 w{width} S{S} {data}: {calls - len(errors)} of {calls} calls bit for bit")
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("data", ["normal", "outliers", "rowscale"])
def test_twelve_tiles_on_three_blocks(data):
    """width 256, S = 50, 11 images: 3 groups x 4 heads = 12 live tiles of 24; on 3 blocks every block walks tiles (a first, middle and last one), skips
    the dead ones of the ragged unit, and fetches the next tile's first k-step under its epilogue and attention."""
    width, S, n_img = 256, 50, 11
    t, lib = operands(width, S, data), L.load()
    for fold in (1, 0):
        label = f"walk-{data}{'' if fold else '-nofold'}"
        want = reference(t, width, S, n_img, fold, label)
        lib.ofx_tune(11, 3)
        try:
            got = fused(t, width, S, n_img, fold, label)
        finally:
            lib.ofx_tune(11, -1)
        msg = mismatch(got, want, S, label)
        assert msg is None, msg


def test_refusals_launch_nothing():
    lib = L.load()
    n, W, ld = 2, 256, 264
    X = torch.zeros(n * 65, ld, dtype=torch.float16, device="cuda")
    Wq = torch.zeros(3 * W, 2 * W, dtype=torch.float16, device="cuda")
    W8, s8 = torch.zeros(3 * W, W, dtype=torch.uint8, device="cuda"), torch.full((3 * W,), 127, dtype=torch.uint8, device="cuda")
    bias, stat = torch.zeros(3 * W, device="cuda"), torch.ones(n * 65, 2, device="cuda")
    out, before = E.poisoned(n * 65, ld, torch.float16)

    def call(S=50, width=W, ldx=ld, ldo=ld, x=X.data_ptr(), w8=W8.data_ptr(), sc=s8.data_ptr(), st=None, c=None, n_img=n):
        return lib.ofx_fused_qkv_attention_w2f8(x, Wq.data_ptr(), w8, sc, bias.data_ptr(), st, c, out.data_ptr(), n_img, S, width, width // 64, ldx, ldo, SCALE, stream())

    for S in F.REFUSED_S:
        assert call(S=S) == F.OFX_ESHAPE, S
    assert call(width=192) == F.OFX_ESHAPE and b"128" in lib.ofx_last_error()          # 3 heads: fine for the f16 forms, no whole fp8 super-step here
    assert call(width=64) == F.OFX_ESHAPE
    assert call(ldx=W + 4) == F.OFX_ESHAPE and call(ldo=W + 4) == F.OFX_ESHAPE and call(ldo=W - 8) == F.OFX_ESHAPE
    assert call(w8=None) == F.OFX_EINVAL and call(sc=None) == F.OFX_EINVAL
    assert call(st=stat.data_ptr()) == F.OFX_EINVAL
    assert call(x=None) == F.OFX_EINVAL and call(n_img=0) == F.OFX_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(E.bits(out), before), "a refused call wrote to out"
    assert call() == F.OFX_OK                                                          # the same arguments, nothing missing: accepted
    torch.cuda.synchronize()


def _records(fn):
    lib = L.load()
    lib.ofx_profile_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        recs = (L.ProfRecord * 4096)()
        n = lib.ofx_profile_records(recs, 4096)
        ms, fl, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_longlong * 4)()
        L.check(lib.ofx_profile_read(ms, fl, cnt))
    finally:
        lib.ofx_profile_enable(0)
    return out, [(r.kind, r.kmul, r.M, r.N, r.K) for r in recs[:n]]


def test_vit_b32_embeddings_do_not_depend_on_the_switch():
    from conftest import W_SEED
    from outfitx_amd import synth
    from outfitx_amd.encoders import CLIPImageEncoder
    lib = L.load()
    enc = CLIPImageEncoder(vision_config={"patch_size": 32})
    enc.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in synth.vision_weights(W_SEED, patch=32).items()}, strict=True)
    enc = enc.cuda().eval()
    enc.tower_precision = "f16w2x"
    px = torch.from_numpy(synth.pixel_values(81, 163)).view(163, 1, 3, 224, 224).cuda()

    def run(n):
        with torch.no_grad():
            return enc(px[:n]).view(n, -1).cpu().numpy()

    for n in (160, 163):
        out = {}
        for v in (1, 0):
            lib.ofx_tune(22, v)
            try:
                out[v] = _records(lambda: run(n))
            finally:
                lib.ofx_tune(22, 1)
        (on, rec_on), (off, rec_off) = out[1], out[0]
        assert np.isfinite(on).all() and np.array_equal(on, off), (n, np.abs(on - off).max())
        fused_on, fused_off = [r for r in rec_on if r[0] == 7], [r for r in rec_off if r[0] == 7]
        assert fused_on == [(7, 2, n * 50, 2304, 768)] * 11 and not fused_off, (n, fused_on, fused_off)
        qkv_off = [r for r in rec_off if r[0] == 8 and r[3] == 2304]
        assert len(qkv_off) == 11 and not [r for r in rec_on if r[0] == 8 and r[3] == 2304], n       # the pair's qkv GEMMs ran as gemm_w2f8_kernel, and only there
