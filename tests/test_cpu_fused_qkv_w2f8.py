"""The scale-byte address of fused_qkv_attn_w2f8_kernel (csrc/fused_qkv_attn.hip), without a GPU.

ofx_pack_lo8 writes the E8M0 scale byte of weight row n at scale8[((n >> 7) * 16 + (n & 15)) * 8 + ((n >> 4) & 7)] (include/ofx.h; one
64-bit word per (128-row block, n & 15)), laid out for gemm_w2f8_kernel, whose wave owns a whole 128-row block and picks fragment j's
byte with an immediate.  The fused kernel's tile is ONE head: its 64 q, 64 k and 64 v rows are halves of three different blocks, and a
wave's six 16-row fragments (tile columns wc 96 + 16 j) span two of them.  `kernel_byte` below transcribes what the kernel does - load_consts'
word address, stash_consts' parity shift and two-register gather, the selector immediates of FQ8_MFMA8 - and must land on pack_lo8's byte
for every head of widths 256 and 768 (both parities), every wave column, fragment and lane row."""
import pytest


def pack_lo8_byte(n):
    """include/ofx.h, ofx_pack_lo8: where row n's scale byte lies."""
    return ((n >> 7) * 16 + (n & 15)) * 8 + ((n >> 4) & 7)


def kernel_byte(width, head, wc, j, fr):
    """-> the byte offset into scale8 that fragment j of a wave in tile column half wc reads for its lane row fr."""
    word = lambda which: ((which * (width >> 7) + (head >> 1)) * 16 + fr) * 8          # load_consts: sw[which]
    shift = (head & 1) * 4                                                               # stash_consts: sw >> ((head & 1) * 32), in bytes
    q = [word(0) + shift + b for b in range(4)]                                         # the four bytes of each shifted 32-bit word
    k = [word(1) + shift + b for b in range(4)]
    v = [word(2) + shift + b for b in range(4)]
    sa = q if wc == 0 else k[2:] + v[:2]                                                 # wc ? (k >> 16) | (v << 16) : q
    sb = k[:2] if wc == 0 else v[2:]                                                     # wc ? v >> 16 : k
    return sa[j] if j < 4 else sb[j - 4]                                                 # FQ8_MF(j, j & 3, j < 4 ? sc_a : sc_b)


@pytest.mark.parametrize("width", [256, 768])
def test_every_fragment_reads_the_scale_byte_pack_lo8_wrote(width):
    heads = width // 64
    seen = set()
    for head in range(heads):
        for wc in range(2):
            for j in range(6):
                for fr in range(16):
                    c = wc * 96 + j * 16 + fr                                            # tile column = which * 64 + r
                    n = (c >> 6) * width + head * 64 + (c & 63)                          # the weight row behind it
                    assert kernel_byte(width, head, wc, j, fr) == pack_lo8_byte(n), (width, head, wc, j, fr, n)
                    seen.add(n)
    assert seen == set(range(3 * width))                                                 # every q | k | v row of every head, once


def test_the_parity_shift_matters():
    """An odd head read with an even head's bytes lands on the neighbouring head's rows: the transcription is sensitive to the slip."""
    width, fr = 256, 3
    for wc in range(2):
        for j in range(6):
            c = wc * 96 + j * 16 + fr
            n_even = (c >> 6) * width + 0 * 64 + (c & 63)
            assert kernel_byte(width, 1, wc, j, fr) == pack_lo8_byte(n_even + 64) != pack_lo8_byte(n_even)
