"""The packed weight arenas' layout walks and the one record -> GemmArgs builder (outfitx_amd/csrc/ofx_weights.h), run without a device:
a stand-alone program, built as HIP source with the Makefile's compiler and flags, configures a handle from a descriptor through
ofx_configure, walks the three arenas on a counting arena (twice) and prints every region and every packed GEMM's launch arguments.
Everything is checked against formulas and a table written out here: region bytes 2 * kmul * N * K (weight rows), 4 * N (fp32 vectors),
N * K + N (an fp8 pair, present exactly where has_f8 says), their number and order, 256-byte alignment, no overlap, total = end of the
last region, and per weight form K / lda / a_wrap / k_mult and which of W8 / bias / col_sum are set."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

BF16X, F16X, BF16X3, F16W2 = 0, 1, 2, 3              # ofx_precision (include/ofx.h)
PATCH, QKV, OUT, FC1, FC2 = 1, 2, 4, 8, 16           # OFX_W2_*
PLAIN, SPLIT, X3 = "plain", "split", "x3"
KMUL = {PLAIN: 1, SPLIT: 2, X3: 3}
# the smallest dimensions ofx_create accepts that still reach both sides of has_f8 (K = 128 < 256 on fc2, K = 256 / 768 elsewhere)
D, HEADS = 512, 8
VW, VMLP, VP, VIMG, VL = 256, 128, 16, 32, 2
TW, TMLP, VOCAB, NPOS, TL = 256, 128, 8, 4, 2
PD = 128
KP, S = 3 * VP * VP, (VIMG // VP) ** 2 + 1

FIELDS = ("outfit_precision", "d_ffn", "n_layers", "tower_precision", "vit_w2_mask", "vit_w2_qkv_layers", "vit_x3", "txt_x3", "proj_x3", "txt_w2_mask")

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "ofx_weights.h"
static void show(const char* name, const GemmArgs& g) {
    printf("gemm %%s %%d %%d %%d %%d %%d %%d %%d\n", name, g.K, g.lda, g.a_wrap, g.k_mult, g.W8 != nullptr && g.w8_scale != nullptr, g.bias != nullptr, g.col_sum != nullptr);
}
static void gemm(const char* name, const PackedGemm& c, int K) { GemmArgs g{}; use_gemm(g, c, K); show(name, g); }
static void walk(const char* arena, ofx_handle& h, size_t (*layout)(ofx_handle&, Arena&)) {
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<Region> log;
        Arena A; A.log = &log;
        const size_t total = layout(h, A);
        for (const Region& r : log) printf("region %%s %%d %%s%%s%%s %%zu %%zu\n", arena, pass, r.tag, *r.part ? "." : "", r.part, r.off, r.bytes);
        printf("total %%s %%d %%zu\n", arena, pass, total);
    }
}
static void layers(const std::vector<ClipLayer>& Ls, int W, int MLP) {
    for (const ClipLayer& L : Ls) { gemm("qkv", L.qkv, W); gemm("o", L.o, W); gemm("fc1", L.fc1, W); gemm("fc2", L.fc2, MLP); }
}
int main() {
    int v[10];
    while (scanf("%%d %%d %%d %%d %%d %%d %%d %%d %%d %%d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9) == 10) {
        ofx_model_desc d;
        memset(&d, 0, sizeof(d));
        d.d_model = %(D)d; d.n_head = %(HEADS)d; d.max_items = 16; d.outfit_act = OFX_ACT_MISH; d.ln_eps = 1e-5f;
        d.vit_width = %(VW)d; d.vit_heads = %(VW)d / 64; d.vit_mlp = %(VMLP)d; d.vit_patch = %(VP)d; d.vit_image = %(VIMG)d; d.vit_layers = %(VL)d;
        d.txt_width = %(TW)d; d.txt_heads = %(TW)d / 64; d.txt_mlp = %(TMLP)d; d.txt_vocab = %(VOCAB)d; d.txt_max_pos = %(NPOS)d; d.txt_layers = %(TL)d;
        d.proj_dim = %(PD)d;
        d.outfit_precision = v[0]; d.d_ffn = v[1]; d.n_layers = v[2]; d.tower_precision = v[3]; d.vit_w2_mask = v[4]; d.vit_w2_qkv_layers = v[5];
        d.vit_x3 = v[6]; d.txt_x3 = v[7]; d.proj_x3 = v[8]; d.txt_w2_mask = v[9];
        ofx_handle h;
        const char* why = ofx_configure(h, d);
        printf("case %%s\n", why ? why : "ok");
        if (why) continue;
        walk("outfit", h, layout_outfit); walk("vision", h, layout_vision); walk("text", h, layout_text);
        gemm("cir", h.cir, d.d_model);
        { GemmArgs g{}; use_cir_head(g, h); show("cir_head", g); }
        for (const OutfitLayer& L : h.ol) { gemm("in", L.in, d.d_model); gemm("out", L.out, d.d_model); gemm("l1", L.l1, d.d_model); gemm("l2", L.l2, h.ot_ffn_pad); }
        gemm("v_patch", h.v_patch, 3 * d.vit_patch * d.vit_patch); layers(h.vl, d.vit_width, d.vit_mlp); gemm("v_proj", h.v_proj, d.vit_width);
        layers(h.tl, d.txt_width, d.txt_mlp); gemm("t_proj", h.t_proj, d.txt_width);
    }
    return 0;
}
"""


def cases():
    base = dict(outfit_precision=BF16X3, d_ffn=200, n_layers=2, tower_precision=F16X, vit_w2_mask=0, vit_w2_qkv_layers=0, vit_x3=0, txt_x3=0, proj_x3=0,
                txt_w2_mask=0)
    out = [dict(base, outfit_precision=p, d_ffn=f, n_layers=n) for p in (BF16X, F16X, BF16X3, F16W2) for f in (128, 200) for n in (1, 2)]
    every = PATCH | QKV | OUT | FC1 | FC2
    for dt, vm, vx3, tx3, px3, tm in itertools.product((BF16X, F16X), (0, PATCH | OUT | FC2, every), (0, 1), (0, 1), (0, 1), (0, QKV | OUT | FC1 | FC2)):
        out.append(dict(base, tower_precision=dt, vit_w2_mask=vm, vit_x3=vx3, txt_x3=tx3, proj_x3=px3, txt_w2_mask=tm))
    out.append(dict(base, vit_w2_mask=every, vit_w2_qkv_layers=0b01))       # a per-layer rung: qkv split on layer 0 only
    return out


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    d = tmp_path_factory.mktemp("pack_layout")
    src = d / "layout.hip"
    src.write_text(PROGRAM % dict(D=D, HEADS=HEADS, VW=VW, VMLP=VMLP, VP=VP, VIMG=VIMG, VL=VL, TW=TW, TMLP=TMLP, VOCAB=VOCAB, NPOS=NPOS, TL=TL, PD=PD))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function".split()       # the Makefile's FLAGS
    subprocess.run([hipcc, *flags, "-Werror", "-I", os.path.join(ROOT, "outfitx_amd", "csrc"), str(src), "-o", str(d / "layout")], check=True)
    cs = cases()
    text = "".join(" ".join(str(c[k]) for k in FIELDS) + "\n" for c in cs)
    lines = subprocess.run([str(d / "layout")], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    blocks = []
    for ln in lines:
        if ln.startswith("case "):
            blocks.append({"status": ln[5:], "regions": {}, "totals": {}, "gemms": []})
            continue
        f = ln.split()
        if f[0] == "region":
            blocks[-1]["regions"].setdefault((f[1], int(f[2])), []).append((f[3], int(f[4]), int(f[5])))
        elif f[0] == "total":
            blocks[-1]["totals"][(f[1], int(f[2]))] = int(f[3])
        else:
            assert f[0] == "gemm", ln
            blocks[-1]["gemms"].append((f[1], tuple(int(x) for x in f[2:])))
    assert len(blocks) == len(cs)
    return list(zip(cs, blocks))


def has_f8(N, K, f16):
    return f16 and N % 128 == 0 and K % 128 == 0 and K >= 256


def gemm_regions(tag, N, K, form, bias=True, folded=False, f8=False):
    """(regions, f8 present) of one packed GEMM: rows, bias, column sums, fp8 pair."""
    r = [(tag + ".w", 2 * KMUL[form] * N * K)]
    if bias:
        r.append((tag + ".bias", 4 * N))
    if folded:
        r.append((tag + ".col_sum", 4 * N))
    pair = form == SPLIT and f8
    if pair:
        r += [(tag + ".w8", N * K), (tag + ".s8", N)]
    return r, pair


# form -> (K multiplier of GemmArgs::K, of lda, a_wrap = K?, k_mult)
ARGS = {PLAIN: (1, 1, False, 1), SPLIT: (2, 1, True, 1), X3: (3, 3, False, 3)}


def gemm_args(K, form, w8=False, bias=True, col_sum=False, k_mult=None):
    km, am, wrap, kmult = ARGS[form]
    return (km * K, am * K, K if wrap else 0, kmult if k_mult is None else k_mult, int(w8), int(bias), int(col_sum))


def expect_outfit(c):
    form = {BF16X: PLAIN, F16X: PLAIN, BF16X3: X3, F16W2: SPLIT}[c["outfit_precision"]]
    Fp = (c["d_ffn"] + 127) // 128 * 128
    wt = form == PLAIN
    reg = [("outfit_token", 4 * D), ("tgt_img_emb", 4 * (D // 2)), ("cp_w", 4 * D), ("cp_b", 4)]
    reg += gemm_regions("cir", D, D, form, bias=False)[0] + ([("cir.wt", 2 * D * D)] if wt else [])
    gem = [("cir", gemm_args(D, form, bias=False)), ("cir_head", gemm_args(D, form, bias=False, k_mult=1))]      # the head's k_mult = 1 override
    shapes = (("in", 3 * D, D), ("out", D, D), ("l1", Fp, D), ("l2", D, Fp))
    for _ in range(c["n_layers"]):
        for tag, N, K in shapes:
            reg += gemm_regions(tag, N, K, form)[0]                 # the outfit transformer never carries an fp8 pair
            gem.append((tag, gemm_args(K, form)))
        reg += [(t, 4 * D) for t in ("g1", "be1", "g2", "be2")]
        if wt:
            reg += [(tag + ".wt", 2 * N * K) for tag, N, K in shapes]
    return reg, gem


def expect_layers(n, W, MLP, masks, x3, f16):
    reg, gem = [], []
    for l in range(n):
        last = l + 1 == n
        form = lambda bit: X3 if x3 else (SPLIT if masks[l] & bit else PLAIN)
        # folded: qkv in every layer, fc1 except in the pooled last layer; three-product towers fold nothing
        for tag, N, K, bit, folded in (("qkv", 3 * W, W, QKV, not x3), ("o", W, W, OUT, False), ("fc1", MLP, W, FC1, not x3 and not last), ("fc2", W, MLP, FC2, False)):
            r, pair = gemm_regions(tag, N, K, form(bit), folded=folded, f8=has_f8(N, K, f16))
            reg += r
            gem.append((tag, gemm_args(K, form(bit), w8=pair, col_sum=folded)))
        reg += [(t, 4 * W) for t in ("g1", "be1", "g2", "be2")]
    return reg, gem


def expect_vision(c):
    f16 = c["tower_precision"] == F16X
    x3, px3 = bool(c["vit_x3"]), bool(c["proj_x3"] or c["vit_x3"])
    pform = SPLIT if c["vit_w2_mask"] & PATCH else PLAIN
    masks = [c["vit_w2_mask"] & ~(QKV if c["vit_w2_qkv_layers"] and not (c["vit_w2_qkv_layers"] >> l) & 1 else 0) for l in range(VL)]
    r, pair = gemm_regions("v_patch", VW, KP, pform, bias=False, f8=has_f8(VW, KP, f16))
    lr, lg = expect_layers(VL, VW, VMLP, masks, x3, f16)
    jform = X3 if px3 else PLAIN
    reg = [("v_cls", 4 * VW)] + r + [("v_pos", 4 * S * VW), ("v_pre_g", 4 * VW), ("v_pre_b", 4 * VW)] + lr + [("v_post_g", 4 * VW), ("v_post_b", 4 * VW)]
    reg += gemm_regions("v_proj", PD, VW, jform, bias=False)[0]
    gem = [("v_patch", gemm_args(KP, pform, w8=pair, bias=False))] + lg + [("v_proj", gemm_args(VW, jform, bias=False))]
    return reg, gem


def expect_text(c):
    f16 = c["tower_precision"] == F16X
    x3 = bool(c["txt_x3"])
    jform = X3 if x3 or c["proj_x3"] or c["vit_x3"] else PLAIN
    lr, lg = expect_layers(TL, TW, TMLP, [0 if x3 else c["txt_w2_mask"]] * TL, x3, f16)
    reg = [("t_tok", 4 * VOCAB * TW), ("t_pos", 4 * NPOS * TW)] + lr + [("t_fin_g", 4 * TW), ("t_fin_b", 4 * TW)] + gemm_regions("t_proj", PD, TW, jform, bias=False)[0]
    return reg, lg + [("t_proj", gemm_args(TW, jform, bias=False))]


def test_descriptors_are_accepted_where_ofx_create_accepts_them(walked):
    for c, b in walked:
        if c["txt_w2_mask"] and c["txt_x3"]:
            assert "txt_w2_mask" in b["status"]
        else:
            assert b["status"] == "ok", (c, b["status"])
    assert sum(b["status"] == "ok" for _, b in walked) >= 16 + 72 + 1


def test_regions_are_the_written_out_sizes_in_order_aligned_and_disjoint(walked):
    n_f8 = 0
    for c, b in walked:
        if b["status"] != "ok":
            continue
        for arena, expect in (("outfit", expect_outfit), ("vision", expect_vision), ("text", expect_text)):
            want = expect(c)[0]
            got = b["regions"][(arena, 0)]
            assert [(t, n) for t, _, n in got] == want, (c, arena)
            n_f8 += sum(t.endswith(".w8") for t, _ in want)
            end = 0
            for tag, off, n in got:
                assert off % 256 == 0 and end <= off < end + 256 and n > 0, (c, arena, tag)
                end = off + n
            assert b["totals"][(arena, 0)] == end
            assert b["regions"][(arena, 1)] == got and b["totals"][(arena, 1)] == end      # a second walk places everything where the first did
    assert n_f8 > 0


def test_use_gemm_builds_each_forms_arguments(walked):
    seen = set()
    for c, b in walked:
        if b["status"] != "ok":
            continue
        want = expect_outfit(c)[1] + expect_vision(c)[1] + expect_text(c)[1]
        assert b["gemms"] == want, c
        seen |= {(name, a[3], a[2] != 0, a[4], a[6]) for name, a in want}
    # the table reached: the head's override on a three-product weight, an unfolded fc1 (pooled last layer) next to a folded one, the
    # three-product towers' unfolded qkv, a split weight with and without its fp8 pair
    K3 = gemm_args(D, X3, bias=False, k_mult=1)
    assert K3 == (3 * D, 3 * D, 0, 1, 0, 0, 0)
    assert ("cir_head", 1, False, 0, 0) in seen and ("cir", 3, False, 0, 0) in seen
    assert ("fc1", 1, False, 0, 0) in seen and ("fc1", 1, False, 0, 1) in seen
    assert ("qkv", 3, False, 0, 0) in seen and ("qkv", 1, True, 1, 1) in seen and ("fc2", 1, True, 0, 0) in seen
