// The handle and its packed weights (api.hip): the one record of a packed GEMM, the descriptor -> configuration derivation and the
// layout walks of the three weight arenas.  Nothing here makes a HIP call except Arena::reserve / release, so a host program can
// configure a handle and walk its layouts without a device (tests/test_cpu_pack_layout.py).
#pragma once
#include <vector>

#include "ofx_common.h"

// plain [N, K]; split [N, hi(K) | lo(K)] against ONE copy of the activations (GemmArgs::a_wrap); three-product [N, hi | hi | lo]
// against [hi | lo | hi] activation rows of 3 K elements
enum WeightForm { W_PLAIN, W_SPLIT, W_X3 };
inline int w_kmul(WeightForm f) { return f == W_X3 ? 3 : (f == W_SPLIT ? 2 : 1); }           // K multiplier of the weight rows
inline int a_kmul(WeightForm f) { return f == W_X3 ? 3 : 1; }                                // K multiplier of the activation rows
inline int pack_rows_mode(WeightForm f) { return f == W_X3 ? 2 : (f == W_SPLIT ? 3 : 0); }   // ofx_launch_pack_rows mode

struct Region { const char* tag; const char* part; size_t off, bytes; };
struct Arena {                                      // library-owned HBM for packed weights
    char* base = nullptr; size_t cap = 0, off = 0;
    bool fresh = true;                              // newly allocated: zero padding has to be written (it survives re-packs)
    std::vector<Region>* log = nullptr;             // every take in order (layout tests)
    // A default-constructed arena counts, as Bump(nullptr, ~0) does: `off` after a layout walk is the size to reserve.
    int reserve(size_t bytes) {
        if (base && cap >= bytes) { off = 0; return OFX_OK; }
        if (base) (void)hipFree(base);
        base = nullptr; cap = 0; off = 0;
        OFX_HIP(hipMalloc((void**)&base, bytes));
        cap = bytes; fresh = true;
        return OFX_OK;
    }
    template <typename T> T* take(size_t n, const char* tag, const char* part = "") {
        off = align_up(off, 256);
        T* r = (T*)(base + off);
        if (log) log->push_back({tag, part, off, n * sizeof(T)});
        off += n * sizeof(T);
        return r;
    }
    void release() { if (base) (void)hipFree(base); base = nullptr; cap = off = 0; }
};

// fp8 companion of a split-weight copy (gemm_w2f8.hip): {e4m3 lo rows, per-row scale bytes}; filled at pack time for f16 towers and kept
// in the record of the [hi | lo] rows it belongs to (no process-wide table, nothing shared between handles or threads)
struct F8Pair { void* w8 = nullptr; void* s8 = nullptr; };
inline bool has_f8(size_t N, size_t K, int dt) { return dt == OFX_F16 && N % 128 == 0 && K % 128 == 0 && K >= 256; }   // the shapes gemm_w2f8 takes

// One packed GEMM as its launch reads it: the weight rows in ONE form, the bias (null: none), for a LayerNorm-folded weight
// (W . gamma rounded) the column sums of the rounded rows, its bias being bias + W beta (null: not folded), the fp8 copy of a split
// weight's lo halves (a null pair where the shape / type has none) and the W^T operand copy of the training dgrad (null: none).
struct PackedGemm { void* w = nullptr; WeightForm form = W_PLAIN; float* bias = nullptr; float* col_sum = nullptr; F8Pair f8; void* wt = nullptr; };
// The only place a record becomes launch arguments.  K = the logical depth; the A rows are [M, a_kmul K].
inline void use_gemm(GemmArgs& g, const PackedGemm& c, int K) {
    g.W = c.w; g.bias = c.bias; g.col_sum = c.col_sum;
    g.K = w_kmul(c.form) * K; g.lda = a_kmul(c.form) * K; g.k_mult = a_kmul(c.form);
    if (c.form == W_SPLIT) { g.a_wrap = K; g.W8 = c.f8.w8; g.w8_scale = c.f8.s8; }
}
struct OutfitLayer { PackedGemm in, out, l1, l2; float *g1, *be1, *g2, *be2; };      // in_proj, out_proj, linear1, linear2; norm1, norm2
struct ClipLayer { PackedGemm qkv, o, fc1, fc2; float *g1, *be1, *g2, *be2; };

struct ofx_handle {
    int device;
    ofx_model_desc d;
    // outfit transformer
    Arena a_out; bool out_ready = false;
    int ot_dtype, ot_ffn_pad; WeightForm ot_form;       // the form of every outfit-transformer weight: plain (bf16 / f16), split (f16w2), three-product (bf16x3)
    std::vector<OutfitLayer> ol;
    float *outfit_token, *tgt_img_emb, *cp_w, *cp_b; PackedGemm cir;
    // towers
    int tw_dtype;
    int vit_w2_mask = 0, txt_x3 = 0, proj_x3 = 0, vit_x3 = 0, txt_w2_mask = 0;    // operand scheme (ofx_model_desc); x3 towers hold ONLY the K-concatenated [hi | hi | lo] weight copies
    // training: events armed for the NEXT backward call (ofx_train_arm_layer_events), one per outfit-transformer layer
    std::vector<hipEvent_t> bwd_events;
    Arena a_vis; bool vis_ready = false;
    std::vector<ClipLayer> vl;
    PackedGemm v_patch, v_proj; float *v_cls, *v_pos, *v_pre_g, *v_pre_b, *v_post_g, *v_post_b;
    Arena a_txt; bool txt_ready = false;
    std::vector<ClipLayer> tl;
    float *t_tok, *t_pos, *t_fin_g, *t_fin_b; PackedGemm t_proj;
};

// The scoring path's CIR head (ofx_cir_head)
inline void use_cir_head(GemmArgs& g, const ofx_handle& h) {
    use_gemm(g, h.cir, h.d.d_model);
    g.k_mult = 1;       // the head has always launched, and been recorded, as a plain GEMM over K = 3 D in bf16x3: from 6,144 rows on k_mult = 3 would select gemm_x3's kernel
}

// Descriptor -> the handle's configuration (operand types, forms, masks, padded FFN width).  Returns why the descriptor is refused, or null.
inline const char* ofx_configure(ofx_handle& h, const ofx_model_desc& d) {
    // heads of 64 at the widths the project has always scored, heads of 96 at 1536 = 16 x 96, the reference's default (SigLIP) model.
    // (1536 as 24 heads of 64 is no model of the reference, and its single-product path - the MFMA attention at that width - is untested: refused.)
    const bool head64 = d.n_head >= 1 && d.d_model == d.n_head * 64 && (d.d_model == 512 || d.d_model == 768 || d.d_model == 1024);
    const bool head96 = d.n_head >= 1 && d.d_model == d.n_head * 96 && d.d_model == 1536;
    if (!head64 && !head96) return "d_model must be n_head*64 with d_model in 512/768/1024, or n_head*96 with d_model 1536";
    if (d.vit_width != d.vit_heads * 64 || d.txt_width != d.txt_heads * 64) return "tower head_dim must be 64";
    if (d.vit_width % 256 || d.txt_width % 256 || d.proj_dim % 128 || d.vit_mlp % 128 || d.txt_mlp % 128) return "tower dims must be multiples of 128/256";
    if (d.vit_image % d.vit_patch || (d.vit_image / d.vit_patch) * (d.vit_image / d.vit_patch) + 1 > 256) return "ViT sequence (patches+1) must be <= 256";
    if (d.max_items < 0 || d.max_items > 63) return "max_items must be in [0,63]";
    if (d.tower_precision != OFX_PREC_BF16 && d.tower_precision != OFX_PREC_F16) return "tower_precision must be BF16 or F16";
    if (d.outfit_precision < 0 || d.outfit_precision > 3) return "bad outfit_precision";
    if (d.n_layers < 1 || d.vit_layers < 1 || d.txt_layers < 1 || d.d_ffn < 1) return "layer counts / d_ffn must be positive";
    if (d.vit_w2_mask & ~(OFX_W2_PATCH | OFX_W2_QKV | OFX_W2_OUT | OFX_W2_FC1 | OFX_W2_FC2)) return "vit_w2_mask: unknown bit";
    if (d.txt_w2_mask & ~(OFX_W2_QKV | OFX_W2_OUT | OFX_W2_FC1 | OFX_W2_FC2)) return "txt_w2_mask: unknown bit";
    if (d.txt_w2_mask && d.txt_x3) return "txt_w2_mask applies to the single-product text tower (txt_x3 = 0)";
    h.d = d;
    h.ot_dtype = (d.outfit_precision == OFX_PREC_F16 || d.outfit_precision == OFX_PREC_F16W2) ? OFX_F16 : OFX_BF16;
    h.ot_form = d.outfit_precision == OFX_PREC_BF16X3 ? W_X3 : (d.outfit_precision == OFX_PREC_F16W2 ? W_SPLIT : W_PLAIN);
    h.ot_ffn_pad = pad128(d.d_ffn);
    h.tw_dtype = d.tower_precision == OFX_PREC_F16 ? OFX_F16 : OFX_BF16;
    h.vit_w2_mask = d.vit_w2_mask; h.txt_w2_mask = d.txt_w2_mask; h.txt_x3 = d.txt_x3 != 0; h.vit_x3 = d.vit_x3 != 0; h.proj_x3 = d.proj_x3 != 0 || h.vit_x3;
    return nullptr;
}

// ---- layout walks, one per arena, in the order the pack fills it: every pointer of the handle's records comes from here, and so does
// the arena's size (the same walk over a counting arena).  Each returns the bytes walked.
enum { G_BIAS = 1, G_FOLDED = 2, G_F8 = 4 };      // the parts of a record besides its rows; G_F8: where has_f8 and the form is split
inline void take_gemm(Arena& A, PackedGemm& c, const char* tag, size_t N, size_t K, WeightForm form, int parts, int dt) {
    c = PackedGemm{};
    c.form = form;
    c.w = A.take<char>(2 * w_kmul(form) * N * K, tag, "w");
    if (parts & G_BIAS) c.bias = A.take<float>(N, tag, "bias");
    if (parts & G_FOLDED) c.col_sum = A.take<float>(N, tag, "col_sum");
    if ((parts & G_F8) && form == W_SPLIT && has_f8(N, K, dt)) { c.f8.w8 = A.take<char>(N * K, tag, "w8"); c.f8.s8 = A.take<char>(N, tag, "s8"); }
}
inline size_t layout_outfit(ofx_handle& h, Arena& A) {
    const size_t D = h.d.d_model, Fp = h.ot_ffn_pad;
    const WeightForm f = h.ot_form;
    const bool wt = f == W_PLAIN;                   // single-product precisions also keep W^T operand copies for the backward
    const int dt = h.ot_dtype;
    h.outfit_token = A.take<float>(D, "outfit_token"); h.tgt_img_emb = A.take<float>(D / 2, "tgt_img_emb");
    h.cp_w = A.take<float>(D, "cp_w"); h.cp_b = A.take<float>(1, "cp_b");
    take_gemm(A, h.cir, "cir", D, D, f, 0, dt);
    if (wt) h.cir.wt = A.take<char>(2 * D * D, "cir", "wt");
    h.ol.resize(h.d.n_layers);
    for (OutfitLayer& L : h.ol) {
        take_gemm(A, L.in, "in", 3 * D, D, f, G_BIAS, dt);
        take_gemm(A, L.out, "out", D, D, f, G_BIAS, dt);
        take_gemm(A, L.l1, "l1", Fp, D, f, G_BIAS, dt);      // rows d_ffn.. are zero padding, as are l2's columns
        take_gemm(A, L.l2, "l2", D, Fp, f, G_BIAS, dt);
        L.g1 = A.take<float>(D, "g1"); L.be1 = A.take<float>(D, "be1"); L.g2 = A.take<float>(D, "g2"); L.be2 = A.take<float>(D, "be2");
        if (wt) {       // [K_w, N_w] operands of the backward dgrad GEMMs
            L.in.wt = A.take<char>(2 * D * 3 * D, "in", "wt"); L.out.wt = A.take<char>(2 * D * D, "out", "wt");
            L.l1.wt = A.take<char>(2 * D * Fp, "l1", "wt"); L.l2.wt = A.take<char>(2 * Fp * D, "l2", "wt");
        }
    }
    return A.off;
}
// Folded towers (x3 = false): qkv folds LayerNorm 1 in every layer; fc1 folds LayerNorm 2 except in the pooled last layer, which
// materialises it on the pooled rows.  Three-product towers materialise every LayerNorm.  Split copies where the layer's mask says so.
inline void layout_clip_layer(Arena& A, ClipLayer& L, size_t W, size_t MLP, int dt, int w2_mask, bool x3, bool last) {
    auto form = [&](int bit) { return x3 ? W_X3 : ((w2_mask & bit) ? W_SPLIT : W_PLAIN); };
    take_gemm(A, L.qkv, "qkv", 3 * W, W, form(OFX_W2_QKV), G_BIAS | G_F8 | (x3 ? 0 : G_FOLDED), dt);
    take_gemm(A, L.o, "o", W, W, form(OFX_W2_OUT), G_BIAS | G_F8, dt);
    take_gemm(A, L.fc1, "fc1", MLP, W, form(OFX_W2_FC1), G_BIAS | G_F8 | (x3 || last ? 0 : G_FOLDED), dt);
    take_gemm(A, L.fc2, "fc2", W, MLP, form(OFX_W2_FC2), G_BIAS | G_F8, dt);
    L.g1 = A.take<float>(W, "g1"); L.be1 = A.take<float>(W, "be1"); L.g2 = A.take<float>(W, "g2"); L.be2 = A.take<float>(W, "be2");
}
// per-layer rungs: a layer outside vit_w2_qkv_layers / vit_w2_fc1_layers / ... keeps the single-product copy of that GEMM
inline int vit_layer_mask(const ofx_handle& h, int l) {
    const ofx_model_desc& d = h.d;
    int m = h.vit_w2_mask;
    if (d.vit_w2_qkv_layers && !((d.vit_w2_qkv_layers >> l) & 1)) m &= ~OFX_W2_QKV;
    if (d.vit_w2_fc1_layers && !((d.vit_w2_fc1_layers >> l) & 1)) m &= ~OFX_W2_FC1;
    if (d.vit_w2_out_layers && !((d.vit_w2_out_layers >> l) & 1)) m &= ~OFX_W2_OUT;
    if (d.vit_w2_fc2_layers && !((d.vit_w2_fc2_layers >> l) & 1)) m &= ~OFX_W2_FC2;
    return m;
}
inline size_t layout_vision(ofx_handle& h, Arena& A) {
    const ofx_model_desc& d = h.d;
    const size_t W = d.vit_width, KP = 3 * (size_t)d.vit_patch * d.vit_patch, g = d.vit_image / d.vit_patch, S = g * g + 1;
    const int dt = h.tw_dtype;
    h.v_cls = A.take<float>(W, "v_cls");
    take_gemm(A, h.v_patch, "v_patch", W, KP, (h.vit_w2_mask & OFX_W2_PATCH) ? W_SPLIT : W_PLAIN, G_F8, dt);
    h.v_pos = A.take<float>(S * W, "v_pos"); h.v_pre_g = A.take<float>(W, "v_pre_g"); h.v_pre_b = A.take<float>(W, "v_pre_b");
    h.vl.resize(d.vit_layers);
    for (int l = 0; l < d.vit_layers; ++l) layout_clip_layer(A, h.vl[l], W, d.vit_mlp, dt, vit_layer_mask(h, l), h.vit_x3 != 0, l + 1 == d.vit_layers);
    h.v_post_g = A.take<float>(W, "v_post_g"); h.v_post_b = A.take<float>(W, "v_post_b");
    take_gemm(A, h.v_proj, "v_proj", d.proj_dim, W, h.proj_x3 ? W_X3 : W_PLAIN, 0, dt);
    return A.off;
}
inline size_t layout_text(ofx_handle& h, Arena& A) {
    const ofx_model_desc& d = h.d;
    const size_t W = d.txt_width;
    const bool x3 = h.txt_x3 != 0, x3p = x3 || h.proj_x3;          // x3p: the final LayerNorm + text_projection tail in three products
    h.t_tok = A.take<float>((size_t)d.txt_vocab * W, "t_tok"); h.t_pos = A.take<float>((size_t)d.txt_max_pos * W, "t_pos");
    h.tl.resize(d.txt_layers);
    for (int l = 0; l < d.txt_layers; ++l) layout_clip_layer(A, h.tl[l], W, d.txt_mlp, h.tw_dtype, x3 ? 0 : h.txt_w2_mask, x3, l + 1 == d.txt_layers);
    h.t_fin_g = A.take<float>(W, "t_fin_g"); h.t_fin_b = A.take<float>(W, "t_fin_b");
    take_gemm(A, h.t_proj, "t_proj", d.proj_dim, W, x3p ? W_X3 : W_PLAIN, 0, h.tw_dtype);
    return A.off;
}
