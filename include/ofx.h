/* libofx_hip.so — C ABI of the MI355X-native OutfitX compatibility-scoring forward path.
 *
 * The reference (Krual-T/OutfitX) is 100 % Python and has NO FFI / plugin interface; its boundary
 * for this path is the Python nn.Module API `src.models.OutfitX` (reference src/models/outfit_x.py).
 * This header is the boundary that sits directly UNDER that API: every entry point names the
 * reference symbol whose arithmetic it replaces.  The Python host (outfitx_amd/) binds it with
 * ctypes; see INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes only (no torch types); every pointer is a DEVICE pointer
 * unless marked host; every launch goes to the hipStream_t passed as `stream` (void*); no function
 * allocates caller-visible memory; return 0 on success or a negative OFX_E* code with text in
 * ofx_last_error() (thread-local).  gfx950 only.
 *
 * Host synchronisation and state - the complete list:
 *   - no entry point waits for the stream it launches on, with ONE bounded exception: ofx_clip_preprocess /
 *     ofx_vit_b32_fwd_u8 copy a few KB of host-computed resampling plan through a library-owned ring of 4 pinned
 *     slots per device and wait (hipEventSynchronize) only if the copy issued 4 calls earlier on that device has not
 *     left its slot yet;
 *   - ofx_profile_read waits for its events (it is a read-back; profiling is off by default);
 *   - library-owned state: the ofx_handle (packed weight arenas on the handle's device), the per-device pinned ring
 *     above, a host-side cache of resampling coefficient tables, the ofx_tune knobs and the profiling records.
 *     Nothing else is process-global; handles of different devices are independent.
 */
#ifndef OFX_H
#define OFX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFX_ABI_VERSION 6

enum { OFX_OK = 0, OFX_EINVAL = -1, OFX_ESHAPE = -2, OFX_EHIP = -3, OFX_EWORKSPACE = -4, OFX_ESTATE = -5 };
enum ofx_dtype { OFX_F32 = 0, OFX_BF16 = 1, OFX_F16 = 2 };
/* OFX_ACT_MISH_GRAD (backward): out = acc * mish'(resid) - `resid` then carries the saved pre-activation, not an addend */
enum ofx_act { OFX_ACT_NONE = 0, OFX_ACT_QUICK_GELU = 1, OFX_ACT_GELU = 2, OFX_ACT_MISH = 3, OFX_ACT_MISH_GRAD = 4 };
/* MFMA operand precision of a sub-model.  BF16X3 = three bf16 products per term
 * (hi*hi + lo*hi + hi*lo, realised as one K-concatenated GEMM) ~ fp32-grade results. */
/* OFX_PREC_F16W2 (outfit transformer only, round 4): f16 activations against split (hi, lo) f16 weights - two MFMA products per weight on ONE copy of
 * the activations (the towers' scheme): two thirds of bf16x3's weight bytes and matrix work, ~1e-4 instead of ~1e-5 from the fp32 reference; scoring only. */
enum ofx_precision { OFX_PREC_BF16 = 0, OFX_PREC_F16 = 1, OFX_PREC_BF16X3 = 2, OFX_PREC_F16W2 = 3 };
enum ofx_out_kind { OFX_OUT_F32 = 0, OFX_OUT_OP = 1, OFX_OUT_SPLIT3 = 2 };

typedef struct ofx_handle ofx_handle;
typedef void* ofx_stream; /* hipStream_t */

const char* ofx_last_error(void);
int ofx_abi_version(void);

/* ------------------------------------------------------------------ model description ------ */
typedef struct ofx_model_desc {
    /* global outfit Transformer — reference src/models/configs/transformer_config.py:8-24 */
    int d_model, n_head, d_ffn, n_layers, max_items; /* 1024, 16, 2024, 6, 16 */
    int outfit_act;                                   /* OFX_ACT_MISH */
    int outfit_precision;                             /* ofx_precision */
    /* CLIP vision tower (ViT-B/32 by default; any patch / image with (image/patch)^2 + 1 <= 256 tokens, e.g. B/16 at 224) — HF CLIPVisionConfig as loaded by clip_image_encoder.py:20-22 */
    int vit_width, vit_layers, vit_heads, vit_mlp, vit_patch, vit_image, vit_act; /* 768,12,12,3072,32,224 */
    /* CLIP text tower — HF CLIPTextConfig as loaded by clip_text_encoder.py:19-21 */
    int txt_width, txt_layers, txt_heads, txt_mlp, txt_vocab, txt_max_pos, txt_act, txt_eos_id; /* 512,12,8,2048,49408,77 */
    int proj_dim;                                     /* 512 */
    int tower_precision;                              /* OFX_PREC_BF16 | OFX_PREC_F16: operand type of both towers */
    float ln_eps;                                     /* 1e-5 */
    /* Operand scheme of the towers beyond one product per term (all zero = single product everywhere):
     * vit_w2_mask: OFX_W2_* bits - these ViT GEMMs multiply against split (hi, lo) weights, two MFMA products per weight;
     * txt_x3:      the text tower runs three products per term (hi*hi + lo*hi + hi*lo, K-concatenated);
     * proj_x3:     the ViT's post-LayerNorm + visual_projection tail runs three products per term;
     * vit_x3:      the whole ViT runs three products per term (fp32 residual stream, materialised LayerNorms; the MFMA attention core
     *              stays on once-rounded q, k, v, P): ~1.5e-4 end to end on any weight draw at 1.9x the time of the default scheme;
     *              vit_w2_mask then only matters for the patch embedding. */
    int vit_w2_mask, txt_x3, proj_x3, vit_x3;
    /* Finer rungs of the same ladder (round 4; all zero = the behaviour above):
     * txt_w2_mask: OFX_W2_QKV / OUT / FC1 / FC2 bits - with txt_x3 = 0 the TEXT tower runs the ViT's scheme: f16 activations against split
     *              (hi, lo) weights on those GEMMs (1.5-2 product equivalents instead of 3), MFMA attention on once-rounded q, k, v;
     *              its final LayerNorm + text_projection stay three-product when proj_x3 is set;
     * vit_w2_qkv_layers / vit_w2_fc1_layers / vit_w2_out_layers / vit_w2_fc2_layers: bit l set = ViT layer l's qkv / fc1 / out-proj / fc2 GEMM
     *              takes the split weights that the OFX_W2_* bit asks for; 0 = every layer.  (The other layers run the single-product copy:
     *              qkv through the fused QKV + attention kernel.) */
    int txt_w2_mask, vit_w2_qkv_layers, vit_w2_fc1_layers, vit_w2_out_layers, vit_w2_fc2_layers;
} ofx_model_desc;
enum { OFX_W2_PATCH = 1, OFX_W2_QKV = 2, OFX_W2_OUT = 4, OFX_W2_FC1 = 8, OFX_W2_FC2 = 16 };

/* Fills *d with the configuration of the reference's type='clip' model. */
void ofx_default_desc(ofx_model_desc* d);

/* The outfit transformer is scored with heads of 64 columns at d_model in {512, 768, 1024} and with heads of 96 at d_model 1536 (16 x 96,
 * the reference's default SigLIP model); any other (d_model, n_head) makes ofx_create return NULL with the rule in ofx_last_error().
 * The tower rules are unchanged (heads of 64).  Training (every ofx_*_train_fwd / _bwd entry point) exists for heads of 64 and d_model in
 * {512, 768, 1024}: on another handle those calls return OFX_ESHAPE at entry, before anything is launched. */
ofx_handle* ofx_create(int device, const ofx_model_desc* desc);
void ofx_destroy(ofx_handle* h);

/* ------------------------------------------------------------------ weight packing --------- *
 * fp32 torch parameters (device pointers, contiguous) -> MFMA operand layout in the handle's own
 * HBM arena.  Re-run after the parameters change (optimizer.step / load_state_dict).
 * Pointer order = state_dict order of the reference module:
 *   outfit: [outfit_token, target_item_image_emb, cp_ffn.1.weight, cp_ffn.1.bias, cir_ffn.0.weight]
 *           then per layer: in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias,
 *           linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.w, norm1.b, norm2.w, norm2.b
 *   vision: [class_embedding, patch_embedding.weight, position_embedding.weight, pre_layrnorm.w, .b]
 *           then per layer: k_proj.w,.b, v_proj.w,.b, q_proj.w,.b, out_proj.w,.b, layer_norm1.w,.b,
 *           mlp.fc1.w,.b, mlp.fc2.w,.b, layer_norm2.w,.b ; then post_layernorm.w,.b, visual_projection.weight
 *   text:   [token_embedding.weight, position_embedding.weight] then per layer (as vision) ;
 *           then final_layer_norm.w,.b, text_projection.weight                                  */
int ofx_pack_outfit_weights(ofx_handle* h, const void* const* fp32_params, int n_params, ofx_stream stream);
int ofx_pack_vision_weights(ofx_handle* h, const void* const* fp32_params, int n_params, ofx_stream stream);
int ofx_pack_text_weights(ofx_handle* h, const void* const* fp32_params, int n_params, ofx_stream stream);

/* ------------------------------------------------------------------ workspace -------------- */
enum ofx_op { OFX_OP_SET_ENCODER = 0, OFX_OP_VIT = 1, OFX_OP_TEXT = 2, OFX_OP_TOPK = 3 };
/* bytes of scratch the op needs for `n` units (outfits / images / texts / queries) of `len`
 * (max items incl. none / unused / tokens per text / pool rows). */
size_t ofx_workspace_bytes(ofx_handle* h, int op, int n, int len);

/* ------------------------------------------------------------------ hot path --------------- */
/* Rows B/C/D of SURVEY §8a: prefix-token concat + key-padding mask + the 6-layer pre-norm
 * Transformer encoder + "take row 0" — replaces src/models/outfit_x.py:129-142 (CP) and
 * :154-168 (CIR) incl. the nn.TransformerEncoder call.  Padded items are skipped (pad-free).
 *   x         [B, L, d_model] fp32 item embeddings (row-major)
 *   pad_mask  [B, L] uint8/bool, non-zero = padded item (reference: True = pad)
 *   prefix    [d_model] (prefix_stride 0: CP outfit_token) or [B, d_model] (stride d_model: CIR)
 *             fp32; NULL = use the packed outfit_token
 *   out_row0  [B, d_model] fp32: encoder output at the prefix position                         */
int ofx_set_encoder_fwd(ofx_handle* h, const float* x, const uint8_t* pad_mask, const float* prefix,
                        int prefix_stride, int B, int L, float* out_row0, void* ws, size_t ws_bytes,
                        ofx_stream stream);
/* cp_ffn = Dropout -> Linear(d_model,1): raw logit per outfit (outfit_x.py:57-61,143). */
int ofx_cp_head(ofx_handle* h, const float* row0, int B, float* logits, ofx_stream stream);
/* cir_ffn = Linear(d_model,d_model,bias=False) (outfit_x.py:65-67,171). */
int ofx_cir_head(ofx_handle* h, const float* row0, int B, float* emb, void* ws, size_t ws_bytes, ofx_stream stream);
/* CIR prefix token [target_item_image_emb ‖ target text emb] (outfit_x.py:154-158): out [B,d_model]. */
int ofx_cir_prefix(ofx_handle* h, const float* target_text_emb, int B, float* prefix_out, ofx_stream stream);

/* Row F: HF CLIPVisionModelWithProjection(pixel_values).image_embeds (clip_image_encoder.py:74-76)
 * + optional F.normalize (base_image_encoder.py:46-47).  pixels [N,3,vit_image,vit_image] fp32 (already
 * resized/normalised by the host processor; the descriptor's vit_patch / vit_image set the grid: B/32 at 224 is 50 tokens, B/16 at
 * 224 is 197, at most 256 tokens - the entry point keeps its name); emb [N, emb_ld] fp32, written at column emb_col.   */
int ofx_vit_b32_fwd(ofx_handle* h, const float* pixels, int N, float* emb, int emb_ld, int emb_col,
                    int normalize, void* ws, size_t ws_bytes, ofx_stream stream);
/* Row G: HF CLIPTextModelWithProjection(input_ids, attention_mask).text_embeds
 * (clip_text_encoder.py:56-58) + optional F.normalize.  ids/mask [N,T] int64.  `lengths` is a HOST
 * array [N] of tokens to compute per text (= EOS position + 1; causal attention makes later tokens
 * irrelevant), or NULL to compute all T.                                                        */
int ofx_clip_text_fwd(ofx_handle* h, const int64_t* ids, const int64_t* attn_mask, const int* lengths_host,
                      int N, int T, float* emb, int emb_ld, int emb_col, int normalize, void* ws,
                      size_t ws_bytes, ofx_stream stream);
/* The same with the texts' common first position computed once.  shared_first != 0 is the CALLER'S word that (a) ids[i, 0] is the same
 * token for every text (CLIP's BOS), (b) attn_mask is NULL or non-zero in column 0 of every text.  The tower is causal, so position 0 attends
 * to itself only and is then the same row for every text in every layer: the three-product scheme (txt_x3) computes it once, on
 * 1 + N (Tc - 1) rows instead of N Tc (Tc = computed tokens per text) - the same bits as ofx_clip_text_fwd wherever the full-row GEMMs do
 * not plan split-K (batches beyond a few texts; then the fp32 summation order depends on the row count as it does between two batch sizes).
 * The flag is ignored - the call IS ofx_clip_text_fwd - when shared_first == 0, Tc < 2, the text scheme is not the three-product one, or
 * ofx_tune(21, 0) is set.  Same workspace size (ofx_workspace_bytes(OFX_OP_TEXT)).  Added within ABI version 6: nothing existing changed. */
int ofx_clip_text_fwd_shared(ofx_handle* h, const int64_t* ids, const int64_t* attn_mask, const int* lengths_host,
                             int N, int T, float* emb, int emb_ld, int emb_col, int normalize, int shared_first, void* ws,
                             size_t ws_bytes, ofx_stream stream);

/* Row H: torch.cdist(y[B,1,D], cand[B,C,D]).squeeze(1).argmin(-1) (fill_in_the_blank_trainer.py:50-56).
 * idx int64 [B] = the first minimum; dist fp32 [B,C] optional.  D a multiple of 4 (else OFX_EINVAL); rows are read as 16-byte vectors.
 * Non-finite inputs follow torch: a NaN distance wins over every number and the first NaN is returned; +inf is an ordinary (largest) value. */
int ofx_fitb_argmin(const float* y_hat, const float* cand, int B, int C, int D, int64_t* idx, float* dist,
                    ofx_stream stream);
/* Row H with the candidates named by row of a device-resident embedding table (the index form of a FITB batch: no [B, C, D] tensor exists
 * anywhere):  exactly ofx_fitb_argmin with cand[b, c] = table[cand_index[b, c]] - the same kernel body reading its candidate rows through the
 * indices, the same summation order, hence the same bits in idx and dist as the dense call on the gathered rows, the tie and NaN rules included.
 *   table [n_table, ld] fp32, ld >= D, ld % 4 == 0, 16-byte aligned (a row's first D floats are used); cand_index int32 [B, C], contiguous;
 *   y_hat [B, D] fp32, 16-byte aligned; idx int64 [B]; dist fp32 [B, C] optional.
 *   answer int64 [B] with n_correct DEVICE int [1], both or neither: *n_correct += the number of b with idx[b] == answer[b] (the reference's
 *   `correct` of fill_in_the_blank_trainer.py:56).  It accumulates - the caller zeroes it - so a whole test epoch adds into one counter and
 *   reads it once, without a host synchronisation per batch.  Integer atomics only: the count does not depend on the order of arrival.
 *   cand_index lives on the device, so the host cannot check its values: the kernel clamps every entry into [0, n_table).  A wrong index
 *   gives a wrong answer, never an access outside the table.
 * NULL table / cand_index / y_hat / idx, only one of answer / n_correct, table or y_hat not 16-byte aligned: OFX_EINVAL; B < 1, C < 1,
 * D % 4 != 0 or D < 4, ld < D, ld % 4 != 0, n_table outside [1, INT_MAX]: OFX_ESHAPE - a rejected call launches nothing.  One launch on
 * `stream`, no workspace, no handle, no allocation, copy or wait (capturable). */
int ofx_fitb_argmin_indexed(const float* table, int ld, long long n_table, const int* cand_index, const float* y_hat, int B, int C, int D,
                            const int64_t* answer, int64_t* idx, float* dist, int* n_correct, ofx_stream stream);
/* Row I: torch.cdist(Q,P) -> topk(k, largest=False) (complementary_item_retrieval_trainer.py:240-249).
 * fp32-exact distances; ascending; ties -> smaller pool index.  idx int64 [nq,k] = row + index_base.
 * Preconditions, checked: D a multiple of 32 and 1 <= k <= min(128, np) (else OFX_ESHAPE), Q and P 16-byte aligned and no NULL argument
 * (OFX_EINVAL), ws_bytes >= ofx_workspace_bytes(OFX_OP_TOPK, nq, np) (OFX_EWORKSPACE); a rejected call launches nothing.
 * Non-finite inputs: a pool row that holds a NaN or an infinity has a non-finite distance (NaN or +inf) to every query and sorts behind every
 * finite distance, as in torch.topk(largest=False): it is returned only when fewer than k rows are finite; the finite rows are selected and
 * ordered as if it were absent.  A query that holds one gets k distinct in-range rows with non-finite distances, nothing more. */
int ofx_l2_topk(ofx_handle* h, const float* Q, const float* P, int nq, int np, int D, int k, int64_t index_base,
                int64_t* idx, float* dist, void* ws, size_t ws_bytes, ofx_stream stream);
/* Row I per category pool (the validation / test loops, complementary_item_retrieval_trainer.py:192-249, and demo/app.py:184-190): every query
 * searches the pool of its own group only; all groups in one launch sequence (two row-norm launches, one distance launch, one select launch),
 * no host synchronisation.  Q [nq,D]: the queries, each group's contiguous; P [np,D]: all pools concatenated.
 * panels: DEVICE int [n_panels][4] = (q_lo, q_hi, p_lo, p_hi), 16-byte aligned: query rows [q_lo, q_hi), at most 128, search pool rows [p_lo, p_hi)
 * and nothing else.  Precondition, not checked: panels ascend in q_lo, are disjoint and cover [0, nq); max_group_rows >= every p_hi - p_lo.  The
 * kernels clamp what the table holds into [0, nq), [0, np) and max_group_rows, so a wrong table gives wrong results, never an access out of bounds.
 * idx int64 [nq,k] = rows of P, dist fp32 [nq,k]: per query the bits of the flat call on its own pool with index_base = p_lo (ascending, ties ->
 * smaller row, non-finite rows last within the pool).  A pool of fewer than k rows: its rows in order, then idx -1 / dist +inf.
 * gt int64 [nq] (a row of P, < 0 = none) with gt_pos int [nq], both or neither: gt_pos[q] = the j with idx[q,j] == gt[q], else k (also for gt < 0),
 * written by the select from the keys it holds; recall@K = count(gt_pos < K) / count(gt >= 0) for every K <= k.
 * Checked: no NULL among Q, P, panels, idx, dist, ws and the alignment of Q, P, panels (OFX_EINVAL); D a multiple of 32, 1 <= k <= 128,
 * n_panels >= 1, max_group_rows >= 1 (OFX_ESHAPE); ws_bytes >= the _ws figure below for nq, np, max_group_rows (OFX_EWORKSPACE, it holds the
 * norms of all np pool rows, hence np); a rejected call launches nothing. */
size_t ofx_l2_topk_grouped_ws(int nq, int np, int max_group_rows);
int ofx_l2_topk_grouped(ofx_handle* h, const float* Q, const float* P, int nq, int np, int D, int k, const int* panels, int n_panels,
                        int max_group_rows, const int64_t* gt, int64_t* idx, float* dist, int* gt_pos, void* ws, size_t ws_bytes,
                        ofx_stream stream);
/* Merge `parts` candidate lists (after the RCCL all-gather of per-shard top-k): in [parts,nq,k], each list ascending, rows unique across lists.
 * parts * k <= 1024 (else OFX_ESHAPE).  Ordered by (distance bits, global index): NaN distances sort last here as well. */
int ofx_topk_merge(const int64_t* idx_in, const float* dist_in, int parts, int nq, int k, int64_t* idx, float* dist,
                   ofx_stream stream);

/* ------------------------------------------------------------------ image preprocessing ("next" row N2) --- */
/* CLIPImageProcessor(do_convert_rgb=False) as the reference runs it on the host (clip_image_encoder.py:29-31,69-71): resize the
 * shortest edge to `size` with PIL's antialiased BICUBIC (ImagingResample: 22-bit fixed-point coefficients, horizontal then
 * vertical, 8-bit intermediate — bit-exact), centre crop size x size, x 1/255, (x - mean) / std -> out [N, 3, size, size] fp32
 * (device), equal to the host pipeline bit for bit.  src: device buffer holding the N uint8 images row-major with `channels`
 * (3 = RGB interleaved, 1 = grey, replicated) at byte offsets[i]; offsets / heights / widths are HOST arrays.  RGB pixels are
 * fetched as unaligned dwords: src must stay readable 1 byte past the end of every image (give the buffer >= 4 bytes of slack);
 * that byte never reaches a result, and offsets need no alignment.  mean / stdv: HOST arrays of 3 floats. */
size_t ofx_clip_preprocess_ws(const int* heights, const int* widths, int N, int channels, int size);
int ofx_clip_preprocess(const uint8_t* src, const long long* offsets, const int* heights, const int* widths, int N, int channels, int size,
                        const float* mean, const float* stdv, float* out, void* ws, size_t ws_bytes, ofx_stream stream);
/* Op-level forms of the two kernels that build the patch-embedding GEMM's operand (tests and tools; the model path does not go through them).
 *   ofx_clip_preprocess_patches: the same resize / crop / normalise, the vertical pass writing `patches` [N (size / patch)^2, 3 patch^2] operand
 *     type (device) instead of fp32 pixels: row n g^2 + py g + px (g = size / patch), column c patch^2 + ky patch + kx = cast(the fp32 value
 *     ofx_clip_preprocess gives pixel (n, c, py patch + ky, px patch + kx)) - the im2col of Conv2d(3, width, patch, stride patch) in its
 *     weight.reshape(width, -1) column order.  mean / stdv: HOST arrays of 3 floats (as for ofx_clip_preprocess); workspace: ofx_clip_preprocess_ws.
 *     A NULL pointer or op_dtype other than OFX_BF16 / OFX_F16 is OFX_EINVAL; patch <= 0, size % patch != 0 and what ofx_clip_preprocess refuses
 *     are OFX_ESHAPE; a short workspace OFX_EWORKSPACE.  A refused call launches nothing.
 *   ofx_patchify: the pixel route's counterpart: pixels fp32 [N, 3, img, img] (device, 16-byte aligned) -> out [N (img / patch)^2, 3 patch^2]
 *     operand type (16-byte aligned), same layout, out = cast(pixel).  img % patch == 0, img % 8 == 0, patch % 8 == 0, N >= 1 (OFX_ESHAPE). */
int ofx_clip_preprocess_patches(const uint8_t* src, const long long* offsets, const int* heights, const int* widths, int N, int channels, int size,
                                int patch, const float* mean, const float* stdv, void* patches, int op_dtype, void* ws, size_t ws_bytes,
                                ofx_stream stream);
int ofx_patchify(const float* pixels, void* out, int N, int img, int patch, int op_dtype, ofx_stream stream);
/* The two fused: decoded uint8 images -> image embeddings (clip_image_encoder.py:66-76 in one call).  The preprocessor's
 * vertical pass writes the operand-type im2col rows of the patch-embedding GEMM directly, so neither the fp32 pixel_values
 * tensor (0.6 MB / image) nor the patchify pass exists; results equal ofx_clip_preprocess + ofx_vit_b32_fwd bit for bit.
 * mean / stdv: the processor's image_mean / image_std (host, 3 floats); size and patch come from the model descriptor. */
size_t ofx_vit_b32_u8_ws_bytes(ofx_handle* h, const int* heights, const int* widths, int N, int channels);
int ofx_vit_b32_fwd_u8(ofx_handle* h, const uint8_t* src, const long long* offsets, const int* heights, const int* widths, int N, int channels,
                       const float* mean, const float* stdv, float* emb, int emb_ld, int emb_col, int normalize, void* ws, size_t ws_bytes,
                       ofx_stream stream);

/* ------------------------------------------------------------------ indexed (varlen) set input ("next" row N3) --- */
/* The same encoder with the outfits given as ROW INDICES into a device-resident embedding table [n_table, ld] fp32
 * (the precomputed-embedding store kept in HBM) instead of a padded [B, L, D] tensor + mask: outfit b holds items
 * item_index[cu_items[b] .. cu_items[b+1]); cu_items[0] = 0; at most max_len (<= 63; <= 31 for the training entry points) items per outfit.  Replaces the
 * reference's collate (outfit_x_base_processor.py:20-81: per-item torch.tensor + cat + stack, then a 12.6 MB/256-outfit
 * H2D copy) by a few KB of indices.  Bit-identical to the dense call on the same items.  Workspace: ofx_workspace_bytes
 * (OFX_OP_SET_ENCODER, B, max_len). */
int ofx_set_encoder_fwd_indexed(ofx_handle* h, const float* table, int ld, long long n_table, const int* item_index, const int* cu_items,
                                const float* prefix, int prefix_stride, int B, int max_len, float* out_row0, void* ws, size_t ws_bytes,
                                ofx_stream stream);

/* ------------------------------------------------------------------ training step ("next" row N1) --- */
/* CP path on precomputed embeddings with a tape, and its backward: what torch autograd computes for the reference's
 * CP trainer step (compatibility_prediction_trainer.py:57-81) with dropout = 0.  Needs outfit_precision BF16 or F16, heads of 64 and
 * d_model in {512, 768, 1024}: every forward and backward entry point of the step returns OFX_ESHAPE at entry on another handle
 * (d_model 1536 scores only).
 * grads: one fp32 buffer, layout from ofx_cp_train_grad_floats (offsets per packed tensor, padded shapes:
 * linear1 [ffn_pad, D], linear2 [D, ffn_pad], ffn_pad = d_ffn rounded up to 128). */
size_t ofx_cp_train_tape_bytes(ofx_handle* h, int B, int L);
size_t ofx_cp_train_ws_bytes(ofx_handle* h, int B, int L);
size_t ofx_cp_train_grad_floats(ofx_handle* h, size_t* offsets, int n_offsets);
/* dropout_p / seed: torch's train-mode dropout (attention probabilities, dropout1, FFN dropout, dropout2 of every layer and
 * the head's nn.Dropout) with stateless masks = hash(seed, site, row, col); the backward call must repeat both values.
 * Same distribution as torch's, not the same random stream. */
int ofx_cp_train_fwd(ofx_handle* h, const float* x, const uint8_t* pad_mask, int B, int L, float* logits, void* tape, size_t tape_bytes,
                     void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream);
int ofx_cp_train_bwd(ofx_handle* h, void* tape, size_t tape_bytes, const float* dlogits, int B, int L, float* grads, size_t grad_floats,
                     void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream);
int ofx_cp_train_fwd_indexed(ofx_handle* h, const float* table, int ld, long long n_table, const int* item_index, const int* cu_items,
                             int B, int max_len, float* logits, void* tape, size_t tape_bytes, void* ws, size_t ws_bytes,
                             float dropout_p, unsigned seed, ofx_stream stream);
/* CIR / FITB path (outfit_x.py:147-172) with a tape and its backward: prefix = [target_item_image_emb | target_text[b]],
 * y [B, d_model] = row0 Wc^T (cir_ffn, no bias, no dropout).  The set is given either padded (x, pad_mask) or indexed
 * (table, ld, n_table, item_index, cu_items) - pass NULL for the form not used.  Gradients land in the same flat buffer
 * (slots: target_item_image_emb, cir_ffn weight, all layer tensors; the CP head's and outfit_token's slots are not written). */
int ofx_cir_train_fwd(ofx_handle* h, const float* x, const uint8_t* pad_mask, const float* table, int ld, long long n_table,
                      const int* item_index, const int* cu_items, const float* target_text, int B, int L, float* y, void* tape,
                      size_t tape_bytes, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream);
int ofx_cir_train_bwd(ofx_handle* h, void* tape, size_t tape_bytes, const float* dy, int B, int L, float* grads, size_t grad_floats,
                      void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream);
/* The same backward passes writing every gradient straight into a caller tensor of the PARAMETER's own shape (linear1 [d_ffn, D],
 * linear2 [D, d_ffn], ...): grad_ptrs = host array of 5 + 12 * n_layers device pointers in pack order (entries of tensors that are
 * not on the path are ignored); accumulate != 0 adds to the existing contents - torch's p.grad += g without the extra kernels. */
int ofx_cp_train_bwd_into(ofx_handle* h, void* tape, size_t tape_bytes, const float* dlogits, int B, int L, float* const* grad_ptrs,
                          int n_ptrs, int accumulate, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream);
int ofx_cir_train_bwd_into(ofx_handle* h, void* tape, size_t tape_bytes, const float* dy, int B, int L, float* const* grad_ptrs,
                           int n_ptrs, int accumulate, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, ofx_stream stream);
/* Data-parallel overlap: arm one hipEvent_t per outfit-transformer layer (events[l], n = n_layers; n = 0 disarms) for the NEXT
 * ofx_*_train_bwd* call on this handle only.  That call records events[l] on its stream as soon as the 12 gradient tensors of layer l
 * (Win, bin, Wo, bo, W1, b1, W2, b2, g1, be1, g2, be2) are final - layers finish last-to-first - so the host can start that
 * layer's gradient all-reduce on another stream while the backward of the layers below still runs (outfitx_amd/trainer.py). */
int ofx_train_arm_layer_events(ofx_handle* h, void* const* events, int n);
/* out[rows, cols] fp32 = keep-mask / (1 - p) of dropout site `site` (layer l: 4l + {0 attention [B*heads, 32*i + j], 1 dropout1,
 * 2 FFN, 3 dropout2}; 4 * n_layers = head), exactly as the kernels compute it.  Test / debugging aid. */
int ofx_dropout_mask(float dropout_p, unsigned seed, int site, int rows, int cols, float* out, ofx_stream stream);
/* FocalLoss(alpha, gamma, mean) forward and d loss / d logits * upstream (src/losses/focal_loss.py:23-41). loss / dlogits may be NULL. */
int ofx_focal_loss(const float* logits, const float* labels, int B, float alpha, float gamma, float upstream, float* loss, float* dlogits,
                   ofx_stream stream);
/* The same with the reference's `reduction` argument (focal_loss.py:36-41): 1 mean, 2 sum, 0 none.  `per_elem` [B] (required for
 * 'none', optional otherwise) receives the unreduced losses; for 'none' dlogits is the per-element derivative (times upstream) and
 * *loss, if given, their sum. */
int ofx_focal_loss_ex(const float* logits, const float* labels, int B, float alpha, float gamma, float upstream, int reduction, float* loss,
                      float* per_elem, float* dlogits, ofx_stream stream);
/* SetWiseRankingLoss(margin) forward and upstream * d loss / d y_hat (src/losses/set_wise_ranking_loss.py:15-36), the CIR trainer's loss
 * (complementary_item_retrieval_trainer.py:79-88), fp32, one pass over the negatives.  Stateless (no handle).
 *   y, y_hat [B, D]; neg [B, K, D] (contiguous; may be NULL when K = 0); neg_mask [B, K], one byte per entry, non-zero = padded
 *   (NULL = nothing padded).  d_pos = ||y_hat - y + 1e-6|| (F.pairwise_distance's eps), d_k = ||y_hat - neg_k||;
 *   *loss = sum over valid (b, k) of relu(d_pos - d_k + margin) / max(#valid in the batch, 1)
 *         + mean over b of relu(d_pos - min over valid k of d_k + margin)       (a row without a valid negative adds 0);
 *   dy_hat [B, D] (may be NULL: value only) = upstream * d loss / d y_hat: relu'(0) = 0, ties for the hardest negative go to the lowest
 *   index, a zero distance contributes a zero direction (never a NaN).  There is no gradient into y or neg.
 *   d_pos [B], d_neg [B, K] (either may be NULL): the distances, for tests and diagnostics; padded entries of d_neg read +inf and their
 *   rows of neg are never loaded.
 * Supported: B >= 1, K >= 0, D % 4 == 0, 4 <= D <= 4096 (else OFX_ESHAPE); y, y_hat, neg, dy_hat 16-byte aligned.  Workspace:
 * the size function below (no alignment beyond 16 bytes; contents need not survive the call).  Two launches; deterministic - no
 * floating-point atomics, two calls on the same inputs return the same bits.  While K * D <= 10240 floats (K <= 10 at D = 1024) a row's negatives
 * stay in LDS between the distance pass and the gradient pass; beyond that the gradient pass re-reads them (outfitx_amd/csrc/rank_loss.hip). */
size_t ofx_set_rank_loss_ws_bytes(int B, int K, int D);
int ofx_set_rank_loss(const float* y, const float* y_hat, const float* neg, const uint8_t* neg_mask, int B, int K, int D, float margin,
                      float upstream, float* loss, float* dy_hat, float* d_pos, float* d_neg, void* ws, size_t ws_bytes, ofx_stream stream);
/* The same loss with the positives and the negatives named by row of a device-resident embedding table (the index form of a CIR batch:
 * no [B, K, D] tensor exists anywhere):  exactly ofx_set_rank_loss with y[b] = table[pos_index[b]] and neg[b, k] = table[neg_index[b, k]] -
 * the same kernel body reading its rows through the indices, the same summation order, hence the same bits as the dense call on the
 * gathered rows, in *loss, dy_hat, d_pos and d_neg alike.
 *   table [n_table, ld] fp32, ld >= D, ld % 4 == 0, 16-byte aligned (a row's first D floats are used); pos_index int32 [B]; neg_index int32
 *   [B, K], contiguous (may be NULL when K = 0).  neg_index[b, k] < 0 means padded - it replaces the mask byte: the row is never loaded and
 *   d_neg reads +inf there.
 *   The index arrays live on the device, so the host cannot check their values: the kernel clamps pos_index into [0, n_table) and a
 *   non-negative neg_index to <= n_table - 1.  A wrong index gives a wrong result, never an access outside the table.
 * NULL or misaligned table / y_hat / dy_hat / ws, NULL pos_index, NULL neg_index with K > 0: OFX_EINVAL; the dense call's shape rules, ld,
 * 1 <= n_table <= INT_MAX: OFX_ESHAPE; short workspace (ofx_set_rank_loss_ws_bytes(B, K, D), unchanged): OFX_EWORKSPACE - a rejected call
 * launches nothing.  Two launches (the first counts neg_index >= 0), no floating-point atomics, bit-reproducible, same LDS residency rule. */
int ofx_set_rank_loss_indexed(const float* table, int ld, long long n_table, const int* pos_index, const int* neg_index, const float* y_hat,
                              int B, int K, int D, float margin, float upstream, float* loss, float* dy_hat, float* d_pos, float* d_neg,
                              void* ws, size_t ws_bytes, ofx_stream stream);

/* ------------------------------------------------------------------ CIR training batches, built on the device --- */
/* One index-form CIR training batch (what ofx_cir_train_fwd and ofx_set_rank_loss_indexed take) drawn where the embedding table lives:
 * PolyvoreComplementaryItemRetrievalDataset.__getitem__ + __get_negative_sample (polyvore_complementary_item_retrieval_dataset.py:50-67,
 * 94-109) and the processor's truncation for B queries at once - the same distributions, not Python's random stream.  Stateless (no handle).
 * The training split and the negative pools, all DEVICE int32 arrays, uploaded once:
 *   outfit_cu [n_outfits + 1], outfit_rows [n_outfit_rows]: outfit o = table rows outfit_rows[outfit_cu[o] .. outfit_cu[o + 1]), 2 .. 64 of them;
 *   pos_cu [n_outfits + 1], pos_slots [n_pos_slots]: the positions inside outfit o that may become the positive (positive_idx_list);
 *   pool_cu [n_pools + 1], pool_rows [n_pool_rows]: the table rows that share a sampling key (semantic_category 'easy', category_id 'hard' -
 *     the easy -> hard switch is a second set of these four arrays), each pool in table order;
 *   row_pool [n_table], row_slot [n_table]: a row's pool (negative = in none) and its position inside that pool;
 *   outfit_ids [B]: the outfits of this batch (the same outfit may appear in several slots: every slot draws on its own).
 * Per query b, o = outfit_ids[b], n items, P eligible positions; word(stream, i) = the 32-bit word of (seed, draw, stream, b, i) and
 * below(u, n) = (u * n) >> 32 (ofx_draw_u32 and ofx_draw_below in outfitx_amd/csrc/ofx_common.h; the bias of below is under n / 2^32):
 *   positive   p = pos_slots[pos_cu[o] + below(word(0, 0), P)];  target_item_index[b] = t = outfit_rows[outfit_cu[o] + p];
 *   remainder  the other n - 1 items in file order j = 0 .. n - 2 get keys word(1, j); ordered by (key, j) ascending - a uniform shuffle -
 *              the first min(n - 1, max_len) go to item_index[cu_seqlens[b] ...];  cu_seqlens [B + 1] = the running sum of those lengths;
 *   negatives  pool g = row_pool[t] of m rows, the target at slot s_t = row_slot[t].  m - 1 >= K: Floyd's algorithm over [0, m - 1): for
 *              s = 0 .. K - 1, j = m - 1 - K + s, v = below(word(2, s), j + 1), slot s takes v, or j when an earlier slot holds v - a uniform
 *              K-subset from K words, no rejection loop; value v names pool slot v + (v >= s_t), i.e. never the target.  m - 1 < K: the other
 *              m - 1 rows in pool order, then -1.  Rows of the query's own outfit are not excluded (the reference does not either).
 * Outputs (DEVICE int32): item_index [B * max_len], compact - elements at or past cu_seqlens[B] are NOT written; cu_seqlens [B + 1];
 * target_item_index [B]; neg_items_index [B, K], -1 = empty slot (NULL when K = 0).
 * Two launches on `stream` (the scan of the lengths, then one wave per query), no workspace, allocation, copy or wait (capturable).  A pure
 * function of its arguments: the same (seed, draw) repeats the batch to the bit; tests/cir_sampler_ref.py restates it in numpy.
 * Checked: a NULL pointer, a pointer that is not 16-byte aligned, B < 1: OFX_EINVAL; K outside [0, 64], max_len outside [1, 31] (the training
 * step's limit), n_outfits < 1, n_table < 1, another count negative, B * max(K, max_len) > INT_MAX: OFX_ESHAPE; a refused call launches
 * nothing.  The host cannot see the arrays' contents: the kernels clamp every value they index with into its array (by the counts given
 * here), so a wrong table gives wrong draws, never an access out of bounds. */
int ofx_cir_sample_batch(const int* outfit_cu, const int* outfit_rows, int n_outfits, int n_outfit_rows, const int* pos_cu, const int* pos_slots,
                         int n_pos_slots, const int* pool_cu, const int* pool_rows, int n_pools, int n_pool_rows, const int* row_pool,
                         const int* row_slot, int n_table, const int* outfit_ids, int B, unsigned seed, unsigned draw, int K, int max_len,
                         int* item_index, int* cu_seqlens, int* target_item_index, int* neg_items_index, ofx_stream stream);

/* ------------------------------------------------------------------ optimizer step ---------- */
/* The accumulation boundary of the trainers (compatibility_prediction_trainer.py:70-80 = complementary_item_retrieval_trainer.py:89-99):
 * torch.nn.utils.clip_grad_norm_(max_norm) -> torch.optim.AdamW step (amsgrad off, maximize off) -> zero the gradient, over ONE flat
 * fp32 gradient arena (outfitx_amd/trainer.py FlatGrads).  Stateless (no handle): with ofx_*_train_bwd* writing the gradients, a caller
 * without torch can train.
 *   grad, exp_avg, exp_avg_sq: arenas of n_arena floats in the same layout - every tensor starts at a multiple of 64 floats, the gaps
 *   between tensors are padding (zero).  The parameters stay wherever the caller keeps them: segments[i] says that arena floats
 *   [offset, offset + numel) belong to the fp32 tensor at `param`.  The table is a DEVICE array, sorted by offset, non-overlapping, every
 *   offset a multiple of 64 and every param 16-byte aligned; it is only read, so it can be built once.  The host cannot see it and
 *   checks none of this.
 *   g     = grad_scale * grad                        (whole arena, padding included; grad_scale = 1 / world folds the mean over ranks in)
 *   norm  = ||g||_2;  *grad_norm = norm              (before clipping, what clip_grad_norm_ returns)
 *   norm not finite:  *skipped = 1, grad := 0, and the parameters, both moments and *step are left as they were
 *   otherwise:        *skipped = 0;  t = *step + 1;  *step = t      (*step is a float, as torch keeps it; 0 before the first step)
 *                     g *= min(max_norm / (norm + 1e-6), 1)
 *                     param *= 1 - lr * weight_decay
 *                     exp_avg += (g - exp_avg) * (1 - beta1);   exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * g * g
 *                     param -= lr / (1 - beta1^t) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)
 *                     grad := 0                      (every float of the arena, padding included)
 *   Element arithmetic is fp32; the sum of squares, 1 - lr * weight_decay, the bias corrections 1 - beta^t and the clip coefficient
 *   (from the fp32 norm it reports) are computed in double from the double arguments, as torch computes them from Python floats.
 *   Nothing is read or written beyond param + numel; the moments' padding is not written.  grad_norm, skipped, step: 1 element each.
 * Supported: 1 <= n_segments <= 1024, n_arena > 0 and a multiple of 64 (else OFX_ESHAPE); a NULL pointer, or grad / exp_avg /
 * exp_avg_sq / ws not 16-byte aligned: OFX_EINVAL; ws_bytes below the size function: OFX_EWORKSPACE.  A rejected call launches nothing.
 * Workspace: the size function below (0 for an unsupported n_arena); contents need not survive the call.  Two launches on `stream`, no
 * allocation, copy or wait (capturable); deterministic - no atomics, two calls from the same state return the same bits
 * (outfitx_amd/csrc/optim.hip). */
typedef struct ofx_opt_segment { float* param; long long offset; long long numel; } ofx_opt_segment;
size_t ofx_adamw_step_ws_bytes(long long n_arena);
int ofx_adamw_step(const ofx_opt_segment* segments, int n_segments, float* grad, float* exp_avg, float* exp_avg_sq, long long n_arena,
                   float* step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double grad_scale,
                   float* grad_norm, int* skipped, void* ws, size_t ws_bytes, ofx_stream stream);
/* The same boundary behind a dynamic loss scale: torch.amp.GradScaler's unscale_ -> clip_grad_norm_ -> step -> update as one call, for
 * training with f16 operands (the arena then holds *loss_scale times the gradient, because the loss was multiplied by it before the
 * backward).  Arguments, workspace, refusals and guarantees of ofx_adamw_step, plus the scaler's state, which lives on the device and is
 * read AND rewritten: loss_scale (1 float) and growth_tracker (1 int, the unskipped steps since the scale last changed).
 *   g     = (grad_scale * (float)(1.0 / *loss_scale)) * grad      (one fp32 factor; exact for a power-of-two scale)
 *   norm, *grad_norm, *skipped, the update and the zeroing: as above on this g - *grad_norm is the UNSCALED norm
 *   skipped:    *loss_scale *= backoff_factor;  *growth_tracker = 0
 *   otherwise:  *growth_tracker += 1;  when it equals growth_interval: *loss_scale *= growth_factor (kept as it is if the product is not
 *               finite), *growth_tracker = 0.  The products are formed in double and stored as float, as torch does.
 * Additionally refused, before anything is launched: loss_scale / growth_tracker NULL or not 4-byte aligned (OFX_EINVAL); growth_factor
 * < 1, backoff_factor outside (0, 1] or growth_interval < 1, NaNs included (OFX_EINVAL).  Same workspace size; still two launches, no
 * atomics, nothing read back. */
int ofx_adamw_step_scaled(const ofx_opt_segment* segments, int n_segments, float* grad, float* exp_avg, float* exp_avg_sq, long long n_arena,
                          float* step, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double grad_scale,
                          float* loss_scale, int* growth_tracker, double growth_factor, double backoff_factor, int growth_interval,
                          float* grad_norm, int* skipped, void* ws, size_t ws_bytes, ofx_stream stream);

/* ------------------------------------------------------------------ profiling --------------- */
/* HIP-event timing of every launch, by category {0 GEMM, 1 norm/embed, 2 attention, 3 other}.
 * enable(mask) clears and starts recording the categories in the bit mask (1 GEMM | 2 norm | 4 attention | 8 other; 0 = off); read() waits for the events (host sync) and returns the
 * summed milliseconds, executed FLOPs (GEMM only) and launch counts; arrays of 4.  Process-global, not thread-safe: benchmarks and tests only. */
void ofx_profile_enable(int on);
int ofx_profile_read(double* ms, double* flops, long long* launches);
/* Per-launch records of the last recording, in launch order (call BEFORE ofx_profile_read, which clears them).  GEMM records carry
 * their shape and kernel: M, N, K (logical depth), kmul (executed K = kmul x K: 2 split weights [hi | lo], 3 three-product
 * K-concatenation) and kind (1 128x128 tile kernel incl. its split-K / 64-row variants, 2 256x256, 3 256x128, 4 256x256 ping-pong,
 * 6 dual-weight 256x256, 7 fused QKV projection + attention); flops = executed FLOPs; bytes = ALGORITHMIC HBM bytes of the launch (every operand
 * read once - A [M, K], the weight rows as stored - and every output / in-place stream element read and written once, as the
 * launch's epilogue is configured).  Returns the count. */
typedef struct ofx_prof_record { int cat, M, N, K, kind, kmul; float ms; double flops; double bytes; } ofx_prof_record;
int ofx_profile_records(ofx_prof_record* out, int cap);

/* Process-wide tuning knobs (benchmarks / tests only).  Unknown knobs return OFX_EINVAL.
 * knob 2: GEMM kernel, 0 (default) = the automatic choice, 1 = 128x128, 2 = 256x256, 3 = 256x128, 4 = 256x256 ping-pong, 5 = 64x128,
 *         6 = the dual-weight 256x256 kernel for split weights (every other GEMM keeps the automatic choice);
 * knob 5: split-K of small GEMMs, 1 (default) = planned, 0 = never, >= 2 = forced (low byte = splits, bit 8 = 64-row tiles; a forced value whose
 *         low byte is 0 names no slices and is OFX_EINVAL);
 * knob 6: accepts only 2, the one tower form (a no-op kept for callers that set it): the CLIP towers' LayerNorms are folded into the
 *         neighbouring GEMM epilogues and their residual stream is an operand-type (hi, lo) pair updated in place; 0 and 1 (fp32 stream,
 *         materialised LayerNorms) are retired and return OFX_EINVAL;
 * knob 7: 1 (default) single-product precisions (training; scoring in bf16 / f16) run the MFMA varlen attention, 0 the fp32 set kernels;
 * knob 8: 1 (default) the ViT's last layer computes queries for the CLS rows only, 0 runs the full QKV GEMM;
 * knob 9: bit 0 (default on) / bit 1 (default off): ViT layers with single-product / split (hi, lo) q | k | v weights run the fused
 *         QKV-projection + attention kernel; cleared: the GEMM -> HBM -> attention-kernel pair;
 * knob 10: 1 (default) small-batch outfit-transformer GEMMs (split-K plans) leave their second pass to the consumer kernel (set
 *          attention sums the q | k | v slabs; reduce + LayerNorm in one launch), 0 the separate reduce and LayerNorm launches;
 * knob 11: grid size of the persistent dual-weight GEMM (default -1 = one block per CU of the device, each walking its tiles and
 *          fetching the next tile's first k-steps under the current epilogue), 0 = one block per tile.
 * knob 15: three-product GEMMs: 1 (default) the operand-tiles-loaded-once kernel from 192 tiles on, 2 always, 0 never.
 * knob 16: 1 (default) gemm_x3_kernel launches one block per CU walking its tiles, 0 = one block per tile (short-lived blocks).
 * knob 17: 1 (default) ofx_l2_topk on pools of >= 32,768 rows runs sample + filter (the distance matrix is never written), 0 = always
 *          distance matrix + radix select.  Same results either way.
 * knob 18: 1 (default) the split-weight GEMM's f16 outputs (qkv, fc1) are stored straight from the accumulator layout, 0 = through the LDS
 *          transpose of rounds 1-3; any other value is OFX_EINVAL.  Bit-identical results.
 * knob 20: validation only, default 0: 1 = a three-product ViT (vit_x3) keeps q | k | v in fp32 and runs the fp32 attention kernel instead of the MFMA attention
 *          on operand-rounded q | k | v (several times slower; tools/parity_selfcheck.py uses it for its reference run).
 * knob 21: 1 (default) ofx_clip_text_fwd_shared honours its shared_first flag, 0 = it runs the full rows (A/B runs and tests).
 * knob 22: 1 (default) ViT layers with split q | k | v weights and their fp8 copy run the fused QKV-projection + attention kernel's fp8-correction
 *          variant wherever the qkv GEMM would run as gemm_w2f8_kernel (f16 operands, >= 256 tiles of 256 x 256), 0 = the GEMM -> HBM ->
 *          attention-kernel pair.  Bit-identical results.  Independent of knob 9, whose bits keep their meaning. */
int ofx_tune(int knob, int value);
/* A counter that every ofx_tune call bumps, and whether per-launch profiling events are being recorded: the host mirror replays a
 * stream-captured forward (outfitx_amd/graphs.py) only while the counter still has the value it had at capture time and no recording
 * is on (events ride on launches; a replayed graph issues none). */
unsigned ofx_config_generation(void);
int ofx_profile_enabled(void);
/* A HIP stream of the LOWEST dispatch priority on `device` (hipStreamCreateWithPriority, non-blocking): the host mirror runs the text tower on it
 * beside the ViT on the caller's stream, so that its workgroups take CUs only when the caller's stream has none ready.  Caller destroys it. */
int ofx_stream_create_low_priority(int device, ofx_stream* out);
int ofx_stream_destroy(ofx_stream stream);

/* ------------------------------------------------------------------ op level (tests) ------- */
int ofx_gemm(const void* A, const void* W, void* C, const float* bias, const float* resid, int M, int N, int K,
             int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, ofx_stream stream);
/* The same against a SPLIT weight matrix W2 [N, 2K], row n = [hi(K) | lo(K)] (ofx_convert mode 3): C = A (hi + lo)^T + ... with one
 * copy of A - two MFMA products per weight, ~22 significant weight bits.  K multiple of 64. */
int ofx_gemm_w2(const void* A, const void* W2, void* C, const float* bias, const float* resid, int M, int N, int K,
                int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, ofx_stream stream);
/* Three-product GEMM: A3 [M, lda >= 3K] rows [hi | lo | hi], W3 [N, 3K] rows [hi | hi | lo] (ofx_convert mode 2), C = hi.hi + lo.hi + hi.lo.
 * From 192 tiles of 256 x 128 on (ofx_tune(15, 2): always; 0: never) the kernel that stages each operand tile once (gemm_x3.hip), else the
 * K-concatenated single-product kernels on K' = 3K.  K multiple of 32, N of 128. */
int ofx_gemm_x3(const void* A3, const void* W3, void* C, const float* bias, const float* resid, int M, int N, int K,
                int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, ofx_stream stream);
/* The same with the correction product A . lo^T on the block-scaled fp8 matrix instruction (2x the f16 rate; f16 operands only):
 * ofx_pack_lo8 turns the lo halves of W2 [N, 2K] into W8 [N, K] e4m3 bytes (per row scaled to max |lo| 2^sw in [128, 256), the
 * 128-blocks k-permuted as the kernel's in-register fp8 activation image is) + scale8 [N] E8M0 bytes; N and K multiples of 128.
 * ofx_gemm_w2f8 = A hi^T + bf8(A 2^shift) fp8(lo 2^sw)^T 2^-(shift + sw): the weight error drops from 2^-12 to ~2^-15 relative, the
 * activation operand stays the one f16 copy.  Since round 4 the in-register activation image is E5M2 (f16's exponent range, 3 significant bits,
 * shift 0): it follows any finite f16 operand - no magnitude precondition on A; values above 57,344 are clamped there (rounds 3's e4m3 image
 * saturated at |a| > 112 and then corrected such a column only in part).  Small problems (fewer than 256 tiles of 256 x 256) run ofx_gemm_w2's path on W2. */
int ofx_pack_lo8(const void* W2, void* W8, void* scale8, int N, int K, ofx_stream stream);
int ofx_gemm_w2f8(const void* A, const void* W2, const void* W8, const void* scale8, void* C, const float* bias, const float* resid, int M, int N, int K,
                  int lda, int ldc, int ldr, int act, int out_kind, ofx_stream stream);
/* The same as a LayerNorm-fold consumer, as the ViT layers launch it for qkv and fc1: C [M, ldc >= N] in the operand type (f16) =
 * act( (A hi^T + bf8(A) fp8(lo)^T - col_sum[n] mean[m]) rstd[m] + bias[n] ), row_stat [M, 2] = (mean, rstd) per row, col_sum [N].  No residual. */
int ofx_gemm_w2f8_fold(const void* A, const void* W2, const void* W8, const void* scale8, void* C, const float* bias, const float* row_stat, const float* col_sum,
                       int M, int N, int K, int lda, int ldc, int act, ofx_stream stream);
/* Weight-gradient GEMM of the training step: C[M,N] fp32 = sum_k A[k, m] * B[k, n]; A [K, lda] and B [K, ldb] row-major
 * operand-type matrices whose ROW index is contracted (dW = dY^T X without transposed copies).  M, N multiples of 256.
 * k_dev: optional device-side live row count (<= K).  Both operands must be readable up to round_up(K, 64) rows.
 * slab: ofx_gemm_tn_ws(M,N,K) bytes of scratch for the deterministic split-K (NULL = no split). */
size_t ofx_gemm_tn_ws(int M, int N, int K);
int ofx_gemm_tn(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K, const int* k_dev,
                void* slab, size_t slab_bytes, int op_dtype, ofx_stream stream);
/* ofx_gemm with split-K scratch: slab of ofx_gemm_splitk_ws(M,N,K) bytes (0 = the shape is not split) */
size_t ofx_gemm_splitk_ws(int M, int N, int K);
int ofx_gemm_splitk(const void* A, const void* W, void* C, const float* bias, const float* resid, int M, int N, int K,
                    int lda, int ldc, int ldr, int act, int out_kind, int op_dtype, void* slab, size_t slab_bytes, ofx_stream stream);
/* The non-attention kernels of the training backward, one call each.  A dropout site is (dropout_p, seed, site) exactly as the step
 * builds it: mask element (row, col) is what ofx_dropout_mask returns for the same arguments, dropout_p = 0 is no dropout.  NULL required
 * pointers, misaligned pointers and dropout_p outside [0, 1) are OFX_EINVAL, an unsupported shape OFX_ESHAPE, a short workspace
 * OFX_EWORKSPACE; a refused call launches nothing.  `m_dev`, where taken, is an optional device-side live row count: the kernels use
 * min(*m_dev, M) rows and neither read nor write rows from there on, except as said under ofx_gemm_train.
 *
 *   ofx_gemm_train: ofx_gemm_splitk with the training epilogue: C = drop(act(A W^T + bias)) + resid, and for OFX_ACT_MISH_GRAD
 *     C = drop(A W^T + bias) * mish'(resid) (resid, required then, is the saved pre-activation).  aux_out: optional fp32 [M, N] copy of
 *     A W^T + bias before activation and dropout (row stride N).  Mask element = (output row, output column).  Live rows are written in
 *     full and nothing at or past row M is touched; rows [*m_dev, M) of C and aux_out are not written by any kernel of the dispatcher
 *     (128- and 64-row tiles, 256x256, 256x128, ping-pong, split-K reduce: tiles past the live rows leave at once, the operand loads
 *     clamp onto the last live row, the epilogues and the reduce stop at the live count), and those rows of A and resid are not read:
 *     they may hold anything.  tests/test_gpu_bwd_ops.py holds every kernel to this.
 *   ofx_gemm_tn_into: ofx_gemm_tn storing only C[:m_valid, :n_valid] (0 = all; n_valid a multiple of 4; ldc >= n_valid may be < N),
 *     accumulate: C += the product instead of C = (one fp32 addition per element, after the split-K sum).  Nothing else of C is written.
 *   ofx_transpose_cast: dst [C, ldd >= R] operand type = round-to-nearest-even cast of src [R, C] fp32 transposed; columns R .. ldd - 1 of
 *     dst are not written.  row_dst: optional row-major copy [R, ld_row >= C] of the same cast, columns C .. ld_row - 1 not written.
 *   ofx_layernorm_bwd: rows r < min(*m_dev, M) of fp32 [M, D] dy and x, stats [M, 2] = (mean, rstd) of x's rows, gamma [D]:
 *         g = dy gamma, xh = (x - mean) rstd, dx[r] = rstd (g - mean(g) - xh mean(g xh)) + addend,
 *     addend = add[r] (add_map NULL), add[add_map[r]] (add_map[r] >= 0) or nothing (add NULL or add_map[r] < 0).  dx fp32 [M, D];
 *     dx_op [M, D] operand type = cast(dx . mask of the site) - dx itself stays undropped.  Column sums over the live rows, each optional:
 *     dgamma = sum dy xh, dbeta = sum dy, dcols = sum dx . mask (the fp32 values before the cast); accumulate: += instead of =.
 *     D in {512, 768, 1024}; ws: ofx_layernorm_bwd_ws(D) bytes (0 for another D).  Rows at or past the live count are not written.
 *   ofx_colsum: out_k[c % seg] (+)= sum over r < min(*m_dev, M) of row_scale[r] * x[gather ? gather[r] : r][c], k = c / seg, for the
 *     columns c < C with c % seg < valid (valid = 0: seg); NULL out_k: that segment is skipped.  x: fp32 (x_kind 0) or the operand
 *     type (x_kind 1), row stride ld >= C.  C and ld multiples of 4, C <= 3 seg, M >= 1.  ws: ofx_colsum_ws(C) bytes.  A live count of 0
 *     stores zeros (accumulate: leaves the outputs as they are).
 *   ofx_head_bwd: block b writes row r = cu ? cu[b] : b of dX (fp32 [rows, D]) and dXb (operand type): CP mode (dlogits given, w [D]):
 *     dX[r] = dlogits[b] * w * mask_head(b, c); CIR mode (dlogits NULL, w [B, D] ready row gradients, db must be NULL): dX[r] = w[b] *
 *     mask_head(b, c) - w may alias dX when cu is NULL.  dXb[r] = cast(dX[r] * mask_below(r, c)).  db (CP mode, optional): db[0] (+)=
 *     sum_b dlogits[b].  A negative site = no dropout there.  Other rows of dX and dXb are not written.  D a multiple of 4. */
int ofx_gemm_train(const void* A, const void* W, void* C, const float* bias, const float* resid, float* aux_out, int M, const int* m_dev,
                   int N, int K, int lda, int ldc, int ldr, int act, int out_kind, float dropout_p, unsigned seed, int site, int op_dtype,
                   void* slab, size_t slab_bytes, ofx_stream stream);
int ofx_gemm_tn_into(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K, const int* k_dev,
                     int m_valid, int n_valid, int accumulate, void* slab, size_t slab_bytes, int op_dtype, ofx_stream stream);
int ofx_transpose_cast(const float* src, void* dst, int R, int C, int ldd, void* row_dst, int ld_row, int op_dtype, ofx_stream stream);
size_t ofx_layernorm_bwd_ws(int D);
int ofx_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, const float* add, const int* add_map,
                      float* dx, void* dx_op, float* dgamma, float* dbeta, float* dcols, int M, const int* m_dev, int D, float dropout_p,
                      unsigned seed, int site, int accumulate, int op_dtype, void* ws, size_t ws_bytes, ofx_stream stream);
size_t ofx_colsum_ws(int C);
int ofx_colsum(const void* x, int x_kind, int ld, const int* gather, const float* row_scale, float* out0, float* out1, float* out2, int seg,
               int C, int valid, int M, const int* m_dev, int accumulate, int op_dtype, void* ws, size_t ws_bytes, ofx_stream stream);
int ofx_head_bwd(const float* dlogits, const float* w, const int* cu, float* dX, void* dXb, float* db, int B, int D, float dropout_p,
                 unsigned seed, int head_site, int below_site, int accumulate, int op_dtype, ofx_stream stream);
/* The kernels of the towers' LayerNorm-fold chain (knob 6), one call each, through the launchers the ViT and text layers use.  The residual
 * stream is an operand-type pair (hi at xb, lo = x - hi at xlo); no LayerNorm is materialised.  NULL required pointers, misaligned pointers
 * and an op_dtype that is not OFX_BF16 / OFX_F16 are OFX_EINVAL, an unsupported shape OFX_ESHAPE; a refused call launches nothing.
 * w_form names the weight operand: 0 = plain W [N, K]; 1 = split W2 [N, 2K], row n = [hi(K) | lo(K)] (ofx_gemm_w2); 2 = split plus the fp8
 * copy (W8, scale8) of its lo half (ofx_gemm_w2f8; f16 only, N and K multiples of 128).  W8 / scale8 are ignored for w_form 0 and 1.  The
 * kernel is chosen as for ofx_gemm / ofx_gemm_w2 / ofx_gemm_w2f8: knob 2 and knob 11 apply.
 *
 *   ofx_gemm_fold_producer: the out-proj / fc2 form.  v = fp32(A W^T + bias) + (fp32(xb) + fp32(xlo)), per element; xb := cast(v),
 *     xlo := cast(v - xb), both [M, N] with row stride N, updated IN PLACE; stat_part [M, N / 64, 2] fp32 = per row and 64-column segment
 *     (sum of v, sum of v^2), of the fp32 v before the split.  Rows at or past M of xb, xlo and stat_part are not touched.  N a multiple
 *     of 128 (OFX_ESHAPE); act must be OFX_ACT_NONE and resid NULL - the stream is the residual - else OFX_EINVAL (they are taken so that
 *     the launcher's refusal can be reached).  A, W, W8, xb, xlo, bias 16-byte aligned, stat_part 8-byte aligned.
 *   ofx_gemm_fold: the qkv / fc1 form for w_form 0 and 1 (w_form 2 is ofx_gemm_w2f8_fold, which stays):  C [M, ldc >= N] operand type =
 *     act((A W^T - col_sum[n] mean[m]) rstd[m] + bias[n]), (mean, rstd)[m] = row_stat[2 m stat_ld], [2 m stat_ld + 1]; columns N .. ldc - 1
 *     are not written.  W holds the gamma-scaled rows and col_sum, bias what ofx_fold_pack returns.  stat_ld >= 1 (with lda = stat_ld K:
 *     every stat_ld-th row of a stream, the pruned last ViT layer).  row_stat and col_sum are required (OFX_EINVAL); no residual.
 *   ofx_stats_finalize: stat [rows, 2] = (mean, rstd) from stat_part [rows, slots, 2]: s = sum of the slots' sums, q = of their sums of
 *     squares, in slot order; mean = s / W, rstd = rsqrt(max(q / W - mean^2, 0) + eps), all fp32 - ONE pass: the relative error of rstd
 *     grows as 2^-24 E[x^2] / Var[x] (tests/test_gpu_fold_ops.py holds the kernel to the derived bound).
 *   ofx_row_stats_cast: x fp32 [rows, W] -> xb = cast(x), xlo = cast(x - xb), stat [rows, 2] = two-pass (mean, rstd) of x's rows.  W % 4 == 0.
 *   ofx_fold_pack: w fp32 [N, K], gamma, beta [K], bias [N] -> wf [N, K] = cast(fp32(w gamma)), or with split != 0 wf [N, 2K] = [hi | lo],
 *     lo = cast(fp32(w gamma) - hi); col_sum [N] = the fp32 sum of the ROUNDED values wf holds (hi and lo); bias_f [N] = bias + sum_k beta[k] w[n, k].
 *   ofx_vit_embed_ln: row n S + t = LN((t == 0 ? cls : patch_out[n (S - 1) + t - 1]) + pos[t]) gamma + beta, patch_out fp32 [N (S - 1), D],
 *     cls, gamma, beta [D], pos [S, D].  Writes EITHER x fp32 [N S, D], OR the stream form of the same values: xb = cast(x), xlo = cast(x - xb)
 *     and stat [N S, 2] = two-pass (mean, rstd) of x's rows.  Passing both or neither is OFX_EINVAL.  D in {512, 768, 1024} (OFX_ESHAPE).
 *   ofx_gather_hilo: dst fp32 [rows, W] = fp32(hi[idx[r]]) + fp32(lo[idx[r]]), hi and lo operand type [*, W], W % 4 == 0.  idx lives on the
 *     device and is not checked: every entry must name a row of hi / lo. */
int ofx_gemm_fold_producer(const void* A, const void* W, const void* W8, const void* scale8, void* xb, void* xlo, float* stat_part, const float* bias,
                           const float* resid, int M, int N, int K, int lda, int ldr, int act, int w_form, int op_dtype, ofx_stream stream);
int ofx_gemm_fold(const void* A, const void* W, void* C, const float* bias, const float* row_stat, int stat_ld, const float* col_sum, int M, int N, int K,
                  int lda, int ldc, int act, int w_form, int op_dtype, ofx_stream stream);
int ofx_stats_finalize(const float* stat_part, int slots, int W, float eps, float* stat, int rows, ofx_stream stream);
int ofx_row_stats_cast(const float* x, void* xb, void* xlo, float* stat, int rows, int W, float eps, int op_dtype, ofx_stream stream);
int ofx_fold_pack(const float* w, const float* gamma, const float* beta, const float* bias, void* wf, float* col_sum, float* bias_f, int N, int K, int split,
                  int op_dtype, ofx_stream stream);
int ofx_vit_embed_ln(const float* patch_out, const float* cls, const float* pos, const float* gamma, const float* beta, float* x, void* xb, void* xlo,
                     float* stat, int N, int S, int D, float eps, int op_dtype, ofx_stream stream);
int ofx_gather_hilo(const void* hi, const void* lo, const int* idx, float* dst, int rows, int W, int op_dtype, ofx_stream stream);
int ofx_layernorm(const float* x, const int* row_idx, const float* gamma, const float* beta, void* y, int rows,
                  int D, int ldy, int out_kind, int op_dtype, float eps, ofx_stream stream);
/* MFMA attention over fixed-length sequences of 1 .. 256 rows (the CLIP towers; up to 64 rows one wavefront holds the whole sequence, 65 ..
 * 256 rows - ViT-B/16: 197 - take a workgroup per (sequence, head) with the same roundings; seq_len > 256: OFX_ESHAPE): qkv [nseq * seq_len, ld] operand type, q at column 0, k at
 * k_off, v at v_off, head h at + 64 h; out [nseq * seq_len, ldo] operand type = softmax(q k^T * scale + mask) v, columns n_head * 64 .. ldo - 1
 * not written.  key_mask: optional int64 [nseq, mask_ld], 0 = key ignored; causal: key j > query i ignored.  ld, k_off, v_off multiples of 8,
 * ldo of 4 (OFX_ESHAPE); qkv 16-byte and out 8-byte aligned (OFX_EINVAL).
 * A FULLY MASKED QUERY ROW (key 0 masked under the causal mask; a sequence whose mask is all zero) has probabilities 0, so its output row is
 * exactly 0 - in all three copies of a split3 row.  This is the library's own rule for both attention kernels (this one and the fp32 one
 * below); HF's result for such a row depends on its version. */
int ofx_attention(const void* qkv, void* out, const int64_t* key_mask, int nseq, int seq_len, int n_head, int ld,
                  int ldo, int k_off, int v_off, int mask_ld, int causal, float scale, int op_dtype, ofx_stream stream);
/* ofx_attention plus the two fields of its launcher that ofx_attention cannot set, as the towers launch it:
 *   only_row0 != 0: only query row 0 of every sequence (row b * seq_len of out) is computed and stored, the same bits as the full call's;
 *     every other row of out is not written (the pruned last ViT layer).
 *   split3_w = W > 0: out rows are [hi(W) | lo(W) | hi(W)] (the A operand of a three-product GEMM): hi = cast(o) at columns 64 h .., lo =
 *     cast(o - hi) at W + 64 h .., hi again at 2 W + 64 h ..; W a multiple of 8, ldo >= 3 W (OFX_ESHAPE); columns 3 W .. ldo - 1 and, where
 *     W > n_head * 64, the columns between the copies are not written.  split3_w = 0: ofx_attention's rows.
 * NULL qkv / out and an op_dtype that is not OFX_BF16 / OFX_F16 are OFX_EINVAL; split3_w < 0, a key_mask with mask_ld < seq_len and what
 * ofx_attention refuses are OFX_ESHAPE.  A refused call launches nothing. */
int ofx_attention_ex(const void* qkv, void* out, const int64_t* key_mask, int nseq, int seq_len, int n_head, int ld, int ldo, int k_off,
                     int v_off, int mask_ld, int causal, int only_row0, int split3_w, float scale, int op_dtype, ofx_stream stream);
/* fp32 VALU attention over varlen sets (the outfit transformer): qkv fp32 [rows, 3 D] (q | k | v), sequence b = rows cu_seqlens[b] ..
 * cu_seqlens[b + 1] (1 .. max_len <= 64 of them), D = n_head * 64 or n_head * 96 (any other head width: OFX_ESHAPE), head h at columns
 * D / n_head * h.  out [rows, ldo]: out_kind 0 fp32 | 1 operand type | 2 [hi(D) | lo(D) | hi(D)] (ldo >= 3 D); operand-type rows need
 * ldo % 8 == 0.  only_row0: query row 0 of every set alone is computed and stored.  scale: the caller's, 1 / sqrt(head width) in the
 * outfit transformer.  Heads of 96 (d_model 1536 = 16 x 96, the reference's default SigLIP width) run their own instances of the
 * kernel: one wavefront per (set, head) as at 64, lanes 0 .. 31 owning a second column; every row count of the 64-wide instances is
 * kept (the 64-row instance declares 68.6 KB of LDS, inside gfx950's 160 KiB per workgroup), so no set is refused at 96 that runs at 64.
 * The same holds for ofx_set_attention_slabs, ofx_set_attention_op and ofx_attention_f32, which launch this kernel. */
int ofx_set_attention(const float* qkv, void* out, const int* cu_seqlens, int nseq, int n_head, int D, int ldo,
                      int out_kind, int max_len, int only_row0, float scale, int op_dtype, ofx_stream stream);
/* ofx_set_attention reading q | k | v from the QKV GEMM's split-K slabs (small-batch scores): slabs fp32 [splits][rows, 3 D], slab s at
 * slabs + s * plane_floats, bias fp32 [3 D]; element = (((s0 + s1) + ...) + s_{splits-1}) + bias, fp32 additions in exactly that order, so
 * the result equals ofx_set_attention on that array bit for bit.  Under only_row0 q of rows > 0 is not read.  splits = 1 is ofx_set_attention
 * itself (bias and plane_floats unused).  slabs, bias and out 16-byte aligned, plane_floats a multiple of 4, no NULL among slabs, out,
 * cu_seqlens, nseq >= 1, splits >= 1, op_dtype OFX_BF16 / OFX_F16 (else OFX_EINVAL); with splits > 1 the launcher's own rules: max_len <= 32,
 * bias given, plane_floats > 0 (OFX_EINVAL).  out_kind outside 0 .. 2 and what ofx_set_attention refuses are OFX_ESHAPE.  A refused call
 * launches nothing. */
int ofx_set_attention_slabs(const float* slabs, size_t plane_floats, int splits, const float* bias, void* out, const int* cu_seqlens, int nseq,
                            int n_head, int D, int ldo, int out_kind, int max_len, int only_row0, float scale, int op_dtype, ofx_stream stream);
/* Split-K second pass fused with the LayerNorm behind it (small batches of the outfit transformer), for the rows r < min(*m_dev, rows)
 * (m_dev NULL: rows):  x[r] = ((((s0[r] + s1[r]) + ...) + bias) + resid[r]), fp32 additions in that order, then y[r] = LN(x[r]) gamma + beta
 * with two-pass fp32 statistics (agrees with ofx_layernorm to fp32 rounding, not bit for bit: the sums take another order).
 * slab fp32 [splits][rows, D], slab s at slab + s * plane_floats; bias [D] and resid [rows, ldr] optional, resid may alias x; x fp32
 * [rows, ldx]; y [rows, ldy]: out_kind 0 fp32 | 1 operand type | 2 [hi(D) | lo(D) | hi(D)] (ldy >= 3 D).  Columns D .. of x, the columns of y
 * behind its D (3 D) and all rows at or past the live count are not written.  D in {512, 768, 1024, 1536}, ldx, ldr, ldy multiples of 4 and >= D,
 * rows >= 1, splits >= 1, slabs that do not overlap (OFX_ESHAPE); NULL slab / x / gamma / beta / y, pointers off 16 bytes (y: 8 for the
 * operand-type kinds, m_dev: 4), plane_floats % 4 != 0, a bad op_dtype: OFX_EINVAL.  A refused call launches nothing. */
int ofx_splitk_reduce_ln(const float* slab, size_t plane_floats, int splits, const float* bias, const float* resid, int ldr, float* x, int ldx,
                         const float* gamma, const float* beta, void* y, int ldy, int out_kind, float eps, int rows, const int* m_dev, int D,
                         int op_dtype, ofx_stream stream);
/* The attention kernels of the training step, one call each (both settings of knob 7).  q | k | v and dqkv are operand-type rows [rows, 3 D]
 * (the tape's layout), sequence b = rows cu_seqlens[b] .. cu_seqlens[b + 1] (1 .. max_len of them, never none), head h at columns 64 h.
 * The MFMA kernels and both backward kernels are built for heads of 64 only: ofx_attention_varlen wants k_off = n_head * 64, v_off = 2 k_off
 * and ld >= 3 k_off, ofx_set_attention_bwd D = n_head * 64 (else OFX_ESHAPE, nothing launched); ofx_set_attention_op also takes heads of 96.
 * Dropout on the attention probabilities is site `site` of (dropout_p, seed): mask element (b * n_head + h, query * 32 + key), the values
 * ofx_dropout_mask returns for the same arguments; dropout_p = 0 is no dropout, dropout needs max_len <= 32 (OFX_ESHAPE).  NULL pointers,
 * nseq <= 0 and dropout_p outside [0, 1) are OFX_EINVAL; a refused call launches nothing.
 *   ofx_attention_varlen: the MFMA forward (knob 7 = 1): out [rows, ldo] operand type; only_row0: query row 0 of every sequence alone
 *     is computed and stored (row cu_seqlens[b]), the other rows of out are not written.
 *   ofx_set_attention_op: the VALU forward (knob 7 = 0), ofx_set_attention on operand-type q | k | v.
 *   ofx_set_attention_bwd: d_o fp32 [rows, D], or [nseq, D] with only_row0 (the gradient of query row 0 of every sequence; the other
 *     queries have none); dqkv = dq | dk | dv, all rows of every sequence written (dq rows > 0 are zero under only_row0);
 *     mfma 1 / 0 = the MFMA / the VALU kernel; max_len <= 32. */
int ofx_attention_varlen(const void* qkv, void* out, const int* cu_seqlens, int nseq, int max_len, int n_head, int ld, int ldo, int k_off,
                         int v_off, int only_row0, float scale, float dropout_p, unsigned seed, int site, int op_dtype, ofx_stream stream);
int ofx_set_attention_op(const void* qkv, void* out, const int* cu_seqlens, int nseq, int n_head, int D, int ldo, int out_kind, int max_len,
                         int only_row0, float scale, float dropout_p, unsigned seed, int site, int op_dtype, ofx_stream stream);
int ofx_set_attention_bwd(const void* qkv, const float* d_o, void* dqkv, const int* cu_seqlens, int nseq, int n_head, int D, int max_len,
                          int only_row0, float scale, float dropout_p, unsigned seed, int site, int mfma, int op_dtype, ofx_stream stream);
/* Fused QKV projection + scaled-dot-product attention of a CLIP ViT layer (HF CLIPAttention's q/k/v_proj + softmax(q k^T * scale) v,
 * reached from clip_image_encoder.py:74-76), q | k | v staged in LDS only: X [nseq * seq_len, ldx] operand type, Wqkv [3 width, width]
 * (q | k | v rows), bias [3 width]; optional LayerNorm-fold consumer inputs row_stat [rows, 2] (mean, rstd) + col_sum [3 width];
 * out [nseq * seq_len, ldo] operand type (heads concatenated).  seq_len in [33, 64] except 35, 36 and 42 (a block's last image would read
 * key rows past the 16 zeroed pad rows behind its 256-row tile), width = n_head * 64, n_head >= 2, ldx and ldo >= width and multiples of 8
 * (else OFX_ESHAPE); NULL X, Wqkv, bias or out, nseq <= 0, or row_stat without col_sum: OFX_EINVAL; a refused call launches nothing.  No
 * mask.  Columns width .. ldo - 1 of out are not written; rows at or past nseq * seq_len of X and row_stat are not read (tile rows past the
 * end are clamped onto the last row).  X and out must not alias.  q | k | v are ONE rounding of the fp32 projection to the operand type and
 * the attention is attention_mfma_kernel's wave core: on operands whose fp32 sums are exact the output equals ofx_gemm* -> ofx_attention
 * value for value (tests/test_gpu_fused_qkv_exact.py). */
int ofx_fused_qkv_attention(const void* X, const void* Wqkv, const float* bias, const float* row_stat, const float* col_sum, void* out,
                            int nseq, int seq_len, int width, int n_head, int ldx, int ldo, float scale, int op_dtype, ofx_stream stream);
/* The same against split weights: Wqkv2 [3 width, 2 width], row n = [hi(width) | lo(width)] (ofx_convert mode 3): q | k | v = X . (hi + lo)^T,
 * two MFMA products per weight on one copy of the activations (the default tower scheme 'f16w2x'). */
int ofx_fused_qkv_attention_w2(const void* X, const void* Wqkv2, const float* bias, const float* row_stat, const float* col_sum, void* out,
                               int nseq, int seq_len, int width, int n_head, int ldx, int ldo, float scale, int op_dtype, ofx_stream stream);
/* The same with the correction product X . lo^T on the block-scaled fp8 matrix instruction, as ofx_gemm_w2f8 computes it: W8 [3 width, width]
 * bytes and scale8 [3 width] = ofx_pack_lo8 of Wqkv2; f16 operands only.  Every accumulator sees the instruction sequence of gemm_w2f8_kernel,
 * so q | k | v - and the output - equal ofx_gemm_w2f8(_fold) (256 x 256 kernel) -> ofx_attention bit for bit on ANY operands
 * (tests/test_gpu_fused_qkv_w2f8.py).  The blocks walk their tiles as the dual-weight GEMMs do: knob 11 sets the grid.  Refused as above, and:
 * width not a multiple of 128 (or weights of 2 GiB and more): OFX_ESHAPE; NULL W8 or scale8: OFX_EINVAL.  Rows at or
 * past nseq * seq_len of X are not read (they count as zeros).  Added within ABI version 6: nothing existing changed. */
int ofx_fused_qkv_attention_w2f8(const void* X, const void* Wqkv2, const void* W8, const void* scale8, const float* bias, const float* row_stat,
                                 const float* col_sum, void* out, int nseq, int seq_len, int width, int n_head, int ldx, int ldo, float scale,
                                 ofx_stream stream);
/* fp32-arithmetic attention over fixed-length sequences of <= 64 rows (the three-product CLIP text tower): qkv fp32 [nseq * seq_len, 3 D]
 * (q | k | v), HF's causal AND key-padding mask (key_mask [nseq, mask_ld] int64, 0 = ignored, may be NULL); out as ofx_set_attention.
 * A fully masked query row has probabilities 0: its output row is exactly 0, in all three copies of a split3 row (the library's own rule, as
 * under ofx_attention; HF's result for such a row depends on its version). */
int ofx_attention_f32(const float* qkv, void* out, const int64_t* key_mask, int nseq, int seq_len, int n_head, int D, int ldo, int out_kind,
                      int mask_ld, int causal, float scale, int op_dtype, ofx_stream stream);
/* fp32 [rows, cols] -> operand type; mode 0 plain, 1 [hi|lo|hi] (activation split), 2 [hi|hi|lo] (weight split) */
int ofx_convert(const float* src, void* dst, int rows, int cols, int mode, int op_dtype, ofx_stream stream);

#ifdef __cplusplus
}
#endif
#endif
