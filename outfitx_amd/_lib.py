"""ctypes binding of libofx_hip.so (the C ABI declared in include/ofx.h).

The product path has NO fallback: if the shared library is missing or a call fails, an exception is
raised.  The library is built in-tree by `make` / `__graft_entry__.build()`.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OFX_LIB: an alternative build of the SAME library (tools only, e.g. `make EXTRA=... LIB=outfitx_amd/libofx_hip_alt.so OBJ=build/obj_alt`)
LIB_PATH = os.environ.get("OFX_LIB") or os.path.join(_HERE, "libofx_hip.so")

OFX_OK = 0
ABI_VERSION = 6          # include/ofx.h OFX_ABI_VERSION
F32, BF16, F16 = 0, 1, 2
ACT_NONE, ACT_QUICK_GELU, ACT_GELU, ACT_MISH = 0, 1, 2, 3
PREC_BF16, PREC_F16, PREC_BF16X3 = 0, 1, 2
OUT_F32, OUT_OP, OUT_SPLIT3 = 0, 1, 2
OP_SET_ENCODER, OP_VIT, OP_TEXT, OP_TOPK = 0, 1, 2, 3
PREC_F16W2 = 3          # outfit transformer only: f16 activations x split (hi, lo) f16 weights, two products per weight (include/ofx.h)
PRECISIONS = {"bf16": PREC_BF16, "f16": PREC_F16, "fp16": PREC_F16, "bf16x3": PREC_BF16X3, "f16w2": PREC_F16W2}
# CLIP tower operand schemes: name -> (operand type, vit_w2_mask, txt_x3, proj_x3, vit_x3); `tower_scheme` below adds the
# per-layer rungs.  Parity figures: max|d| / max|ref| over all 256 CP logits of bench.py's batch against the reference's own fp32 CPU output, 100
# weight seeds (profiles/r04_seed_sweep_bench_scale.json, profiles/r04_rung_screen_100_seeds.json) - a DISTRIBUTION over weight draws, not a constant:
#   "bf16" / "f16": one MFMA product per term everywhere (fastest; 7e-3 / 0.7-2.8e-3 end to end: outside the north star's 1e-3).
#   "f16w2x" (DEFAULT): every ViT GEMM (patch embedding, qkv, out-proj, fc1, fc2) against split (hi, lo) weights, the correction product on the fp8
#     matrix instruction at the bench's batch size (gemm_w2f8.hip; e5m2 activation image since round 4); text tower, projection tails and the outfit
#     transformer in three products.  100 of 100 seeds inside 1e-3: median 2.5e-4, p90 4.5e-4, worst 6.3e-4; lognormal fit: P(>= 1e-3) 0.12 % per draw.
#     Also inside 1e-3 on every draw of the 8-outfit tests, whose worst (seed 99: all eight reference logits below 0.27) reads 8.9e-4.
#   "f16w2h" = "f16w2x@qkv=0-5" (the cheapest rung the round-4 screens found inside 8e-4 at the bench's batch size): only the first six ViT layers keep
#     the qkv correction (layers 6-11 run the fused single-product QKV + attention kernel): 3.2 % faster (8,092 vs 7,837 outfits/s on one box); 100 of
#     100 inside 1e-3 at 256 outfits: median 3.0e-4, p90 5.4e-4, worst 7.35e-4; P(>= 1e-3) 0.24 % per draw - but 1.53e-3 on the 8-outfit seed-99 draw
#     (same absolute error, 4e-4, over a batch whose largest logit is 0.27), which is why it is not the default.
#     Rungs below it that were swept and rejected (worst seed >= 8e-4 at 256 outfits): qkv on layers 0-3 (8.05e-4), fc1 on fewer layers (9.6e-4 /
#     7.7e-4), fc2 or out-proj corrections on half the layers (9.2e-4 ... 1.06e-3), the text tower in split-weight form (1.65e-3).
#   "f16w2": split weights on patch / out-proj / fc2 only (qkv through the fused kernel): 9 % faster than f16w2x, worst seeds at 1.0e-3.
W2_PATCH, W2_QKV, W2_OUT, W2_FC1, W2_FC2 = 1, 2, 4, 8, 16
TOWER_SCHEMES = {
    "bf16": (PREC_BF16, 0, 0, 0, 0), "f16": (PREC_F16, 0, 0, 0, 0), "fp16": (PREC_F16, 0, 0, 0, 0),
    "f16w2": (PREC_F16, W2_PATCH | W2_OUT | W2_FC2, 1, 1, 0),
    "bf16w2": (PREC_BF16, W2_PATCH | W2_OUT | W2_FC2, 1, 1, 0),
    # rungs between the two (studies: tests/studies/bench_scale_sweep.py): + qkv, or + fc1
    "f16w2q": (PREC_F16, W2_PATCH | W2_QKV | W2_OUT | W2_FC2, 1, 1, 0),
    "f16w2f": (PREC_F16, W2_PATCH | W2_OUT | W2_FC1 | W2_FC2, 1, 1, 0),
    # every ViT weight split (qkv then runs as dual-weight GEMM + attention kernel instead of the fused kernel)
    "f16w2x": (PREC_F16, W2_PATCH | W2_QKV | W2_OUT | W2_FC1 | W2_FC2, 1, 1, 0),
    # every tower GEMM in three products (the patch embedding against split weights; the ViT's MFMA attention core stays on f16
    # q, k, v, P): 1.3-1.8e-4 end to end on the default scheme's worst seeds, 1.9x the time (60.5 vs 32 ms per cfg2 step)
    "f16x3": (PREC_F16, W2_PATCH, 1, 1, 1), "bf16x3": (PREC_BF16, W2_PATCH, 1, 1, 1),
}
SCHEME_ALIASES = {"f16w2h": "f16w2x@qkv=0-5"}
DEFAULT_TOWER_PRECISION = "f16w2x"


def _layer_bits(spec: str) -> int:
    """'0-5,8' -> bit mask of ViT layers."""
    m = 0
    for part in spec.split(","):
        a, _, b = part.partition("-")
        for l in range(int(a), int(b or a) + 1):
            m |= 1 << l
    return m


def tower_scheme(name: str) -> dict:
    """A tower_precision string -> the ofx_model_desc fields it sets.  A key of TOWER_SCHEMES, optionally followed by '@' and ';'-separated
    options (the finer rungs of round 4, tests/studies/bench_scale_sweep.py):
      txt=w2            the text tower in the ViT's scheme (f16 activations x split weights on qkv / out / fc1 / fc2) instead of three products;
      qkv=0-5  fc1=0-3,8  out=none  fc2=6-11   ViT layers whose qkv / fc1 / out-proj / fc2 GEMM keeps its split weights (the others run the
                        single-product copy).
    Raises ValueError on anything else."""
    name = SCHEME_ALIASES.get(name, name)
    base, _, opts = name.partition("@")
    if base not in TOWER_SCHEMES:
        raise ValueError(f"unknown tower_precision {name!r}; one of {sorted(list(TOWER_SCHEMES) + list(SCHEME_ALIASES))} [+ '@txt=w2;qkv=<layers>;fc1=<layers>']")
    prec, mask, txt_x3, proj_x3, vit_x3 = TOWER_SCHEMES[base]
    d = {"tower_precision": prec, "vit_w2_mask": mask, "txt_x3": txt_x3, "proj_x3": proj_x3, "vit_x3": vit_x3,
         "txt_w2_mask": 0, "vit_w2_qkv_layers": 0, "vit_w2_fc1_layers": 0, "vit_w2_out_layers": 0, "vit_w2_fc2_layers": 0}
    for o in filter(None, opts.split(";")):
        k, _, v = o.partition("=")
        try:
            if k == "txt" and v == "w2":
                d["txt_x3"], d["txt_w2_mask"] = 0, W2_QKV | W2_OUT | W2_FC1 | W2_FC2
            elif k in ("qkv", "fc1", "out", "fc2"):
                bits = _layer_bits(v) if v not in ("", "none") else 0
                if bits == 0:
                    d["vit_w2_mask"] &= ~{"qkv": W2_QKV, "fc1": W2_FC1, "out": W2_OUT, "fc2": W2_FC2}[k]
                d[f"vit_w2_{k}_layers"] = bits
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"tower_precision {name!r}: bad option {o!r} (txt=w2 | qkv= / fc1= / out= / fc2=<layers>, layers like 0-5,8 or none)") from None
    return d
ACTS = {"none": ACT_NONE, "quick_gelu": ACT_QUICK_GELU, "gelu": ACT_GELU, "mish": ACT_MISH}


class OfxError(RuntimeError):
    pass


class ModelDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "d_model", "n_head", "d_ffn", "n_layers", "max_items", "outfit_act", "outfit_precision",
        "vit_width", "vit_layers", "vit_heads", "vit_mlp", "vit_patch", "vit_image", "vit_act",
        "txt_width", "txt_layers", "txt_heads", "txt_mlp", "txt_vocab", "txt_max_pos", "txt_act", "txt_eos_id",
        "proj_dim", "tower_precision")] + [("ln_eps", C.c_float)] + [(n, C.c_int) for n in ("vit_w2_mask", "txt_x3", "proj_x3", "vit_x3", "txt_w2_mask", "vit_w2_qkv_layers", "vit_w2_fc1_layers", "vit_w2_out_layers", "vit_w2_fc2_layers")]


class OptSegment(C.Structure):          # ofx_opt_segment: 24 bytes, three 8-byte words
    _fields_ = [("param", C.c_void_p), ("offset", C.c_longlong), ("numel", C.c_longlong)]


class ProfRecord(C.Structure):
    _fields_ = [("cat", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("kind", C.c_int), ("kmul", C.c_int), ("ms", C.c_float), ("flops", C.c_double), ("bytes", C.c_double)]


_vp, _i, _f, _sz, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64

# name -> (restype, argtypes); every symbol include/ofx.h declares
SIGNATURES = {
    "ofx_last_error": (C.c_char_p, []),
    "ofx_abi_version": (_i, []),
    "ofx_stream_create_low_priority": (_i, [_i, C.POINTER(_vp)]),
    "ofx_stream_destroy": (_i, [_vp]),
    "ofx_default_desc": (None, [C.POINTER(ModelDesc)]),
    "ofx_create": (_vp, [_i, C.POINTER(ModelDesc)]),
    "ofx_destroy": (None, [_vp]),
    "ofx_pack_outfit_weights": (_i, [_vp, C.POINTER(_vp), _i, _vp]),
    "ofx_pack_vision_weights": (_i, [_vp, C.POINTER(_vp), _i, _vp]),
    "ofx_pack_text_weights": (_i, [_vp, C.POINTER(_vp), _i, _vp]),
    "ofx_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "ofx_set_encoder_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ofx_cp_head": (_i, [_vp, _vp, _i, _vp, _vp]),
    "ofx_cir_head": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "ofx_cir_prefix": (_i, [_vp, _vp, _i, _vp, _vp]),
    "ofx_vit_b32_fwd": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "ofx_clip_text_fwd": (_i, [_vp, _vp, _vp, C.POINTER(_i), _i, _i, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "ofx_clip_text_fwd_shared": (_i, [_vp, _vp, _vp, C.POINTER(_i), _i, _i, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "ofx_fitb_argmin": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ofx_fitb_argmin_indexed": (_i, [_vp, _i, C.c_longlong, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "ofx_l2_topk": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i64, _vp, _vp, _vp, _sz, _vp]),
    "ofx_l2_topk_grouped_ws": (_sz, [_i, _i, _i]),
    "ofx_l2_topk_grouped": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ofx_topk_merge": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ofx_clip_preprocess_ws": (_sz, [_vp, _vp, _i, _i, _i]),
    "ofx_clip_preprocess": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ofx_clip_preprocess_patches": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _sz, _vp]),
    "ofx_patchify": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ofx_vit_b32_u8_ws_bytes": (_sz, [_vp, _vp, _vp, _i, _i]),
    "ofx_vit_b32_fwd_u8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp]),
    "ofx_set_encoder_fwd_indexed": (_i, [_vp, _vp, _i, C.c_longlong, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ofx_cp_train_fwd_indexed": (_i, [_vp, _vp, _i, C.c_longlong, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _f, C.c_uint, _vp]),
    "ofx_cp_train_tape_bytes": (_sz, [_vp, _i, _i]),
    "ofx_cp_train_ws_bytes": (_sz, [_vp, _i, _i]),
    "ofx_cp_train_grad_floats": (_sz, [_vp, C.POINTER(_sz), _i]),
    "ofx_cp_train_fwd": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _f, C.c_uint, _vp]),
    "ofx_cp_train_bwd": (_i, [_vp, _vp, _sz, _vp, _i, _i, _vp, _sz, _vp, _sz, _f, C.c_uint, _vp]),
    "ofx_cir_train_fwd": (_i, [_vp, _vp, _vp, _vp, _i, C.c_longlong, _vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp, _sz, _f, C.c_uint, _vp]),
    "ofx_cir_train_bwd": (_i, [_vp, _vp, _sz, _vp, _i, _i, _vp, _sz, _vp, _sz, _f, C.c_uint, _vp]),
    "ofx_cp_train_bwd_into": (_i, [_vp, _vp, _sz, _vp, _i, _i, C.POINTER(_vp), _i, _i, _vp, _sz, _f, C.c_uint, _vp]),
    "ofx_cir_train_bwd_into": (_i, [_vp, _vp, _sz, _vp, _i, _i, C.POINTER(_vp), _i, _i, _vp, _sz, _f, C.c_uint, _vp]),
    "ofx_train_arm_layer_events": (_i, [_vp, C.POINTER(_vp), _i]),
    "ofx_dropout_mask": (_i, [_f, C.c_uint, _i, _i, _i, _vp, _vp]),
    "ofx_focal_loss": (_i, [_vp, _vp, _i, _f, _f, _f, _vp, _vp, _vp]),
    "ofx_focal_loss_ex": (_i, [_vp, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "ofx_set_rank_loss_ws_bytes": (_sz, [_i, _i, _i]),
    "ofx_set_rank_loss": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ofx_set_rank_loss_indexed": (_i, [_vp, _i, C.c_longlong, _vp, _vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ofx_cir_sample_batch": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, C.c_uint, C.c_uint, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "ofx_adamw_step_ws_bytes": (_sz, [C.c_longlong]),
    "ofx_adamw_step": (_i, [_vp, _i, _vp, _vp, _vp, C.c_longlong, _vp] + [C.c_double] * 7 + [_vp, _vp, _vp, _sz, _vp]),
    "ofx_adamw_step_scaled": (_i, [_vp, _i, _vp, _vp, _vp, C.c_longlong, _vp] + [C.c_double] * 7 + [_vp, _vp, C.c_double, C.c_double, _i] + [_vp, _vp, _vp, _sz, _vp]),
    "ofx_profile_enable": (None, [_i]),
    "ofx_profile_read": (_i, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
    "ofx_profile_records": (_i, [C.POINTER(ProfRecord), _i]),
    "ofx_tune": (_i, [_i, _i]),
    "ofx_config_generation": (C.c_uint, []),
    "ofx_profile_enabled": (_i, []),
    "ofx_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "ofx_gemm_w2": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "ofx_gemm_x3": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "ofx_pack_lo8": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "ofx_gemm_w2f8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "ofx_gemm_w2f8_fold": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "ofx_gemm_tn_ws": (_sz, [_i, _i, _i]),
    "ofx_gemm_tn": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _i, _vp]),
    "ofx_gemm_splitk_ws": (_sz, [_i, _i, _i]),
    "ofx_gemm_splitk": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "ofx_gemm_train": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _f, C.c_uint, _i, _i, _vp, _sz, _vp]),
    "ofx_gemm_tn_into": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _sz, _i, _vp]),
    "ofx_transpose_cast": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp]),
    "ofx_layernorm_bwd_ws": (_sz, [_i]),
    "ofx_layernorm_bwd": (_i, [_vp] * 11 + [_i, _vp, _i, _f, C.c_uint, _i, _i, _i, _vp, _sz, _vp]),
    "ofx_colsum_ws": (_sz, [_i]),
    "ofx_colsum": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _sz, _vp]),
    "ofx_head_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, C.c_uint, _i, _i, _i, _i, _vp]),
    "ofx_gemm_fold_producer": (_i, [_vp] * 9 + [_i] * 8 + [_vp]),
    "ofx_gemm_fold": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "ofx_stats_finalize": (_i, [_vp, _i, _i, _f, _vp, _i, _vp]),
    "ofx_row_stats_cast": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp]),
    "ofx_fold_pack": (_i, [_vp] * 7 + [_i, _i, _i, _i, _vp]),
    "ofx_vit_embed_ln": (_i, [_vp] * 9 + [_i, _i, _i, _f, _i, _vp]),
    "ofx_gather_hilo": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "ofx_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "ofx_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "ofx_attention_ex": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "ofx_set_attention_slabs": (_i, [_vp, _sz, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "ofx_splitk_reduce_ln": (_i, [_vp, _sz, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _i, _i, _vp]),
    "ofx_fused_qkv_attention": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "ofx_fused_qkv_attention_w2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "ofx_fused_qkv_attention_w2f8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "ofx_set_attention": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "ofx_attention_varlen": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, C.c_uint, _i, _i, _vp]),
    "ofx_set_attention_op": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, C.c_uint, _i, _i, _vp]),
    "ofx_set_attention_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _f, C.c_uint, _i, _i, _i, _vp]),
    "ofx_attention_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "ofx_convert": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
}

_lib = None


def load() -> C.CDLL:
    """Load the library once; raise (never fall back) when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OfxError(f"{LIB_PATH} not found: build it with `make` (or __graft_entry__.build()); "
                       "outfitx_amd has no CPU/PyTorch fallback for the scoring path")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError if the .so does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.ofx_abi_version() != ABI_VERSION:
        raise OfxError("libofx_hip.so ABI version mismatch; rebuild")
    for kv in filter(None, os.environ.get("OFX_TUNE", "").split(",")):       # experiments / A-B runs only: OFX_TUNE=18:0,17:0 -> ofx_tune(18, 0), ofx_tune(17, 0) at load
        knob, _, val = kv.partition(":")
        if lib.ofx_tune(int(knob), int(val)) != OFX_OK:
            raise OfxError(f"OFX_TUNE: ofx_tune({knob}, {val}) was refused")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != OFX_OK:
        msg = load().ofx_last_error()
        raise OfxError(f"{what or 'ofx call'} failed (code {rc}): {msg.decode() if msg else ''}")


def default_desc() -> ModelDesc:
    d = ModelDesc()
    load().ofx_default_desc(C.byref(d))
    return d
