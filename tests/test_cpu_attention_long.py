"""CPU side of the attention over 65 .. 256 rows and of the ViT-B/16 image tower built on it (tests/attn_long_cases.py has the cases):

  1  the inputs of tests/test_gpu_attention_long.py are pinned by checksum;
  2  they are sharp: a multi-tile kernel that drops its last key tile, exchanges two key tiles' V rows or sums over the first 64 keys only
     lands, at EVERY length and in both operand types, outside the GPU test's criterion e <= 1.6 max(e_emul, 1e-2 u) on some block;
     the fourth mutant - the row MAX over the first 64 keys only - is shown to be invisible (softmax is shift invariant): no output
     test can see it on finite scores, and a pass of the GPU test says nothing about it;
  3  oracle/np_oracle.vit_forward, the GPU tower tests' reference, is pinned at patch 16 (197 tokens) against
     transformers.CLIPVisionModelWithProjection on seeded weights, at the tolerance tests/test_oracle_golden.py holds it to at patch 32;
  4  CLIPImageEncoder takes its architecture from a checkpoint's config or from vision_config=, loads it strictly, and raises
     NotImplementedError for what the kernels do not take instead of running a random ViT-B/32.

MEASURED (float64): worst block ratio per mutant over the nine lengths, bf16 | f16 - the smallest is what the criterion has to catch:
  drop_last_tile  min over S 48 | 384 (S = 241: one live key in the dropped tile), up to 279 | 2220
  swap_v_tiles    min 216 | 1710, up to 520 | 4330
  sum_first_64    min 19.5 | 150 (S = 65)
  max_first_64    1.0000 at every S, both types: not a fault an output can show
"""
import numpy as np
import pytest
import torch

import attn_long_cases as C
from conftest import rel_err
from oracle import attn_fwd as A
from oracle import np_oracle as O
from outfitx_amd import synth

QKV_CRC = {65: '6ae3be7a', 80: 'a619f6b9', 81: '63fc01b0', 128: '7ae649c1', 129: '6804cca5', 196: '3a666659', 197: '143f80b5', 241: '8e82c19a',
           256: 'd4552701'}
MASK_CRC = {'tail65': '5f1e7436', 'holes65': '2e5a0810', 'causal_holes65': '2e5a0810', 'key065': '6b4a0348', 'allzero65': 'e123ef8b',
            'tail129': 'd5d6515d', 'holes129': 'fc12ed98', 'causal_holes129': 'fc12ed98', 'key0129': '8ee7077f', 'allzero129': '57b1628c',
            'tail197': 'b9ddf1f1', 'holes197': '0f8f5e16', 'causal_holes197': '0f8f5e16', 'key0197': '7a908877', 'allzero197': '54ecd2fe',
            'tail256': '862e31e3', 'holes256': '94ee16d0', 'causal_holes256': '94ee16d0', 'key0256': '7a418479', 'allzero256': '3a588c1b'}


def test_inputs_are_pinned():
    got = {S: synth.checksum(C.qkv(S)) for S in C.LENGTHS}
    masks = {}
    for S in C.MASKED_S:
        for f in ("tail", "holes", "causal_holes"):
            m, causal = C.key_mask(f, S)
            assert m.shape == (C.NSEQ, C.MASK_LD) and m[:, S:].all() and m[:, 0].all() and causal == (f == "causal_holes")
            masks[f"{f}{S}"] = synth.checksum(m)
        for name, m, causal in C.masked_row_cases(S):
            dead = np.broadcast_to(A.dead_of(m, causal, S), (C.NSEQ, C.H, S, S))
            assert dead.all(-1).any() and not dead.all(-1).all(), "some fully masked query rows, not only such rows"
            masks[f"{name}{S}"] = synth.checksum(m)
    print("QKV_CRC =", got)
    print("MASK_CRC =", masks)
    assert got == QKV_CRC and masks == MASK_CRC
    assert len(C.CASES) == 9 + 4 * 4 and {S for S, f in C.CASES if f != "none"} == set(C.MASKED_S)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("S", C.LENGTHS)
def test_cases_are_sharp_against_multi_tile_faults(S, dt):
    q, k, v = C.heads64(S, dt)
    ref = A.attn_fwd_ref(q, k, v, None, C.SCALE)
    emul = A.attn_fwd_emul(q, k, v, None, C.SCALE, dt)
    assert np.array_equal(C.emul_mutant(q, k, v, None, C.SCALE, dt, None), emul), "the mutants' base is the oracle's emulation"
    assert C.worst_ratio(emul, ref, emul, dt) <= 1.0
    for mutant in ("drop_last_tile", "swap_v_tiles", "sum_first_64"):
        r = C.worst_ratio(C.emul_mutant(q, k, v, None, C.SCALE, dt, mutant), ref, emul, dt)
        print(f"MUTANT {mutant} {dt} S={S} worst block ratio {r:.3g}")
        assert r > C.F_OP, (mutant, S, dt, r)
    # the max over a part of the row: the same P up to the last bits of float64, so the same rounded output almost everywhere
    r = C.worst_ratio(C.emul_mutant(q, k, v, None, C.SCALE, dt, "max_first_64"), ref, emul, dt)
    print(f"MUTANT max_first_64 {dt} S={S} worst block ratio {r:.4f}")
    assert r <= 1.001, "shift invariance: this fault cannot be seen in the output"


def test_oracle_vit_forward_at_patch_16_against_transformers():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from test_oracle_golden import TOL
    Wv = synth.vision_weights(41, n_layers=2, patch=16)
    assert Wv["vision_model.embeddings.position_embedding.weight"].shape == (197, 768)
    cfg = CLIPVisionConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=2, num_attention_heads=12, patch_size=16, image_size=224,
                           projection_dim=512, hidden_act="quick_gelu")
    hf = CLIPVisionModelWithProjection(cfg).eval()
    sd = {k: torch.from_numpy(v) for k, v in Wv.items()}
    extra = {k: v for k, v in hf.state_dict().items() if k not in sd}          # buffers only (position_ids)
    assert all("position_ids" in k for k in extra)
    hf.load_state_dict({**sd, **extra}, strict=True)
    px = synth.pixel_values(43, 3)
    with torch.no_grad():
        want = hf(pixel_values=torch.from_numpy(px)).image_embeds.numpy()
    got = O.vit_forward(px, Wv, n_layers=2)
    e = rel_err(got, want)
    print(f"np_oracle.vit_forward at patch 16 (197 tokens, 2 layers) vs transformers: {e:.2e}")
    assert got.shape == (3, 512) and e < TOL


TINY = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, patch_size=16, image_size=64, projection_dim=128)


def save_tiny(path, **over):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(3)
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(**{**TINY, **over}, hidden_act="quick_gelu"))
    hf.save_pretrained(str(path))
    return hf


def test_architecture_comes_from_the_checkpoint_and_unsupported_ones_raise(tmp_path):
    from outfitx_amd import encoders as E
    hf = save_tiny(tmp_path / "tiny")
    params = E.load_vision_checkpoint(str(tmp_path / "tiny"))                  # its own shapes, loaded strictly
    assert {k: getattr(params.config, k) for k in TINY} == TINY
    want = {k: v for k, v in hf.state_dict().items() if "position_ids" not in k}
    got = params.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert got["vision_model.embeddings.position_embedding.weight"].shape == (17, 256)
    assert got["vision_model.embeddings.patch_embedding.weight"].shape == (256, 3, 16, 16)
    assert len(params.pack_list()) == 5 + 16 + 3
    assert E.load_vision_checkpoint(str(tmp_path / "nowhere")) is None
    # the encoder judges the architecture before it builds anything: width 256 is none of the tower GEMMs' widths - no random B/32 instead
    with pytest.raises(NotImplementedError, match="widths"):
        E.CLIPImageEncoder(str(tmp_path / "tiny"))
    save_tiny(tmp_path / "heads32", num_attention_heads=8)
    with pytest.raises(NotImplementedError, match="heads of 64"):
        E.CLIPImageEncoder(str(tmp_path / "heads32"))
    for bad, what in (({"num_attention_heads": 24}, "heads of 64"), ({"patch_size": 14, "image_size": 224}, "257 tokens"),
                      ({"patch_size": 16, "image_size": 232}, "multiple of the patch"), ({"hidden_size": 1280, "num_attention_heads": 20}, "widths")):
        with pytest.raises(NotImplementedError, match=what):
            E.CLIPImageEncoder(vision_config=bad)
    with pytest.raises(NotImplementedError, match="dim_per_modality"):
        E.CLIPImageEncoder(vision_config={"projection_dim": 768}, dim_per_modality=512)
    with pytest.raises(ValueError, match="unknown fields"):
        E.CLIPImageEncoder(vision_config={"patch": 16})


def test_vision_config_builds_a_b16_tower_and_a_missing_checkpoint_still_warns(tmp_path):
    from outfitx_amd import encoders as E
    from outfitx_amd.configs import ItemEncoderConfig
    enc = E.CLIPImageEncoder(vision_config={"patch_size": 16, "num_hidden_layers": 1})
    c = enc.model.config
    assert (c.patch_size, c.image_size, c.hidden_size, c.num_attention_heads, c.projection_dim) == (16, 224, 768, 12, 512)
    assert enc.model.vision_model.embeddings.position_embedding.weight.shape == (197, 768)
    assert enc.image_size == (224, 224) and enc.processor.size == {"shortest_edge": 224} and not enc.pretrained
    d = enc._desc()
    assert (d.vit_patch, d.vit_image, d.vit_width, d.vit_heads, d.vit_layers, d.proj_dim) == (16, 224, 768, 12, 1, 512)
    enc.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in synth.vision_weights(5, n_layers=1, patch=16).items()}, strict=True)
    with pytest.warns(UserWarning, match="not available offline"):             # unchanged: no checkpoint -> random ViT-B/32 and a warning
        plain = E.CLIPImageEncoder(str(tmp_path / "no-such-checkpoint"))
    assert plain.model.config.patch_size == 32 and not plain.pretrained
    cfg = ItemEncoderConfig(type="clip")
    cfg.clip_vision_config = {"projection_dim": 768}                            # passed through, and judged against dim_per_modality = 512
    with pytest.raises(NotImplementedError, match="dim_per_modality 512"):
        E.ItemEncoder(cfg)
