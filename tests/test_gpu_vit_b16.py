"""The ViT-B/16 image tower (patch 16 at 224: 197 tokens per image, the MFMA attention over 65 .. 256 rows) on a real MI355X, through the
drop-in encoders: CLIPImageEncoder(vision_config={"patch_size": 16}), 12 layers, synthetic weights on the B/16 shapes.

  - against the fp32 oracle O.vit_forward (pinned at patch 16 to transformers by tests/test_cpu_attention_long.py), unit-normalised,
    max|d| / max|ref|, for 2 and 9 images (394 and 1773 rows: below and across several GEMM tiles), at the tolerances
    test_gpu_model.test_folded_towers_vs_the_fp32_oracle holds the B/32 tower to: default scheme 1e-3, bf16 3e-2, f16 4e-3; f16x3 1e-3;
  - the pruned last layer (ofx_tune(8, 1): only_row0 attention, CLS queries only) against the full one within 2e-3, the bound of
    test_gpu_model.test_vit_last_layer_query_pruning_changes_nothing;
  - uint8 images through the fused preprocess route bit-equal to clip_preprocess + the pixel route;
  - a B/32 and a B/16 encoder interleaved in one process: the B/32 embeddings keep their bits;
  - the item encoder end to end: B/16 image half | text half through model(task=CP, encoder_input_dict=...) equals feeding the same
    embeddings precomputed, within the 1e-3 test_gpu_model.test_item_encoder_cp_with_encoder_and_precompute holds both routes to.

MEASURED (MI355X), 2 | 9 images against the fp32 oracle: f16w2x (default) 2.75e-4 | 3.65e-4, bf16 4.34e-3 | 4.35e-3, f16 5.89e-4 | 5.92e-4,
f16x3 6.77e-5 | 8.51e-5 - every scheme inside its bound, none marked; pruned against full last layer: bit-equal at both sizes; item
encoder: image half 3.29e-4 from the oracle, tower-fed and precomputed CP logits bit-equal.  The file runs in 15 s.
"""
import warnings

import numpy as np
import pytest
import torch

from conftest import W_SEED, rel_err
from oracle import np_oracle as O
from outfitx_amd import synth
from outfitx_amd._lib import DEFAULT_TOWER_PRECISION as DEFAULT_TOWERS

pytestmark = pytest.mark.gpu
warnings.simplefilter("ignore")

N_IMG = (2, 9)
PX_SEED = 79


def unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def vision_encoder(patch):
    from outfitx_amd.encoders import CLIPImageEncoder
    enc = CLIPImageEncoder(vision_config={"patch_size": patch})
    enc.load_state_dict({"model." + k: torch.from_numpy(v) for k, v in synth.vision_weights(W_SEED, patch=patch).items()}, strict=True)
    return enc.cuda().eval()


@pytest.fixture(scope="module")
def b16():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    enc = vision_encoder(16)
    assert enc.model.config.patch_size == 16 and enc._desc().vit_patch == 16 and enc.image_size == (224, 224)
    return enc


@pytest.fixture(scope="module")
def pixels():
    return synth.pixel_values(PX_SEED, max(N_IMG))


@pytest.fixture(scope="module")
def oracle(pixels):
    """The fp32 oracle on the 9 images, computed once; the 2-image runs are judged against its first two rows."""
    return unit(O.vit_forward(pixels, synth.vision_weights(W_SEED, patch=16)))


def run(enc, px):
    with torch.no_grad():
        return enc(torch.from_numpy(px).view(px.shape[0], 1, 3, 224, 224).cuda()).view(px.shape[0], -1).cpu().numpy()


@pytest.mark.parametrize("prec,tol", [(DEFAULT_TOWERS, 1e-3), ("bf16", 3e-2), ("f16", 4e-3), ("f16x3", 1e-3)])
def test_b16_tower_vs_the_fp32_oracle(b16, pixels, oracle, prec, tol):
    b16.tower_precision = prec
    try:
        got = {n: run(b16, pixels[:n]) for n in N_IMG}
    finally:
        b16.tower_precision = DEFAULT_TOWERS
    errs = {}
    for n, a in got.items():
        assert a.shape == (n, 512) and np.isfinite(a).all()
        assert np.abs(np.linalg.norm(a, axis=-1) - 1).max() < 1e-5
        errs[n] = rel_err(a, oracle[:n])
        print(f"PARITY vit-b16 {prec} n={n}: {errs[n]:.2e} (bound {tol:g})")
    assert all(e < tol for e in errs.values()), (prec, errs)


def test_b16_last_layer_query_pruning_changes_nothing(b16, pixels):
    from outfitx_amd import _lib as L
    lib = L.load()
    for n in N_IMG:
        outs = []
        for prune in (1, 0):
            lib.ofx_tune(8, prune)
            try:
                outs.append(run(b16, pixels[:n]))
            finally:
                lib.ofx_tune(8, 1)
        e = rel_err(outs[0], outs[1])
        print(f"PARITY vit-b16 pruned vs full last layer n={n}: {e:.2e} (bound 2e-3)")
        assert np.isfinite(outs[0]).all() and e < 2e-3, (n, e)


def test_b16_uint8_images_through_the_fused_preprocess_route(b16):
    from PIL import Image
    from outfitx_amd.encoders import clip_preprocess
    g = np.random.default_rng(16)
    shapes = [(300, 300, 3), (280, 350, 3), (90, 130), (37, 53, 3), (224, 224, 3), (640, 480, 3)]
    ims = [[Image.fromarray(g.integers(0, 256, s, dtype=np.uint8))] for s in shapes]
    assert b16.fused_preprocess
    with torch.no_grad():
        a = b16(ims)
        b = b16(clip_preprocess([r[0] for r in ims], 224).view(len(ims), 1, 3, 224, 224).cuda())
        b16.fused_preprocess = False
        try:
            c = b16(ims)
        finally:
            b16.fused_preprocess = True
    assert torch.isfinite(b).all() and torch.equal(a, b) and torch.equal(c, b)


def test_b32_and_b16_encoders_interleave(b16, pixels):
    b32 = vision_encoder(32)
    alone = [run(b32, pixels[:n]) for n in N_IMG]
    mixed = []
    for n in N_IMG:
        first = run(b16, pixels[:n])
        mixed.append(run(b32, pixels[:n]))
        assert np.array_equal(run(b16, pixels[:n]), first)
    assert all(np.array_equal(a, m) for a, m in zip(alone, mixed))
    want = unit(O.vit_forward(pixels[:2], synth.vision_weights(W_SEED)))
    assert rel_err(alone[0], want) < 1e-3


def test_item_encoder_end_to_end_with_a_b16_image_tower():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    cfg = ItemEncoderConfig(type="clip")
    cfg.clip_vision_config = {"patch_size": 16}
    m = OutfitX(OutfitXConfig(item_encoder=cfg))
    assert m.item_encoder.image_enc.model.config.patch_size == 16 and m.item_encoder.image_size == (224, 224)
    sd = synth.outfit_transformer_weights(W_SEED)
    sd.update(synth.vision_weights(W_SEED, synth.IMG_PREFIX, patch=16))
    sd.update(synth.text_weights(W_SEED, synth.TXT_PREFIX))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    B, L = 2, 3
    px = torch.from_numpy(synth.pixel_values(81, B * L).reshape(B, L, 3, 224, 224)).cuda()
    ids, att = synth.token_batch(81, B * L, 64, np.array([4, 8, 6, 3, 9, 12]))
    texts = {"input_ids": torch.from_numpy(ids).view(B, L, 64), "attention_mask": torch.from_numpy(att).view(B, L, 64)}
    mask = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        items = m.item_encoder(px, texts)
        fed = m(task=CP, outfit_embedding=None, outfit_mask=mask, encoder_input_dict={"images": px, "texts": texts}).cpu().numpy()
        pre = m(task=CP, outfit_embedding=items, outfit_mask=mask).cpu().numpy()
    assert items.shape == (B, L, 1024) and np.isfinite(fed).all() and fed.shape == (B, 1)
    halves = items.view(B, L, 2, 512).norm(dim=-1).cpu().numpy()
    assert np.abs(halves - 1).max() < 1e-5
    img = unit(O.vit_forward(px.view(B * L, 3, 224, 224).cpu().numpy(), synth.vision_weights(W_SEED, patch=16)))
    e_img = rel_err(items.view(B * L, 1024)[:, :512].cpu().numpy(), img)
    e = rel_err(fed, pre)
    print(f"PARITY vit-b16 item encoder: image half vs oracle {e_img:.2e}; CP logits tower-fed vs precomputed {e:.2e}")
    assert e_img < 1e-3 and e < 1e-3
