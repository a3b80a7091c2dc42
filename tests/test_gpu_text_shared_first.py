"""The text tower's shared first-position row (ofx_clip_text_fwd_shared, ofx_tune(21, v)).

Every CLIP text starts with the same BOS token and the text tower is causal, so position 0 of a text attends to itself only: its row
carries the same bits for every text in every layer.  The three-product text path computes it once - rows 1 + N (Tc - 1) instead of
N Tc - when the host can vouch for the precondition (engine.shared_first_row).  Checked here, at the model's text-tower dimensions:

  1. mode on == knob off, bit for bit, with the GEMMs' summation order made independent of M (always gemm_x3_kernel; or the 128 x 128
     kernel with split-K off) - N in {1, 2, 37, 300}, ragged lengths with Tc in {2, 3, 8, 9, 33, 64} (one text's EOS at position 1, one
     at Tc - 1), masks zero after EOS, normalize on and off;
  2. default knobs, both modes, against the numpy oracle at the bound of test_gpu_model.test_text_tower_vs_reference_golden's default
     scheme, 1e-3 (max |d| / max |ref|).  At N = 300 the oracle runs on 24 of the texts (the first, with its EOS at Tc - 1, the last,
     with its EOS at position 1, and 22 spread between: a text's embedding does not depend on its neighbours), everything else on all;
  3. the four fallbacks run the full rows (M of the tower's QKV GEMM read from the profile records) and equal the knob-off result;
  4. a captured CP call whose pinned ids stop sharing their first token is not replayed from the shared-row graph;
  5. the host predicate alone (no GPU).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import W_SEED, rel_err
from oracle import np_oracle as O
from outfitx_amd import synth
from outfitx_amd.engine import TextLengths, shared_first_row

T = 64
NS = (1, 2, 37, 300)
TCS = (2, 3, 8, 9, 33, 64)
KNOB_DEFAULTS = {2: 0, 5: 1, 15: 1, 21: 1}


# ------------------------------------------------------------------------------------------ 5. the host predicate (no GPU)
def test_host_predicate():
    ids, att = (torch.from_numpy(a) for a in synth.token_batch(3, 5, T, [2, 8, 3, 8, 5]))
    assert shared_first_row(ids, att) and shared_first_row(ids, None)
    assert shared_first_row(ids[:1], att[:1])                                      # one text shares with itself
    other = ids.clone(); other[3, 0] = synth.BOS_ID - 1
    assert not shared_first_row(other, att)                                        # differing first ids
    masked = att.clone(); masked[2, 0] = 0
    assert not shared_first_row(ids, masked) and shared_first_row(ids, None)       # one text masks position 0
    assert not shared_first_row(ids[:, :1], att[:, :1])                            # one position per text: nothing to share
    assert not shared_first_row(ids.to("meta"), None)                              # ids not on the host: never examined
    assert not shared_first_row(ids, att.to("meta"))
    assert not shared_first_row(ids.view(5, 1, T), None)
    # what the encoder hands to Engine.text: the lengths (EOS position + 1) with the predicate of the ids they came from
    from types import SimpleNamespace
    from outfitx_amd.encoders import CLIPTextEncoder
    enc = SimpleNamespace(model=SimpleNamespace(config=SimpleNamespace(eos_token_id=2)))       # all that _lengths reads of its encoder
    enc._lengths = lambda *a: CLIPTextEncoder._lengths(enc, *a)
    ln = enc._lengths(ids, att)
    assert isinstance(ln, TextLengths) and list(ln) == [2, 8, 3, 8, 5] and ln.shared_first
    assert not enc._lengths(other, att).shared_first and not enc._lengths(ids, masked).shared_first
    assert enc._lengths(ids, None).shared_first
    assert not enc._lengths(ids).shared_first                                      # no word about the mask: the full rows
    assert enc._lengths(ids.to("meta"), None) is None
    assert TextLengths([3, 4]).shared_first is False and TextLengths([3, 4], True) == [3, 4]


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import warnings
    warnings.simplefilter("ignore")
    from src.models import OutfitX
    from src.models.configs import ItemEncoderConfig, OutfitXConfig
    m = OutfitX(OutfitXConfig(item_encoder=ItemEncoderConfig(type="clip")))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.full_state_dict(W_SEED).items()}, strict=True)
    return m.cuda().eval()


@contextlib.contextmanager
def knobs(**kv):
    """knobs(k21=0, k15=2): ofx_tune(21, 0), ofx_tune(15, 2); the defaults again on the way out."""
    from outfitx_amd import _lib as L
    lib = L.load()
    try:
        for k, v in kv.items():
            L.check(lib.ofx_tune(int(k[1:]), v), "ofx_tune")
        yield
    finally:
        for k in kv:
            lib.ofx_tune(int(k[1:]), KNOB_DEFAULTS[int(k[1:])])


def batch(N, Tc):
    """N ragged texts whose longest computes Tc positions: text 0's EOS sits at Tc - 1, the last text's at position 1 (BOS, EOS),
    the others' anywhere between; the attention mask is zero after the EOS."""
    g = np.random.default_rng(1000 * N + Tc)
    n = g.integers(2, Tc + 1, N)
    n[0] = Tc
    if N > 1:
        n[-1] = 2
    ids, att = synth.token_batch(N * 100 + Tc, N, T, n)
    assert ((att == 1) == (np.arange(T)[None] < n[:, None])).all() and (ids[np.arange(N), n - 1] == synth.EOS_ID).all()
    return ids, att


def embed(model, ids, att, normalize, device_ids=False):
    N = ids.shape[0]
    to = (lambda a: torch.from_numpy(a).cuda()) if device_ids else torch.from_numpy
    inp = {"input_ids": to(ids).view(N, 1, T), "attention_mask": None if att is None else to(att).view(N, 1, T)}
    if att is None:
        del inp["attention_mask"]
    with torch.no_grad():
        return model.item_encoder.text_enc(inp, normalize=normalize).view(N, -1).clone()


def qkv_gemm_rows(fn):
    """fn() under the GEMM profile: (fn's result, M of every text-tower QKV GEMM it launched: N = 3 x 512 columns, depth 512 three times)."""
    from outfitx_amd import _lib as L
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
    return out, [r.M for r in recs[:n] if r.cat == 0 and r.N == 1536 and r.K == 512 and r.kmul == 3]


@pytest.mark.gpu
@pytest.mark.parametrize("Tc", TCS)
@pytest.mark.parametrize("N", NS)
def test_mode_on_is_bit_identical_to_knob_off(model, N, Tc):
    ids, att = batch(N, Tc)
    assert model.item_encoder.text_enc.tower_precision.startswith("f16w2")        # the default scheme: three-product text tower
    for fixed in ({"k15": 2}, {"k2": 1, "k5": 0}):                                  # summation order independent of M
        for normalize in (False, True):
            with knobs(**fixed):
                on, rows_on = qkv_gemm_rows(lambda: embed(model, ids, att, normalize))
                with knobs(k21=0):
                    off, rows_off = qkv_gemm_rows(lambda: embed(model, ids, att, normalize))
            assert rows_on == [1 + N * (Tc - 1)] * 12 and rows_off == [N * Tc] * 12, (rows_on, rows_off)
            assert torch.isfinite(on).all() and torch.equal(on, off), (fixed, normalize, (on - off).abs().max().item())


_oracle = {}


def oracle(N, Tc):
    """(rows, un-normalised oracle embeddings of those rows), computed once per case; the ids cut at Tc columns - causal attention:
    what follows the last EOS of the batch reaches no pooled row."""
    if (N, Tc) not in _oracle:
        ids, att = batch(N, Tc)
        rows = np.arange(N) if N <= 37 else np.unique(np.concatenate([[0, N - 1], np.linspace(1, N - 2, 22).astype(int)]))
        _oracle[(N, Tc)] = rows, O.text_forward(ids[rows, :Tc], att[rows, :Tc], synth.text_weights(W_SEED))
    return _oracle[(N, Tc)]


@pytest.mark.gpu
@pytest.mark.parametrize("Tc", TCS)
@pytest.mark.parametrize("N", NS)
def test_both_modes_vs_oracle_at_default_knobs(model, N, Tc):
    ids, att = batch(N, Tc)
    rows, want = oracle(N, Tc)
    want_n = want / np.maximum(np.linalg.norm(want, axis=-1, keepdims=True), 1e-12)
    for normalize in (False, True):
        on = embed(model, ids, att, normalize).cpu().numpy()
        with knobs(k21=0):
            off = embed(model, ids, att, normalize).cpu().numpy()
        ref = want_n if normalize else want
        e_on, e_off = rel_err(on[rows], ref), rel_err(off[rows], ref)
        print(f"N={N} Tc={Tc} normalize={normalize}: shared {e_on:.2e} full {e_off:.2e}")
        assert e_on < 1e-3 and e_off < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["first_ids_differ", "mask_column0_zero", "one_token", "device_ids"])
def test_fallbacks_run_the_full_rows(model, case):
    N, Tc = 37, 8
    ids, att = batch(N, Tc)
    device_ids = case == "device_ids"
    if case == "first_ids_differ":
        ids[5, 0] = synth.BOS_ID - 1                        # (below the EOS id: the pooled position stays)
    elif case == "mask_column0_zero":
        att[9, 0] = 0
    elif case == "one_token":                                # every EOS at position 0: one computed token per text
        ids[:] = synth.EOS_ID
        att[:] = 0; att[:, 0] = 1
        Tc = 1
    elif case == "device_ids":
        Tc = T                                               # no host lengths: all T positions
    got, rows = qkv_gemm_rows(lambda: embed(model, ids, att, True, device_ids))
    with knobs(k21=0):
        off, rows_off = qkv_gemm_rows(lambda: embed(model, ids, att, True, device_ids))
    assert rows == [N * Tc] * 12 == rows_off, (rows, rows_off)
    assert torch.isfinite(got).all() and torch.equal(got, off)


@pytest.mark.gpu
def test_a_batch_that_stops_sharing_is_not_replayed_from_the_shared_graph(model):
    from outfitx_amd.graphs import capture_cp_forward
    from src.models.datatypes import OutfitCompatibilityPredictionTask as CP
    B, n = 2, 2
    px = torch.from_numpy(synth.pixel_values(811, B * n).reshape(B, n, 3, 224, 224)).cuda()
    ids, att = synth.token_batch(811, B * n, T, [8, 5, 2, 7])
    texts = {"input_ids": torch.from_numpy(ids).view(B, n, T).pin_memory(), "attention_mask": torch.from_numpy(att).view(B, n, T).pin_memory()}
    mask = torch.zeros(B, n, dtype=torch.bool, device="cuda")
    call = lambda: model(task=CP, outfit_embedding=None, outfit_mask=mask, encoder_input_dict={"images": px, "texts": texts})
    was, model._replay = model.graph_replay, None
    try:
        with torch.no_grad():
            # the explicit capture: replays while the pinned ids share their first token, raises once they do not
            model.graph_replay = False
            ref, rows = qkv_gemm_rows(lambda: call().clone())
            assert rows == [1 + B * n * 7] * 12
            cap = capture_cp_forward(model, mask, px, texts)
            assert cap.captured_shared_first and torch.equal(cap.replay(), ref)
            # the drop-in call: launch by launch twice, captured, replayed
            model.graph_replay = True
            outs = [call() for _ in range(4)]
            st = model._replay.stats
            assert (st["eager"], st["captures"], st["replays"]) == (2, 1, 2) and all(torch.equal(o, ref) for o in outs)
            texts["input_ids"][1, 0, 0] = synth.BOS_ID - 1            # in place: column 0 is no longer uniform
            with pytest.raises(ValueError, match="share their first position"):
                cap.replay()
            assert cap.replays == 1
            got = call()                                              # another key: launch by launch, full rows
            assert (st["eager"], st["captures"], st["replays"]) == (3, 1, 2)
            model.graph_replay = False
            full, rows = qkv_gemm_rows(lambda: call().clone())
            assert rows == [B * n * 8] * 12
            with knobs(k21=0):
                off = call().clone()
            assert torch.equal(got, full) and torch.equal(got, off) and not torch.equal(got, ref)
    finally:
        model.graph_replay, model._replay = was, None
