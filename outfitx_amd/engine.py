"""Thin Python host over the C ABI: owns an ofx_handle, packs torch parameters into it, lends
torch-allocated workspaces and output tensors, and launches on torch's current HIP stream.

PyTorch is plumbing here (device memory, streams); all arithmetic happens in libofx_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import _lib as L


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _f32c(t: torch.Tensor, device) -> torch.Tensor:
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    return t


def shared_first_row(ids: torch.Tensor, att: Optional[torch.Tensor]) -> bool:
    """Whether the text tower may compute position 0 once for all texts of ids [N, T] (ofx_clip_text_fwd_shared's precondition): the ids are
    on the host (the test costs no device sync), every text starts with the same token (CLIP's BOS) and no text masks position 0.  The
    tower is causal, so position 0 then is the same row for every text in every layer.  Tc >= 2 and the three-product scheme, the other
    two conditions of the mode, are Engine.text's to check."""
    if ids.device.type != "cpu" or ids.dim() != 2 or ids.shape[0] < 1 or ids.shape[1] < 2:
        return False
    if not bool((ids[:, 0] == ids[0, 0]).all()):
        return False
    if att is not None and (att.device.type != "cpu" or att.shape != ids.shape or not bool((att[:, 0] != 0).all())):
        return False
    return True


class TextLengths(list):
    """Tokens to compute per text (EOS position + 1) as CLIPTextEncoder computes them from host ids, with shared_first_row of those ids:
    the ids travel to the device before Engine.text sees them, the host-side facts about them travel here."""

    def __init__(self, lengths, shared_first: bool = False):
        super().__init__(lengths)
        self.shared_first = bool(shared_first)


class SetInput(NamedTuple):
    """A staged set input (Engine.stage_set).  `args` are the seven set-input arguments in ofx_cir_train_fwd's order - x, pad_mask,
    table, ld, n_table, item_index, cu_items -: the dense form fills the first two, the indexed form the other five."""
    B: int
    L: int
    staged: tuple            # the device tensors behind the pointers in `args` that this call may have made
    args: tuple

    @property
    def indexed(self) -> bool:
        return self.args[0] is None


class Engine:
    """One per (module, device).  `precision`: MFMA operand format of the outfit transformer
    ('bf16x3' | 'bf16' | 'f16'); `tower_precision`: operand scheme of the CLIP towers - a name `_lib.tower_scheme` accepts: 'f16w2x' (default:
    every ViT weight split; all 100 weight seeds swept at the bench's batch size inside 1e-3 of the reference, worst 6.3e-4) | 'f16w2h' (the qkv
    correction on ViT layers 0-5 only: 3 % faster, worst 7.35e-4 at that batch size, outside 1e-3 on one small-logit 8-outfit draw) | 'f16w2' (faster; worst seeds at 1.0e-3) | 'f16x3' (every
    tower GEMM three-product) | 'f16' | 'bf16' (single product, outside 1e-3) | any of them + '@qkv=<layers>;fc1=...' (per-layer rungs)."""

    def __init__(self, device: torch.device, desc: Optional[L.ModelDesc] = None,
                 precision: str = "bf16x3", tower_precision: str = L.DEFAULT_TOWER_PRECISION):
        self.lib = L.load()
        if device.type != "cuda":
            raise L.OfxError(f"outfitx_amd runs on an MI355X HIP device only (got {device}); there is no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        d = desc if desc is not None else L.default_desc()
        d.outfit_precision = L.PRECISIONS[precision]
        for k, v in L.tower_scheme(tower_precision).items():       # ValueError on an unknown scheme
            setattr(d, k, v)
        self.desc = d
        self.h = self.lib.ofx_create(self.device.index, C.byref(d))
        if not self.h:
            raise L.OfxError("ofx_create failed: " + self.lib.ofx_last_error().decode())
        self._ws: Dict[int, torch.Tensor] = {}
        self._keep: List[torch.Tensor] = []
        self.signature = {"outfit": None, "vision": None, "text": None}

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ofx_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---------------------------------------------------------------- weights
    def _pack(self, fn, tensors: Sequence[torch.Tensor], what: str):
        ts = [_f32c(t.detach(), self.device) for t in tensors]
        arr = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        with torch.cuda.device(self.device):
            L.check(fn(self.h, arr, len(ts), _stream(self.device)), f"ofx_pack_{what}_weights")
        # the pack kernels read `ts` asynchronously on the current stream; keep temporaries alive until they are done
        self._keep = [t for t in ts]

    def pack_outfit(self, tensors): self._pack(self.lib.ofx_pack_outfit_weights, tensors, "outfit")
    def pack_vision(self, tensors): self._pack(self.lib.ofx_pack_vision_weights, tensors, "vision")
    def pack_text(self, tensors): self._pack(self.lib.ofx_pack_text_weights, tensors, "text")

    # ---------------------------------------------------------------- workspace
    def workspace(self, nbytes: int) -> torch.Tensor:
        key = _stream(self.device)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(int(nbytes * 1.05) + 4096, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def ws_bytes(self, op: int, n: int, length: int) -> int:
        return int(self.lib.ofx_workspace_bytes(self.h, op, n, length))

    @staticmethod
    def cir_sample_batch(split: Dict[str, torch.Tensor], pools: Dict[str, torch.Tensor], outfit_ids: torch.Tensor, seed: int, draw: int, K: int,
                         max_len: int, n_pool_rows: Optional[int] = None):
        """One CIR training batch drawn on the device (ofx_cir_sample_batch; semantics in include/ofx.h).  The entry is stateless: it
        takes no handle, so a dataset calls this without an engine.  split: the int32 device tensors 'outfit_cu', 'outfit_rows', 'pos_cu',
        'pos_slots'; pools: 'pool_cu', 'pool_rows', 'row_pool', 'row_slot' (sampler.CIRDeviceDataset and sampler.CIRNegativePools build
        both); outfit_ids: int32 [B] on the same device (another dtype or device, or a view that is not 16-byte aligned, is copied
        first).  n_pool_rows: the live length of pool_rows when the tensor is longer (an empty array is uploaded as one element).
        -> (item_index [B * max_len] - compact, its tail past cu_seqlens[B] is uninitialised -, cu_seqlens [B + 1], target_item_index [B],
        neg_items_index [B, K]), int32.  Two launches on the current stream; no copy to or from the host and no wait when outfit_ids is
        already an aligned device tensor."""
        lib = L.load()
        dev = split["outfit_cu"].device
        if dev.type != "cuda":
            raise L.OfxError("cir_sample_batch needs HIP tensors; there is no CPU path")
        ts = [split[k] for k in ("outfit_cu", "outfit_rows", "pos_cu", "pos_slots")] + [pools[k] for k in ("pool_cu", "pool_rows", "row_pool", "row_slot")]
        for t in ts:
            if t.device != dev or t.dtype != torch.int32 or not t.is_contiguous():
                raise ValueError(f"cir_sample_batch: every table must be a contiguous int32 tensor on {dev}")
        ocu, orows, pcu, pslots, gcu, grows, rpool, rslot = ts
        if rpool.numel() != rslot.numel() or pcu.numel() != ocu.numel():
            raise ValueError("cir_sample_batch: row_pool / row_slot or outfit_cu / pos_cu differ in length")
        ids = outfit_ids if isinstance(outfit_ids, torch.Tensor) else torch.as_tensor(outfit_ids)
        ids = ids.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        if ids.data_ptr() % 16:
            ids = ids.clone()                                   # a slice of a longer tensor: a fresh allocation is aligned
        B, K, max_len = ids.numel(), int(K), int(max_len)
        item_index = torch.empty(max(B * max_len, 1), dtype=torch.int32, device=dev)
        cu = torch.empty(B + 1, dtype=torch.int32, device=dev)
        target = torch.empty(B, dtype=torch.int32, device=dev)
        neg = torch.empty(B, max(K, 0), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.ofx_cir_sample_batch(_ptr(ocu), _ptr(orows), ocu.numel() - 1, orows.numel(), _ptr(pcu), _ptr(pslots), pslots.numel(), _ptr(gcu),
                                             _ptr(grows), gcu.numel() - 1, grows.numel() if n_pool_rows is None else int(n_pool_rows), _ptr(rpool),
                                             _ptr(rslot), rpool.numel(), _ptr(ids), B, int(seed) & 0xFFFFFFFF,
                                             int(draw) & 0xFFFFFFFF, K, max_len, _ptr(item_index), _ptr(cu), _ptr(target), _ptr(neg) if K > 0 else None,
                                             _stream(dev)), "ofx_cir_sample_batch")
        return item_index, cu, target, neg

    # ---------------------------------------------------------------- outfit transformer
    def stage_set(self, setin) -> "SetInput":
        """The one place that validates and stages a set input: (x [B,L,D] float, mask [B,L], True / non-zero = pad) or the indexed
        (varlen) form (table [n,D], item_index, cu_seqlens, max_len).  Host-side index tensors are checked here (range, monotone
        offsets, items per outfit); device-side ones are trusted (the kernel clamps indices).  The staged tensors stay referenced
        until the next call: the kernels (and the non-blocking copies) read them asynchronously on the current stream."""
        if len(setin) == 4:
            table, item_index, cu_seqlens, Lq = setin
            if table.device != self.device or table.dtype != torch.float32 or table.dim() != 2 or table.stride(1) != 1:
                raise L.OfxError("embedding table must be a [n, D] fp32 tensor on the engine's device with unit column stride")
            if table.shape[1] != self.desc.d_model:
                raise L.OfxError(f"embedding table has {table.shape[1]} columns, the model needs {self.desc.d_model}")
            B = cu_seqlens.numel() - 1
            max_items = None
            if cu_seqlens.device.type == "cpu":
                cu = cu_seqlens.to(torch.int64)
                n = cu[1:] - cu[:-1]
                if B < 1 or int(cu[0]) != 0 or bool((n < 0).any()) or int(cu[-1]) != item_index.numel():
                    raise ValueError("cu_seqlens must start at 0, be non-decreasing and end at len(item_index)")
                max_items = int(n.max())
            if item_index.device.type == "cpu" and item_index.numel():
                lo, hi = int(item_index.min()), int(item_index.max())
                if lo < 0 or hi >= table.shape[0]:
                    raise IndexError(f"item_index out of range [0, {table.shape[0]}): min {lo}, max {hi}")
            idx = item_index.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
            cud = cu_seqlens.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
            if max_items is not None and max_items > Lq:
                raise ValueError(f"an outfit holds {max_items} items, max_len is {Lq} (truncate in the processor)")
            s = SetInput(B, Lq, (idx, cud), (None, None, _ptr(table), table.stride(0), table.shape[0], _ptr(idx), _ptr(cud)))
        else:
            x, mask = setin
            B, Lq, _ = x.shape
            x = _f32c(x, self.device)
            m = mask.to(device=self.device)
            m = (m if m.dtype == torch.bool else m != 0).contiguous().view(torch.uint8)
            s = SetInput(B, Lq, (x, m), (_ptr(x), _ptr(m), None, 0, 0, None, None))
        self._keep_set = s.staged
        return s

    def _prefix(self, prefix: Optional[torch.Tensor]):
        """Prefix token(s) -> (staged fp32 tensor or None, row stride): one [D] row for every outfit (stride 0) or one row per outfit."""
        if prefix is None:
            return None, 0
        prefix = _f32c(prefix, self.device)
        return prefix, 0 if prefix.dim() == 1 else self.desc.d_model

    def set_encoder(self, setin, prefix: Optional[torch.Tensor] = None) -> torch.Tensor:
        """setin (either form of stage_set) -> encoder output at the prefix token [B,D] fp32."""
        s = self.stage_set(setin)
        prefix, stride = self._prefix(prefix)
        out = torch.empty(s.B, self.desc.d_model, dtype=torch.float32, device=self.device)
        ws = self.workspace(self.ws_bytes(L.OP_SET_ENCODER, s.B, s.L))
        name, lead = ("ofx_set_encoder_fwd_indexed", s.args[2:]) if s.indexed else ("ofx_set_encoder_fwd", s.args[:2])
        with torch.cuda.device(self.device):
            L.check(getattr(self.lib, name)(self.h, *lead, _ptr(prefix), stride, s.B, s.L, _ptr(out), _ptr(ws), ws.numel(),
                                            _stream(self.device)), name)
        return out

    def cp_head(self, row0: torch.Tensor) -> torch.Tensor:
        B = row0.shape[0]
        out = torch.empty(B, 1, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_cp_head(self.h, _ptr(row0), B, _ptr(out), _stream(self.device)), "ofx_cp_head")
        return out

    def cir_head(self, row0: torch.Tensor) -> torch.Tensor:
        B, D = row0.shape
        out = torch.empty(B, D, dtype=torch.float32, device=self.device)
        ws = self.workspace(B * D * 2 * 3 + 256)
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_cir_head(self.h, _ptr(row0), B, _ptr(out), _ptr(ws), ws.numel(), _stream(self.device)), "ofx_cir_head")
        return out

    def cir_prefix(self, target_text: torch.Tensor) -> torch.Tensor:
        t = _f32c(target_text, self.device)
        B = t.shape[0]
        out = torch.empty(B, self.desc.d_model, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_cir_prefix(self.h, _ptr(t), B, _ptr(out), _stream(self.device)), "ofx_cir_prefix")
        return out

    # ---------------------------------------------------------------- training step (CP and CIR paths, next row N1)
    def grad_layout(self):
        n = 5 + 12 * self.desc.n_layers
        offs = (C.c_size_t * n)()
        total = int(self.lib.ofx_cp_train_grad_floats(self.h, offs, n))
        return total, list(offs)

    def _train_ws(self, B: int, Lq: int) -> torch.Tensor:
        return self.workspace(int(self.lib.ofx_cp_train_ws_bytes(self.h, B, Lq)))

    def train_fwd(self, head: str, setin, target_text: Optional[torch.Tensor] = None, dropout_p: float = 0.0, seed: int = 0):
        """Tape-saving forward of the CP ('cp': -> logits [B,1]) or the CIR / FITB ('cir': target_text [B,512] -> y [B,D]) path over
        either form of set input (stage_set).  -> (out fp32, tape uint8 tensor - a fresh one per call, owned by the caller -, (B, L))"""
        width = {"cp": 1, "cir": self.desc.d_model}[head]
        txt = _f32c(target_text, self.device) if head == "cir" else None
        s = self.stage_set(setin)
        tape = torch.empty(int(self.lib.ofx_cp_train_tape_bytes(self.h, s.B, s.L)), dtype=torch.uint8, device=self.device)
        ws = self._train_ws(s.B, s.L)
        out = torch.empty(s.B, width, dtype=torch.float32, device=self.device)
        if head == "cir":
            name, lead = "ofx_cir_train_fwd", s.args + (_ptr(txt),)
        else:
            name, lead = ("ofx_cp_train_fwd_indexed", s.args[2:]) if s.indexed else ("ofx_cp_train_fwd", s.args[:2])
        with torch.cuda.device(self.device):
            L.check(getattr(self.lib, name)(self.h, *lead, s.B, s.L, _ptr(out), _ptr(tape), tape.numel(), _ptr(ws), ws.numel(),
                                            float(dropout_p), int(seed) & 0xFFFFFFFF, _stream(self.device)), name)
        return out, tape, (s.B, s.L)

    def train_bwd(self, head: str, tape: torch.Tensor, dhead: torch.Tensor, B: int, Lq: int, dropout_p: float = 0.0, seed: int = 0,
                  dests=None) -> Optional[torch.Tensor]:
        """Backward of the 'cp' / 'cir' path from d loss / d head output ([B,1] / [B,D]).  dests None: -> a flat fp32 gradient buffer
        (layout: grad_layout()).  dests given (one fp32 contiguous tensor of the parameter's shape per packed tensor, None for tensors
        off the path): every gradient is ADDED straight into them - p.grad += g without the 75 accumulate kernels of autograd - and
        nothing is returned."""
        if dests is None:
            total, _ = self.grad_layout()
            g = torch.empty(total, dtype=torch.float32, device=self.device)
            name, sink = f"ofx_{head}_train_bwd", (_ptr(g), total)
        else:
            g = None
            ptrs = (C.c_void_p * len(dests))(*[None if t is None else t.data_ptr() for t in dests])
            name, sink = f"ofx_{head}_train_bwd_into", (ptrs, len(dests), 1)         # 1: accumulate
        d = _f32c(dhead, self.device)
        ws = self._train_ws(B, Lq)
        with torch.cuda.device(self.device):
            L.check(getattr(self.lib, name)(self.h, _ptr(tape), tape.numel(), _ptr(d), B, Lq, *sink, _ptr(ws), ws.numel(),
                                            float(dropout_p), int(seed) & 0xFFFFFFFF, _stream(self.device)), name)
        return g

    def arm_layer_events(self, events) -> None:
        """events: one torch.cuda.Event per outfit-transformer layer (each recorded at least once, so that its HIP handle exists);
        the NEXT backward call records events[l] when layer l's gradients are final (ofx_train_arm_layer_events)."""
        arr = (C.c_void_p * len(events))(*[int(e.cuda_event) for e in events])
        L.check(self.lib.ofx_train_arm_layer_events(self.h, arr, len(events)), "ofx_train_arm_layer_events")

    # ---------------------------------------------------------------- towers
    @staticmethod
    def _check_out_rows(out: torch.Tensor, n: int, who: str) -> None:
        """The towers write n rows of out: the library sees a pointer and a stride, so a shorter buffer is refused HERE, before anything is
        launched (a caller that sized out by another count - images and texts that disagree - would otherwise have rows written past its end)."""
        if out.dim() != 2 or out.shape[0] < n:
            raise ValueError(f"{who}: out has shape {tuple(out.shape)}, the tower writes {n} rows")

    def vit(self, pixels: torch.Tensor, out: torch.Tensor, col: int, normalize: bool) -> None:
        """pixels [N,3,H,W] fp32 pixel_values -> out[:, col:col+512] (out is [N, ld] fp32 contiguous)."""
        px = _f32c(pixels, self.device)
        N = px.shape[0]
        self._check_out_rows(out, N, "vit")
        nb = self.ws_bytes(L.OP_VIT, N, 0)
        ws = self.workspace(nb)
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_vit_b32_fwd(self.h, _ptr(px), N, _ptr(out), out.stride(0), col, int(normalize),
                                             _ptr(ws), ws.numel(), _stream(self.device)), "ofx_vit_b32_fwd")

    def _stage_images(self, images: Sequence):
        """uint8 images -> (device byte buffer, host offsets / heights / widths): one pinned staging copy, one H2D."""
        import numpy as np
        arrs = []
        for a in images:
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
                raise ValueError(f"clip_preprocess takes uint8 [H,W,3] or [H,W] images, got {a.dtype} {a.shape}")
            arrs.append(np.repeat(a[:, :, None], 3, 2) if a.ndim == 2 else a)
        N = len(arrs)
        hs = np.asarray([a.shape[0] for a in arrs], np.int32); ws_ = np.asarray([a.shape[1] for a in arrs], np.int32)
        nbytes = hs.astype(np.int64) * ws_ * 3
        offs = np.zeros(N, np.int64); offs[1:] = np.cumsum((nbytes[:-1] + 15) // 16 * 16)
        total = int(offs[-1] + nbytes[-1])
        stage = getattr(self, "_px_stage", None)
        if stage is None or stage.numel() < total + 4:
            stage = torch.empty(int(total * 1.25) + 4096, dtype=torch.uint8).pin_memory()
            self._px_stage = stage
        elif getattr(self, "_px_event", None) is not None:
            self._px_event.synchronize()      # only the previous batch's H2D copy (not the kernels queued behind it) must have left the staging buffer
        buf = stage.numpy()
        for a, o, n in zip(arrs, offs, nbytes):
            buf[o:o + n] = a.reshape(-1)
        src = stage[:total + 4].to(self.device, non_blocking=True)    # + 4: RGB pixels are fetched as unaligned dwords
        self._px_event = torch.cuda.Event()
        self._px_event.record(torch.cuda.current_stream(self.device))
        self._keep_px = src
        return src, offs, hs, ws_

    def clip_preprocess(self, images: Sequence, size: int, mean: Sequence[float], std: Sequence[float]) -> torch.Tensor:
        """uint8 images ([H,W,3] or [H,W] numpy arrays, any sizes) -> normalised pixel_values [N,3,size,size] fp32 on the
        device: the packed bytes travel once (0.27 MB per 300x300 image instead of 0.6 MB of fp32 pixels) and the resize /
        crop / normalise run on the GPU, bit-identical to PIL + CLIPImageProcessor (ofx_clip_preprocess)."""
        src, offs, hs, ws_ = self._stage_images(images)
        N = len(hs)
        out = torch.empty(N, 3, size, size, dtype=torch.float32, device=self.device)
        I = C.POINTER(C.c_int); LL = C.POINTER(C.c_longlong)
        nb = int(self.lib.ofx_clip_preprocess_ws(hs.ctypes.data_as(I), ws_.ctypes.data_as(I), N, 3, size))
        ws = self.workspace(nb)
        m = (C.c_float * 3)(*mean); sd = (C.c_float * 3)(*std)
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_clip_preprocess(_ptr(src), offs.ctypes.data_as(LL), hs.ctypes.data_as(I), ws_.ctypes.data_as(I), N, 3, size,
                                                 m, sd, _ptr(out), _ptr(ws), ws.numel(), _stream(self.device)), "ofx_clip_preprocess")
        return out

    def vit_u8(self, images: Sequence, mean: Sequence[float], std: Sequence[float], out: torch.Tensor, col: int, normalize: bool) -> None:
        """uint8 images -> out[:, col:col+512]: the GPU preprocessor feeds the patch-embedding GEMM directly
        (ofx_vit_b32_fwd_u8); same result as clip_preprocess + vit without the fp32 pixel tensor in between."""
        self._check_out_rows(out, len(images), "vit_u8")
        src, offs, hs, ws_ = self._stage_images(images)
        N = len(hs)
        I = C.POINTER(C.c_int); LL = C.POINTER(C.c_longlong)
        nb = int(self.lib.ofx_vit_b32_u8_ws_bytes(self.h, hs.ctypes.data_as(I), ws_.ctypes.data_as(I), N, 3))
        if nb == 0:
            raise ValueError("ofx_vit_b32_u8_ws_bytes: bad image geometry")
        ws = self.workspace(nb)
        m = (C.c_float * 3)(*mean); sd = (C.c_float * 3)(*std)
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_vit_b32_fwd_u8(self.h, _ptr(src), offs.ctypes.data_as(LL), hs.ctypes.data_as(I), ws_.ctypes.data_as(I), N, 3,
                                                m, sd, _ptr(out), out.stride(0), col, int(normalize), _ptr(ws), ws.numel(),
                                                _stream(self.device)), "ofx_vit_b32_fwd_u8")

    def stage_tokens(self, ids: torch.Tensor, att: Optional[torch.Tensor]):
        """Token ids / mask -> device int64 (non-blocking from pinned memory).  Call this BEFORE enqueuing a long
        kernel sequence: a blocking H2D copy in the middle of a step stalls the host behind everything queued."""
        def mv(t):
            if t is None:
                return None
            if t.device == self.device and t.dtype == torch.int64 and t.is_contiguous():
                return t
            return t.to(device=self.device, dtype=torch.int64, non_blocking=t.device.type == "cpu" and t.is_pinned()).contiguous()
        return mv(ids), mv(att)

    def text(self, ids: torch.Tensor, att: Optional[torch.Tensor], out: torch.Tensor, col: int, normalize: bool,
             lengths: Optional[Sequence[int]] = None) -> None:
        """ids/att [N,T] int64 -> out[:, col:col+512].  lengths: host ints (EOS position + 1) or None; a TextLengths carries the
        shared-first-row predicate of the host ids it was computed from (the ids themselves may already be on the device), host ids
        passed here are examined directly, anything else computes the full rows."""
        self._check_out_rows(out, ids.shape[0], "text")
        shared = lengths.shared_first if isinstance(lengths, TextLengths) else shared_first_row(ids, att)
        ids_d, att_d = self.stage_tokens(ids, att)
        N, T = ids_d.shape
        Tc = T if lengths is None else max(1, min(T, max(int(v) for v in lengths)))
        arr = None if lengths is None else (C.c_int * N)(*[int(v) for v in lengths])
        nb = self.ws_bytes(L.OP_TEXT, N, Tc)
        ws = self.workspace(nb)
        shared = bool(shared) and Tc >= 2 and bool(self.desc.txt_x3)      # (the library checks the last two again, and its ofx_tune(21) knob)
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_clip_text_fwd_shared(self.h, _ptr(ids_d), _ptr(att_d), arr, N, T, _ptr(out), out.stride(0), col,
                                                      int(normalize), int(shared), _ptr(ws), ws.numel(), _stream(self.device)), "ofx_clip_text_fwd_shared")
        self._keep_ids = (ids_d, att_d)

    # ---------------------------------------------------------------- scoring
    def l2_topk(self, Q: torch.Tensor, P: torch.Tensor, k: int, index_base: int = 0):
        Q = _f32c(Q, self.device); P = _f32c(P, self.device)
        nq, D = Q.shape
        npool = P.shape[0]
        idx = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        dist = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        ws = self.workspace(self.ws_bytes(L.OP_TOPK, nq, npool))
        with torch.cuda.device(self.device):
            L.check(self.lib.ofx_l2_topk(self.h, _ptr(Q), _ptr(P), nq, npool, D, k, index_base, _ptr(idx), _ptr(dist),
                                         _ptr(ws), ws.numel(), _stream(self.device)), "ofx_l2_topk")
        return idx, dist

    def l2_topk_grouped(self, Q: torch.Tensor, group_of_query, P: torch.Tensor, pool_offsets, k: int, gt=None, max_ws_bytes: int = 1 << 30):
        """Category-pool retrieval (complementary_item_retrieval_trainer.py:192-249, demo/app.py:184-190): query i searches only pool
        rows [pool_offsets[g], pool_offsets[g + 1]) of P, g = group_of_query[i].  One ofx_l2_topk_grouped call (4 launches) for all
        groups, or one per chunk of queries when the distance buffer would exceed max_ws_bytes.

        Q [nq, D] in the caller's order; group_of_query: nq host ints (sequence or CPU tensor); P [np, D]: all pools concatenated;
        pool_offsets: G + 1 host ints; gt: optional nq rows of P (the ground truth inside the query's own pool; < 0 = none).
        -> (idx int64 [nq, k] rows of P, dist fp32 [nq, k], gt_pos int32 [nq] | None), in the caller's order.  Per query the result has
        the bits of l2_topk(Q[i:i+1], P[lo:hi], k, index_base=lo); a pool of fewer than k rows ends in idx -1 / dist +inf.  gt_pos is
        the position of gt in idx, k when it is not among them, and -1 for a query without ground truth (parallel.grouped_recall
        leaves those out of the ratio).  ValueError before any launch: a group id outside [0, G), a query whose pool is empty, offsets
        that do not start at 0, decrease or end elsewhere than at np, a gt outside its query's pool, a max_ws_bytes that one query
        does not fit."""
        Q = _f32c(Q, self.device); P = _f32c(P, self.device)
        nq, D = Q.shape
        npool = P.shape[0]
        grp = torch.as_tensor(group_of_query, device="cpu").to(torch.int64).reshape(-1)
        off = torch.as_tensor(pool_offsets, device="cpu").to(torch.int64).reshape(-1)
        G = off.numel() - 1
        if G < 1 or int(off[0]) != 0 or int(off[-1]) != npool or bool((off[1:] < off[:-1]).any()):
            raise ValueError("pool_offsets must start at 0, be non-decreasing and end at len(P)")
        if grp.numel() != nq:
            raise ValueError(f"group_of_query has {grp.numel()} entries for {nq} queries")
        if nq and (int(grp.min()) < 0 or int(grp.max()) >= G):
            raise ValueError(f"group_of_query must lie in [0, {G})")
        q_lo, q_hi = off[grp], off[grp + 1]
        if bool((q_hi == q_lo).any()):
            raise ValueError("a query's pool is empty")
        gt_h = None
        if gt is not None:
            gt_h = torch.as_tensor(gt).to(device="cpu", dtype=torch.int64).reshape(-1)
            if gt_h.numel() != nq:
                raise ValueError(f"gt has {gt_h.numel()} entries for {nq} queries")
            if bool(((gt_h >= 0) & ((gt_h < q_lo) | (gt_h >= q_hi))).any()):
                raise ValueError("a gt row lies outside its query's pool")
        idx = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        dist = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        gt_pos = torch.empty(nq, dtype=torch.int32, device=self.device) if gt_h is not None else None
        if nq == 0:
            return idx, dist, gt_pos
        max_rows = int((q_hi - q_lo).max())
        need = lambda n: int(self.lib.ofx_l2_topk_grouped_ws(n, npool, max_rows))
        if need(1) > max_ws_bytes:
            raise ValueError(f"max_ws_bytes={max_ws_bytes}: one query against {max_rows} rows needs {need(1)} bytes")
        lo, hi = 1, nq                                   # most queries per call whose workspace fits
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if need(mid) <= max_ws_bytes else (lo, mid - 1)
        n_chunks = -(-nq // lo)
        chunk = -(-nq // n_chunks)
        # queries sorted by group (stable: the caller's order inside a group)
        order = torch.argsort(grp, stable=True)
        table, chunk_panels = _group_panels(grp[order], off, chunk)
        table = table.to(self.device)
        order_d = order.to(self.device)
        Qs = Q.index_select(0, order_d)
        gt_s = gt_h[order].to(self.device) if gt_h is not None else None
        idx_s, dist_s = torch.empty_like(idx), torch.empty_like(dist)
        pos_s = torch.empty_like(gt_pos) if gt_pos is not None else None
        ws = self.workspace(need(chunk))
        with torch.cuda.device(self.device):
            for c0, c1, first, n_panels in chunk_panels:
                L.check(self.lib.ofx_l2_topk_grouped(self.h, _ptr(Qs[c0:c1]), _ptr(P), c1 - c0, npool, D, k, _ptr(table[first:]), n_panels, max_rows,
                                                     _ptr(gt_s[c0:c1]) if gt_s is not None else None, _ptr(idx_s[c0:c1]), _ptr(dist_s[c0:c1]),
                                                     _ptr(pos_s[c0:c1]) if pos_s is not None else None, _ptr(ws), ws.numel(), _stream(self.device)),
                        "ofx_l2_topk_grouped")
        idx[order_d] = idx_s
        dist[order_d] = dist_s
        if gt_pos is not None:
            gt_pos[order_d] = pos_s
            if bool((gt_h < 0).any()):
                gt_pos.masked_fill_(gt_h.to(self.device) < 0, -1)
        return idx, dist, gt_pos


def _group_panels(sorted_groups: torch.Tensor, offsets: torch.Tensor, chunk: int):
    """The panel table of ofx_l2_topk_grouped for queries sorted by group, cut into calls of `chunk` queries (host int64 tensors in).
    A panel is a run of queries of ONE group inside ONE call, at most 128 long: (q_lo, q_hi) relative to its call's first query, and
    the group's pool rows (p_lo, p_hi).  -> (int32 [n_panels, 4], [(first query, end query, first panel, number of panels) per call])."""
    nq, G = sorted_groups.numel(), offsets.numel() - 1
    cnt = torch.bincount(sorted_groups, minlength=G)
    start = torch.cumsum(cnt, 0) - cnt
    cuts = [torch.arange(s, s + n, 128) for s, n in zip(start.tolist(), cnt.tolist()) if n]
    calls = torch.arange(0, nq, chunk)
    lo = torch.unique(torch.cat(cuts + [calls]))                  # sorted: every panel's first query
    hi = torch.cat([lo[1:], torch.tensor([nq])])
    g = sorted_groups[lo]
    base = lo // chunk * chunk
    table = torch.stack([lo - base, hi - base, offsets[g], offsets[g + 1]], 1).to(torch.int32)
    first = torch.searchsorted(lo, calls).tolist() + [lo.numel()]
    return table, [(c0, min(c0 + chunk, nq), first[i], first[i + 1] - first[i]) for i, c0 in enumerate(calls.tolist())]


def fitb_argmin(y_hat: torch.Tensor, cand: torch.Tensor, return_dist: bool = False):
    """torch.cdist(y[B,1,D], cand[B,C,D]).squeeze(1).argmin(-1) on the GPU, fp32, first minimum."""
    lib = L.load()
    dev = y_hat.device
    if dev.type != "cuda":
        raise L.OfxError("fitb_argmin needs HIP tensors; there is no CPU path")
    y = _f32c(y_hat, dev); c = _f32c(cand, dev)
    B, Cn, D = c.shape
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    dist = torch.empty(B, Cn, dtype=torch.float32, device=dev) if return_dist else None
    with torch.cuda.device(dev):
        L.check(lib.ofx_fitb_argmin(_ptr(y), _ptr(c), B, Cn, D, _ptr(idx), _ptr(dist), _stream(dev)), "ofx_fitb_argmin")
    return (idx, dist) if return_dist else idx


def fitb_argmin_indexed(table: torch.Tensor, cand_index: torch.Tensor, y_hat: torch.Tensor, answer: Optional[torch.Tensor] = None,
                        n_correct: Optional[torch.Tensor] = None, return_dist: bool = False):
    """fitb_argmin with cand[b, c] = table[cand_index[b, c]] read straight from the table (ofx_fitb_argmin_indexed): no [B, C, D] tensor is
    gathered; same bits as fitb_argmin on the gathered rows.
    table [n, ld] fp32 on y_hat's device with unit column stride: a column slice of a wider table is taken as it is (ld = its row stride,
    ld % 4 == 0, first element 16-byte aligned).  A table in any other layout is refused (ValueError), never copied: a copy per call
    would move the whole table for every batch.
    cand_index [B, C] integer; y_hat [B, D], D <= ld: a row's first D floats are used.
    answer [B] integer with n_correct, a 1-element int32 tensor on y_hat's device, both or neither: the call adds the number of questions
    with idx == answer to n_correct in place (zero it first; nothing waits for the device).
    A cand_index on the host is range-checked here (IndexError); one on the device is trusted - the kernel clamps it into the table.
    -> idx [B] int64 (, dist [B, C])."""
    lib = L.load()
    dev = y_hat.device
    if dev.type != "cuda":
        raise L.OfxError("fitb_argmin_indexed needs HIP tensors; there is no CPU path")
    if table.dim() != 2 or y_hat.dim() != 2 or cand_index.dim() != 2 or cand_index.shape[0] != y_hat.shape[0] or table.shape[1] < y_hat.shape[1]:
        raise ValueError(f"fitb_argmin_indexed: table {tuple(table.shape)}, cand_index {tuple(cand_index.shape)}, y_hat {tuple(y_hat.shape)} "
                         "are not [n,>=D], [B,C], [B,D]")
    if (answer is None) != (n_correct is None):
        raise ValueError("fitb_argmin_indexed: answer and n_correct go together")
    B, D = y_hat.shape
    Cn = cand_index.shape[1]
    if cand_index.device.type == "cpu" and cand_index.numel():
        lo, hi = int(cand_index.min()), int(cand_index.max())
        if lo < 0 or hi >= table.shape[0]:
            raise IndexError(f"cand_index out of range [0, {table.shape[0]}): min {lo}, max {hi}")
    tb = table.detach()
    # the table is read in place or not at all: a private fp32 copy per call would move the whole table for every batch
    if (tb.device != dev or tb.dtype != torch.float32 or tb.stride(1) != 1 or tb.stride(0) < tb.shape[1] or tb.stride(0) % 4
            or tb.data_ptr() % 16):
        raise ValueError(f"fitb_argmin_indexed: the table must be fp32 on {dev} with unit column stride, a row stride that is a multiple of 4 "
                         f"floats and a 16-byte aligned first element (a column slice must start at a multiple of 4 columns); got "
                         f"{tb.dtype} on {tb.device}, strides {tuple(tb.stride())}, offset {tb.data_ptr() % 16} bytes past alignment")
    y = _f32c(y_hat.detach(), dev)
    ci = cand_index.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    ans = None
    if answer is not None:
        if answer.numel() != B:
            raise ValueError(f"fitb_argmin_indexed: answer holds {answer.numel()} entries, the batch {B} questions")
        if n_correct.device != dev or n_correct.dtype != torch.int32 or n_correct.numel() != 1:
            raise ValueError(f"fitb_argmin_indexed: n_correct must be a 1-element int32 tensor on {dev}")
        ans = answer.reshape(-1).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    dist = torch.empty(B, Cn, dtype=torch.float32, device=dev) if return_dist else None
    with torch.cuda.device(dev):
        L.check(lib.ofx_fitb_argmin_indexed(_ptr(tb), tb.stride(0), tb.shape[0], _ptr(ci), _ptr(y), B, Cn, D, _ptr(ans), _ptr(idx), _ptr(dist),
                                            _ptr(n_correct), _stream(dev)), "ofx_fitb_argmin_indexed")
    return (idx, dist) if return_dist else idx


def dropout_mask(p: float, seed: int, site: int, rows: int, cols: int, device) -> torch.Tensor:
    """keep-mask / (1 - p) of one dropout site exactly as the training kernels compute it (test aid)."""
    lib = L.load()
    out = torch.empty(rows, cols, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        L.check(lib.ofx_dropout_mask(float(p), int(seed) & 0xFFFFFFFF, site, rows, cols, _ptr(out), _stream(out.device)), "ofx_dropout_mask")
    return out


FOCAL_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def focal_loss(logits: torch.Tensor, labels: torch.Tensor, alpha: float, gamma: float, upstream: float = 1.0, need_grad: bool = True,
               reduction: str = "mean"):
    """FocalLoss(alpha, gamma, reduction) (src/losses/focal_loss.py:23-41) and upstream * d loss / d logits, one kernel.
    'mean' / 'sum' return a 0-d loss; 'none' returns the [B] unreduced losses (dlogits is then the per-element derivative)."""
    lib = L.load()
    dev = logits.device
    if dev.type != "cuda":
        raise L.OfxError("focal_loss needs HIP tensors; there is no CPU path")
    y = _f32c(logits.reshape(-1), dev); t = _f32c(labels.reshape(-1), dev)
    red = FOCAL_REDUCTIONS[reduction]
    loss = torch.empty((), dtype=torch.float32, device=dev)
    per = torch.empty_like(y) if red == 0 else None
    dl = torch.empty_like(y) if need_grad else None
    with torch.cuda.device(dev):
        L.check(lib.ofx_focal_loss_ex(_ptr(y), _ptr(t), y.numel(), float(alpha), float(gamma), float(upstream), red, _ptr(loss), _ptr(per),
                                      _ptr(dl), _stream(dev)), "ofx_focal_loss_ex")
    return (per if red == 0 else loss), dl


def set_rank_loss(y: torch.Tensor, y_hat: torch.Tensor, neg: torch.Tensor, neg_mask: Optional[torch.Tensor], margin: float,
                  upstream: float = 1.0, need_grad: bool = True):
    """SetWiseRankingLoss(margin) (src/losses/set_wise_ranking_loss.py:15-36) and upstream * d loss / d y_hat from one pass over the
    negatives (ofx_set_rank_loss).  y, y_hat [B, D]; neg [B, K, D]; neg_mask [B, K], True / non-zero = padded (None: nothing padded).
    -> (0-d loss, dy_hat [B, D] or None)."""
    lib = L.load()
    dev = y_hat.device
    if dev.type != "cuda":
        raise L.OfxError("set_rank_loss needs HIP tensors; the torch expression in losses.SetWiseRankingLoss is the CPU path")
    if y_hat.dim() != 2 or neg.dim() != 3 or y.shape != y_hat.shape or neg.shape[0] != y_hat.shape[0] or neg.shape[2] != y_hat.shape[1]:
        raise ValueError(f"set_rank_loss: y {tuple(y.shape)}, y_hat {tuple(y_hat.shape)}, neg {tuple(neg.shape)} are not [B,D], [B,D], [B,K,D]")
    B, D = y_hat.shape
    K = neg.shape[1]
    yc, hc, nc = _f32c(y.detach(), dev), _f32c(y_hat.detach(), dev), _f32c(neg.detach(), dev)
    mk = None
    if neg_mask is not None:
        if tuple(neg_mask.shape) != (B, K):
            raise ValueError(f"set_rank_loss: neg_mask {tuple(neg_mask.shape)} is not [B,K] = {(B, K)}")
        mk = neg_mask.to(dev)
        mk = (mk if mk.dtype in (torch.bool, torch.uint8) else mk != 0).contiguous().view(torch.uint8)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dy = torch.empty_like(hc) if need_grad else None
    n_ws = lib.ofx_set_rank_loss_ws_bytes(B, K, D)
    ws = torch.empty(max(n_ws, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.ofx_set_rank_loss(_ptr(yc), _ptr(hc), _ptr(nc) if K else None, _ptr(mk) if K else None, B, K, D, float(margin), float(upstream),
                                      _ptr(loss), _ptr(dy), None, None, _ptr(ws), ws.numel(), _stream(dev)), "ofx_set_rank_loss")
    return loss, dy


def set_rank_loss_indexed(table: torch.Tensor, pos_index: torch.Tensor, neg_index: torch.Tensor, y_hat: torch.Tensor, margin: float,
                          upstream: float = 1.0, need_grad: bool = True, n_table: Optional[int] = None):
    """set_rank_loss with y[b] = table[pos_index[b]] and neg[b, k] = table[neg_index[b, k]] read straight from the table
    (ofx_set_rank_loss_indexed): no [B, D] / [B, K, D] tensor is gathered.  table [n, ld] fp32 with unit column stride (a column slice of
    a wider table is taken as it is, ld = its row stride; ld % 4 == 0); pos_index [B], neg_index [B, K] integer, a negative neg_index =
    padded; y_hat [B, D], D <= ld: a row's first D floats are used.  n_table (default: all rows) is the row count the kernel clamps the
    indices to.  Same bits as set_rank_loss on the gathered rows.  -> (0-d loss, dy_hat [B, D] or None)."""
    lib = L.load()
    dev = y_hat.device
    if dev.type != "cuda":
        raise L.OfxError("set_rank_loss_indexed needs HIP tensors; losses.SetWiseRankingLoss.forward_indexed gathers on the CPU")
    if (table.dim() != 2 or y_hat.dim() != 2 or pos_index.dim() != 1 or neg_index.dim() != 2 or pos_index.shape[0] != y_hat.shape[0]
            or neg_index.shape[0] != y_hat.shape[0] or table.shape[1] < y_hat.shape[1]):
        raise ValueError(f"set_rank_loss_indexed: table {tuple(table.shape)}, pos_index {tuple(pos_index.shape)}, neg_index "
                         f"{tuple(neg_index.shape)}, y_hat {tuple(y_hat.shape)} are not [n,>=D], [B], [B,K], [B,D]")
    B, D = y_hat.shape
    K = neg_index.shape[1]
    tb = table.detach()
    if tb.device != dev or tb.dtype != torch.float32 or tb.stride(1) != 1 or tb.stride(0) < tb.shape[1] or tb.stride(0) % 4:
        tb = _f32c(tb, dev)                            # not the layout the kernel reads in place: a private copy
    ld = tb.stride(0)
    hc = _f32c(y_hat.detach(), dev)
    pi = pos_index.to(device=dev, dtype=torch.int32).contiguous()
    ni = neg_index.to(device=dev, dtype=torch.int32).contiguous()
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dy = torch.empty_like(hc) if need_grad else None
    n_ws = lib.ofx_set_rank_loss_ws_bytes(B, K, D)
    ws = torch.empty(max(n_ws, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.ofx_set_rank_loss_indexed(_ptr(tb), ld, tb.shape[0] if n_table is None else int(n_table), _ptr(pi), _ptr(ni) if K else None,
                                              _ptr(hc), B, K, D, float(margin), float(upstream), _ptr(loss), _ptr(dy), None, None, _ptr(ws),
                                              ws.numel(), _stream(dev)), "ofx_set_rank_loss_indexed")
    return loss, dy


ADAMW_WG_FLOATS = 4096      # arena floats one workgroup of ofx_adamw_step covers per stride step (optim.hip OPT_WG_FLOATS); grid = min(ceil(n / this), 2048)


def adamw_step_ws_bytes(n_arena: int) -> int:
    return int(L.load().ofx_adamw_step_ws_bytes(int(n_arena)))


def adamw_step(segments: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor,
               lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, max_norm: float, grad_scale: float,
               grad_norm: torch.Tensor, skipped: torch.Tensor, ws: Optional[torch.Tensor] = None) -> None:
    """clip_grad_norm_(max_norm) -> AdamW -> zero over a flat gradient arena, two launches on the current stream (ofx_adamw_step; semantics
    in include/ofx.h).  segments: int64 [n, 3] DEVICE rows (param data_ptr, arena offset, numel), sorted by offset (`optim.segment_table`);
    grad / exp_avg / exp_avg_sq: fp32 arenas of the same length (a multiple of 64); step, grad_norm: 1-element fp32, skipped: 1-element
    int32, all on the arena's device; ws: uint8 workspace of adamw_step_ws_bytes(n) (allocated when None).  Everything is updated in
    place; nothing is returned and nothing waits."""
    lib = L.load()
    dev = grad.device
    if dev.type != "cuda":
        raise L.OfxError("adamw_step needs HIP tensors; there is no CPU path")
    for name, t, dt in (("segments", segments, torch.int64), ("grad", grad, torch.float32), ("exp_avg", exp_avg, torch.float32),
                        ("exp_avg_sq", exp_avg_sq, torch.float32), ("step", step, torch.float32), ("grad_norm", grad_norm, torch.float32),
                        ("skipped", skipped, torch.int32)):
        if t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"adamw_step: {name} must be a contiguous {dt} tensor on {dev}")
    n = grad.numel()
    if segments.dim() != 2 or segments.shape[1] != 3 or exp_avg.numel() != n or exp_avg_sq.numel() != n:
        raise ValueError(f"adamw_step: segments {tuple(segments.shape)} is not [n, 3], or the arenas differ in length")
    if ws is None:
        ws = torch.empty(max(lib.ofx_adamw_step_ws_bytes(n), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.ofx_adamw_step(_ptr(segments), segments.shape[0], _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, _ptr(step), float(lr),
                                   float(beta1), float(beta2), float(eps), float(weight_decay), float(max_norm), float(grad_scale),
                                   _ptr(grad_norm), _ptr(skipped), _ptr(ws), ws.numel(), _stream(dev)), "ofx_adamw_step")


def adamw_step_scaled(segments: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: torch.Tensor,
                      lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, max_norm: float, grad_scale: float,
                      loss_scale: torch.Tensor, growth_tracker: torch.Tensor, growth_factor: float, backoff_factor: float, growth_interval: int,
                      grad_norm: torch.Tensor, skipped: torch.Tensor, ws: Optional[torch.Tensor] = None) -> None:
    """adamw_step on an arena that holds loss_scale x the gradient, with torch.amp.GradScaler's unscale_ before it and its update() after
    it, still two launches (ofx_adamw_step_scaled; semantics in include/ofx.h).  loss_scale: 1-element fp32, growth_tracker: 1-element
    int32, both on the arena's device, both read and rewritten; grad_norm receives the UNSCALED norm.  The other arguments are
    adamw_step's."""
    lib = L.load()
    dev = grad.device
    if dev.type != "cuda":
        raise L.OfxError("adamw_step_scaled needs HIP tensors; there is no CPU path")
    for name, t, dt in (("segments", segments, torch.int64), ("grad", grad, torch.float32), ("exp_avg", exp_avg, torch.float32),
                        ("exp_avg_sq", exp_avg_sq, torch.float32), ("step", step, torch.float32), ("loss_scale", loss_scale, torch.float32),
                        ("growth_tracker", growth_tracker, torch.int32), ("grad_norm", grad_norm, torch.float32), ("skipped", skipped, torch.int32)):
        if t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"adamw_step_scaled: {name} must be a contiguous {dt} tensor on {dev}")
    n = grad.numel()
    if segments.dim() != 2 or segments.shape[1] != 3 or exp_avg.numel() != n or exp_avg_sq.numel() != n:
        raise ValueError(f"adamw_step_scaled: segments {tuple(segments.shape)} is not [n, 3], or the arenas differ in length")
    if ws is None:
        ws = torch.empty(max(lib.ofx_adamw_step_ws_bytes(n), 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.ofx_adamw_step_scaled(_ptr(segments), segments.shape[0], _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, _ptr(step), float(lr),
                                          float(beta1), float(beta2), float(eps), float(weight_decay), float(max_norm), float(grad_scale),
                                          _ptr(loss_scale), _ptr(growth_tracker), float(growth_factor), float(backoff_factor), int(growth_interval),
                                          _ptr(grad_norm), _ptr(skipped), _ptr(ws), ws.numel(), _stream(dev)), "ofx_adamw_step_scaled")


def topk_merge(idx_parts: torch.Tensor, dist_parts: torch.Tensor):
    """[parts,nq,k] per-shard candidates (global indices) -> ([nq,k] idx, [nq,k] dist), ascending, ties -> smaller idx."""
    lib = L.load()
    dev = idx_parts.device
    parts, nq, k = idx_parts.shape
    ii = idx_parts.contiguous(); dd = dist_parts.contiguous()
    idx = torch.empty(nq, k, dtype=torch.int64, device=dev)
    dist = torch.empty(nq, k, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.ofx_topk_merge(_ptr(ii), _ptr(dd), parts, nq, k, _ptr(idx), _ptr(dist), _stream(dev)), "ofx_topk_merge")
    return idx, dist
