#!/usr/bin/env python3
"""The MFMA attention op alone: S = 197 (attention_mfma_long_kernel, ViT-B/16) beside S = 50 (attention_mfma_kernel, ViT-B/32) in one run -
256 sequences x 12 heads, both operand types, ofx_attention on unit-normal q | k | v, median of device-event-timed calls taken in
alternation, next to the time its bytes take once at 6.3 TB/s (rows x 3W x 2 B read + rows x W x 2 B written; the HBM rate of the
project's other byte floors).  Prints one JSON line per operand type.   python tools/attn_long_bench.py [nseq]"""
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outfitx_amd import _lib as L

HBM = 6.3e12
lib = L.load()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
H, W = 12, 768
s = torch.cuda.current_stream().cuda_stream
for name, code, td in (("bf16", 1, torch.bfloat16), ("f16", 2, torch.float16)):
    calls, floor = {}, {}
    for S in (50, 197):
        qkv = torch.randn(n * S, 3 * W, device="cuda").to(td)
        out = torch.empty(n * S, W, dtype=td, device="cuda")
        calls[S] = (lambda S=S, qkv=qkv, out=out: L.check(lib.ofx_attention(qkv.data_ptr(), out.data_ptr(), None, n, S, H, 3 * W, W, W, 2 * W, 0, 0, 0.125, code, s)))
        floor[S] = n * S * 4 * W * 2 / HBM * 1e6
    for _ in range(5):
        for f in calls.values(): f()
    torch.cuda.synchronize()
    ev = {S: [] for S in calls}
    for _ in range(50):
        for S, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record()
            ev[S].append((a, b))
    torch.cuda.synchronize()
    med = {S: float(np.median([a.elapsed_time(b) for a, b in ev[S]])) * 1e3 for S in ev}
    print(json.dumps({"op": "ofx_attention", "dtype": name, "nseq": n, "heads": H,
                      **{f"S{S}": {"us": round(med[S], 1), "byte_floor_us": round(floor[S], 1), "ratio_to_floor": round(med[S] / floor[S], 2),
                                   "us_per_1k_rows": round(med[S] / (n * S) * 1e3, 2)} for S in med}}), flush=True)
