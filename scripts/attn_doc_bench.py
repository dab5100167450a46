"""Timing of document-masked flash attention at the Llama-3-8B shape (B 2, S 8192, 32 q / 8 kv heads,
head dim 128, causal) for several document layouts, beside the default path without bounds.

The layouts are timed alternately, ``--runs`` rounds of ``--iters`` timed iterations each (HIP events,
after a warm-up); one JSON line per round.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from easydl_amd.ops.attention import flash_attention, segment_bounds  # noqa: E402
from easydl_amd.trainer.data import PackedTokens  # noqa: E402


def layouts(B, S):
    """name -> document lengths per batch row (None: the default path, no bounds)."""
    packed = PackedTokens(vocab=128, seq=S, mean_doc_len=1024)
    return {
        "default (no bounds)": None,
        "1 x %d" % S: [[S]] * B,
        "2 x %d" % (S // 2): [[S // 2] * 2] * B,
        "8 x %d" % (S // 8): [[S // 8] * 8] * B,
        "PackedTokens mean 1024": [packed.doc_lengths(i) for i in range(B)],
    }


def bounds_of(rows, dev):
    if rows is None:
        return None
    seg = torch.stack([torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r)) for r in rows])
    return segment_bounds(seg.to(dev))


def time_layout(q, k, v, do, bounds, iters):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    for _ in range(iters):
        flash_attention(q, k, v, bounds=bounds)
    e[1].record()
    for _ in range(iters):
        flash_attention(q, k, v, bounds=bounds).backward(do)
    e[2].record()
    torch.cuda.synchronize()
    return round(e[0].elapsed_time(e[1]) / iters, 3), round(e[1].elapsed_time(e[2]) / iters, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    B, S, H, KV = a.batch, a.seq, 32, 8
    dev = torch.device("cuda", 0)
    q, k, v = (torch.randn(B, S, n, 128, device=dev, dtype=torch.bfloat16).transpose(1, 2).requires_grad_()
               for n in (H, KV, KV))
    do = torch.randn(B, H, S, 128, device=dev, dtype=torch.bfloat16)
    lay = layouts(B, S)
    bounds = {n: bounds_of(r, dev) for n, r in lay.items()}
    for b in bounds.values():       # warm-up of every path
        for _ in range(2):
            flash_attention(q, k, v, bounds=b).backward(do)
    torch.cuda.synchronize()
    for run in range(a.runs):       # alternate the layouts inside every round
        row = {"run": run}
        for n, b in bounds.items():
            f, fb = time_layout(q, k, v, do, b, a.iters)
            row[n] = {"fwd_ms": f, "fwdbwd_ms": fb}
        print(json.dumps(row), flush=True)
    docs = {n: (None if r is None else [len(x) for x in r]) for n, r in lay.items()}
    print(json.dumps({"documents_per_row": docs}))


if __name__ == "__main__":
    main()
