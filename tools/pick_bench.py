"""Stand-alone timing of the sampling token choice: `subgc_decode_sample` (any the_k, nucleus the_p) beside `subgc_decode_pick` at
k = 3 and k = 8 (the kernel every k <= 8 keeps), on rows of 9488 fp32 logits.  The launches are replayed from one hipGraph (a Python
call costs more host time than the small kernels run); `--scale` is the spread of the logits (6: peaked like a trained captioner,
2: flat -- a nucleus then reaches far into the row).

    python tools/pick_bench.py [--reps 20] [--scale 6 2]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sub-gc_amd"))
from subgc import ops  # noqa: E402

V, T, TEMP = 9488, 20, 0.6
CASES = [("pick", 3, 1.0), ("pick", 8, 1.0)] + [("sample", k, 1.0) for k in (3, 8, 9, 20, 100, 1000, 9488)] + \
        [("sample", 9488, 0.9), ("sample", 9488, 0.5)]


def timed(fn, reps, dev):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g, dev):
        for _ in range(reps):
            fn()
    g.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(5):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps / 5


def run(n, scale, reps):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    logits = (torch.randn(n, V, generator=gen) * scale).to(dev)
    u = torch.rand(n, generator=gen).to(dev)
    seq, slp = torch.zeros(n, T, dtype=torch.long, device=dev), torch.zeros(n, T, device=dev)
    it, unf = torch.zeros(n, dtype=torch.long, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(T, dtype=torch.int32, device=dev)
    for kind, k, top_p in CASES:
        if kind == "pick":
            fn = lambda: ops.decode_pick(logits, k, TEMP, u, 0, seq, slp, it, unf, cnt[0:1], None, raw=True)
        else:
            fn = lambda: ops.decode_sample(logits, k, top_p, TEMP, u, 0, seq, slp, it, unf, cnt[0:1], None, raw=True)
        us = timed(fn, reps, dev)
        name = "subgc_decode_pick" if kind == "pick" else "subgc_decode_sample"
        print(f"rows {n:4d} scale {scale:g} {name:20s} k {k:5d} the_p {top_p:4.2f}: {us:8.1f} us / launch")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, nargs="+", default=[6.0, 2.0])
    a = ap.parse_args()
    for scale in a.scale:
        for n in (10, 900):
            run(n, scale, a.reps)
