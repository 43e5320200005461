#!/usr/bin/env python3
"""Cost of the label-smoothed language loss (`--label_smoothing`, misc/utils.py:126-156) on one box: interleaved A/B rounds,
label_smoothing 0 against 0.1, of the training step as bench.py builds and steps it (LossWrapper, total loss, GradBucketReducer at world
size 1, FlatAdam at lr 0 with the fused zero_grad), for the headline Sub_GC_Kar fp32 B=128, Full_GC_Kar bf16 B=256 and Flickr bf16 B=64.

    python tools/label_smoothing_cost.py [--configs kar,full_gc_kar,flickr] [--rounds 5] [--steps 10] [--warmup 3] [--smoothing 0.1]

Both criteria run on ONE model and batch (two LossWrappers); each round times both back to back, alternating which goes first, and a
switch is followed by its own warm-up steps.  By the byte counts the smoothed step reads and writes what the plain one does plus one
scalar per logits row, so the expectation is a difference inside the round-to-round spread; nothing is asserted.  Prints one text table
per config and a final JSON line (median ms per step of each criterion, the relative cost and every round's numbers)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]
import torch  # noqa: E402

import bench  # noqa: E402
from subgc import _lib, ops, parallel, synthetic  # noqa: E402
import subgc.models as models  # noqa: E402


def build(name, dev, smoothing):
    cfg = bench.CONFIGS[name]
    torch.manual_seed(1234)
    model = models.setup(argparse.Namespace(**cfg["opt"])).to(dev).train()
    lws = {"nll": models.LossWrapper(model, None), "smooth": models.LossWrapper(model, argparse.Namespace(label_smoothing=smoothing))}
    batch = {k: v.to(dev) for k, v in synthetic.make_train_batch(cfg["batch"], seed=1000, **cfg["data"]).items()}
    adam = parallel.FlatAdam(model, lr=0.0)
    red = parallel.GradBucketReducer(model, optimizer=adam)
    one = ops.fill_(torch.empty((), device=dev, dtype=torch.float32), 1.0)

    def step(mode):
        red.prepare()
        out = lws[mode](*bench.lw_args(batch))
        models.total_loss(out).backward(one)
        red.finish(average=False)
        adam.step(grad_scale=1.0, zero_grad=True)
        return out

    return step, cfg["batch"]


def timed(step, mode, steps, warmup):
    for _ in range(warmup):
        step(mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(mode)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="kar,full_gc_kar,flickr")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--smoothing", type=float, default=0.1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "label_smoothing_cost.py measures the MI355X"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.lib()
    res = {}
    for name in a.configs.split(","):
        step, B = build(name, dev, a.smoothing)
        rows = {"nll": [], "smooth": []}
        for r in range(a.rounds):
            for mode in (("nll", "smooth") if r % 2 == 0 else ("smooth", "nll")):
                rows[mode].append(timed(step, mode, a.steps, a.warmup))
        losses = {mode: float(step(mode)["lang_loss"].detach()) for mode in rows}
        med = {k: statistics.median(v) for k, v in rows.items()}
        rel = med["smooth"] / med["nll"] - 1.0
        res[name] = {"images": B, "steps": a.steps, "smoothing": a.smoothing, "rounds": {k: [round(x, 3) for x in v] for k, v in rows.items()},
                     "median_ms": {k: round(v, 3) for k, v in med.items()}, "cost_pct": round(100 * rel, 2),
                     "lang_loss": {k: round(v, 5) for k, v in losses.items()}}
        print(f"{name} (B={B}, {a.steps} timed steps per round, {a.warmup} warm-up steps after every switch, smoothing {a.smoothing})")
        for mode, v in rows.items():
            print(f"  {mode:6s}: " + " ".join(f"{x:8.3f}" for x in v) + f"   median {med[mode]:8.3f} ms/step  spread {max(v) - min(v):.3f}"
                  f"   lang_loss {losses[mode]:.5f}")
        print(f"  label smoothing: {100 * rel:+.2f} % per step")
        del step
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
