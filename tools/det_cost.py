#!/usr/bin/env python3
"""Cost of the deterministic mode (ops.deterministic / subgc_deterministic) on one box: interleaved A/B rounds, mode off against mode
on, of the training step as bench.py builds and steps it (LossWrapper, total loss, GradBucketReducer at world size 1, FlatAdam at lr 0
with the fused zero_grad), for the headline Sub_GC_Kar fp32 B=128, Full_GC_Kar bf16 B=256 and Flickr bf16 B=64.

    python tools/det_cost.py [--configs kar,full_gc_kar,flickr] [--rounds 5] [--steps 10] [--warmup 3]
    python tools/det_cost.py --only on --configs kar --rounds 1     # one mode only (the rocprofv3 --kernel-trace --stats runs)

Each round times both modes back to back, alternating which goes first; a mode switch is followed by its own warm-up steps.  Prints
one text table per config and a final JSON line (median ms per step of each mode, the relative cost and every round's numbers)."""
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


def build(name, dev):
    cfg = bench.CONFIGS[name]
    torch.manual_seed(1234)
    model = models.setup(argparse.Namespace(**cfg["opt"])).to(dev).train()
    lw = models.LossWrapper(model, None)
    batch = {k: v.to(dev) for k, v in synthetic.make_train_batch(cfg["batch"], seed=1000, **cfg["data"]).items()}
    adam = parallel.FlatAdam(model, lr=0.0)
    red = parallel.GradBucketReducer(model, optimizer=adam)
    one = ops.fill_(torch.empty((), device=dev, dtype=torch.float32), 1.0)

    def step():
        red.prepare()
        out = lw(*bench.lw_args(batch))
        models.total_loss(out).backward(one)
        red.finish(average=False)
        adam.step(grad_scale=1.0, zero_grad=True)
        return out

    return step, cfg["batch"]


def timed(step, on, steps, warmup):
    ops.set_deterministic(on)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="kar,full_gc_kar,flickr")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("on", "off"), help="time one mode only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "det_cost.py measures the MI355X"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.lib()
    res = {}
    for name in a.configs.split(","):
        step, B = build(name, dev)
        rows = {"off": [], "on": []}
        for r in range(a.rounds):
            order = [a.only] if a.only else (("off", "on") if r % 2 == 0 else ("on", "off"))
            for mode in order:
                rows[mode].append(timed(step, mode == "on", a.steps, a.warmup))
        ops.set_deterministic(False)
        med = {k: statistics.median(v) for k, v in rows.items() if v}
        res[name] = {"images": B, "steps": a.steps, "rounds": {k: [round(x, 3) for x in v] for k, v in rows.items() if v},
                     "median_ms": {k: round(v, 3) for k, v in med.items()}}
        print(f"{name} (B={B}, {a.steps} timed steps per round, {a.warmup} warm-up steps after every switch)")
        for mode, v in rows.items():
            if v:
                print(f"  mode {mode:3s}: " + " ".join(f"{x:8.3f}" for x in v) + f"   median {med[mode]:8.3f} ms/step  spread {max(v) - min(v):.3f}")
        if len(med) == 2:
            rel = med["on"] / med["off"] - 1.0
            res[name]["cost_pct"] = round(100 * rel, 2)
            print(f"  deterministic mode: {100 * rel:+.2f} % per step")
        del step
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
