#!/usr/bin/env python3
"""Cost of the one-pass self-critical step (`LossWrapper(..., sc_samples=n)`, n >= 2: n samples per caption row drawn inside the decoder
Function's forward, leave-one-out baseline) against the two-pass step (n = 1: rollout with a greedy half, then the replay) on one box:
interleaved rounds of the training step as bench.py builds and steps it (LossWrapper, total loss, GradBucketReducer at world size 1,
FlatAdam at lr 0 with the fused zero_grad), for the headline Sub_GC_Kar fp32 B=128, Full_GC_Kar bf16 B=256 and Flickr bf16 B=64.

    python tools/sc_samples_cost.py [--configs kar,full_gc_kar,flickr] [--samples 1,2,5] [--rounds 5] [--steps 10] [--warmup 3]

All legs run on ONE model and batch (one LossWrapper per n); each round times every leg once, the order rotating from round to round, and
every switch is followed by its own warm-up steps.  Reported per leg: the median ms per step over the rounds, the spread (max - min), the
ms per GRADIENT-CARRYING CAPTION (step / (n * b5): the two-pass step differentiates b5 sampled captions, its greedy half carries none),
the peak device memory, and from a few more steps bracketed by device synchronisations the decoder Function's forward alone (prepare, the
sampling loop, the reward, the criterion) and the ATen device kernels (every one timed between synchronisations under a
TorchDispatchMode, so their share is an upper bound; their names are listed).  The yardstick is the n = 1 leg of the same run; the
verdict line says whether a caption at n = 2 costs less than one at n = 1 by more than the two legs' spreads together.  Nothing is
asserted.  Prints one text table per config and a final JSON line."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

import bench  # noqa: E402
from subgc import _lib, functions as F_, ops, parallel, selfcritical, synthetic  # noqa: E402
import subgc.models as models  # noqa: E402

HARMLESS = ("view", "reshape", "empty", "as_strided", "detach", "alias", "slice", "select", "transpose", "permute", "expand", "unsqueeze",
            "squeeze", "_unsafe_view", "t.default", "unbind", "split", "narrow", "pin_memory", "is_pinned", "record_stream", "_reshape_alias",
            "lift_fresh", "unfold", "chunk", "set_", "resize_", "stride", "sym_", "is_same_size", "_local_scalar_dense")


class TimedAten(TorchDispatchMode):
    """Every ATen op that launches a device kernel, run between two synchronisations (tests/test_no_aten_gpu.py's notion of such an op)."""

    def __init__(self):
        super().__init__()
        self.ms, self.count = 0.0, collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        ts = [t for t in args if torch.is_tensor(t)]
        watched = not any(h in name for h in HARMLESS) and any(t.is_cuda for t in ts) and not (
            ("copy_" in name or "_to_copy" in name) and any(not t.is_cuda for t in ts))
        if not watched:
            return func(*args, **(kwargs or {}))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = func(*args, **(kwargs or {}))
        torch.cuda.synchronize()
        self.ms += 1e3 * (time.perf_counter() - t0)
        self.count[name] += 1
        return r


def build(name, dev, samples):
    cfg = bench.CONFIGS[name]
    B = cfg["batch"]
    torch.manual_seed(1234)
    model = models.setup(argparse.Namespace(**cfg["opt"])).to(dev).train()
    batch = {k: v.to(dev) for k, v in synthetic.make_train_batch(B, seed=1000, **cfg["data"]).items()}
    W = batch["labels"].size(1) - 2
    rng = np.random.default_rng(7)
    refs = [rng.integers(1, model.vocab_size + 1, (5, W)) * (np.arange(W) < rng.integers(4, W + 1, (5, 1))) for _ in range(B)]
    reward = selfcritical.SelfCriticalReward(selfcritical.RewardReferences(refs, vocab_size=model.vocab_size), 1.0, 0.0)
    lws = {n: models.LossWrapper(model, None, sc_reward=reward, sc_samples=n) for n in samples}
    args = list(bench.lw_args(batch))
    args[6] = torch.arange(B, device=dev, dtype=torch.int32)
    adam = parallel.FlatAdam(model, lr=0.0)
    red = parallel.GradBucketReducer(model, optimizer=adam)
    one = ops.fill_(torch.empty((), device=dev, dtype=torch.float32), 1.0)

    def step(n):
        red.prepare()
        out = lws[n](*args, sc_flag=True)
        models.total_loss(out).backward(one)
        red.finish(average=False)
        adam.step(grad_scale=1.0, zero_grad=True)
        return out

    return step, B, batch["labels"].size(0)


def timed(step, n, steps, warmup):
    for _ in range(warmup):
        step(n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(n)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def bracketed(step, n, steps):
    """-> (decoder forward ms, whole step ms) per step, the decoder Function's forward bracketed by synchronisations (for n = 1 that is
    the replay's forward; the rollout before it is bracketed as well and added)."""
    spent = [0.0]

    def bracket(fn):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            spent[0] += 1e3 * (time.perf_counter() - t0)
            return r
        return run

    from subgc import functions_packed as FP
    saved = [(F_.DecoderFn, "forward", F_.DecoderFn.__dict__["forward"]), (FP.PackedDecoderLossFn, "forward", FP.PackedDecoderLossFn.__dict__["forward"]),
             (selfcritical, "rollout", selfcritical.rollout)]
    for obj, attr, fn in saved:
        raw = fn.__func__ if isinstance(fn, staticmethod) else fn
        setattr(obj, attr, staticmethod(bracket(raw)) if isinstance(fn, staticmethod) else bracket(raw))
    try:
        step(n)
        spent[0] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(n)
        torch.cuda.synchronize()
        whole = 1e3 * (time.perf_counter() - t0) / steps
    finally:
        for obj, attr, fn in saved:
            setattr(obj, attr, fn)
    return spent[0] / steps, whole


def aten(step, n):
    step(n)
    torch.cuda.synchronize()
    with TimedAten() as w:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(n)
        torch.cuda.synchronize()
        whole = 1e3 * (time.perf_counter() - t0)
    return w.ms, whole, dict(w.count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="kar,full_gc_kar,flickr")
    ap.add_argument("--samples", default="1,2,5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sc_samples_cost.py measures the MI355X"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.lib()
    samples = [int(x) for x in a.samples.split(",")]
    res = {}
    for name in a.configs.split(","):
        step, B, b5 = build(name, dev, samples)
        rows, peak = {n: [] for n in samples}, {}
        for n in samples:                                   # peak memory of each leg on its own, before the timed rounds
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            step(n)
            torch.cuda.synchronize()
            peak[n] = torch.cuda.max_memory_allocated() / 2 ** 30
        for r in range(a.rounds):
            for n in samples[r % len(samples):] + samples[:r % len(samples)]:
                rows[n].append(timed(step, n, a.steps, a.warmup))
        med = {n: statistics.median(v) for n, v in rows.items()}
        spread = {n: max(v) - min(v) for n, v in rows.items()}
        cap = {n: med[n] / (n * b5) for n in samples}
        extra = {}
        for n in samples:
            fwd, whole = bracketed(step, n, max(3, a.steps // 2))
            a_ms, a_whole, names = aten(step, n)
            extra[n] = {"decoder_forward_ms": round(fwd, 3), "bracketed_step_ms": round(whole, 3), "aten_ms": round(a_ms, 3),
                        "aten_step_ms": round(a_whole, 3), "aten_kernels": names}
        res[name] = {"images": B, "caption_rows": b5, "steps": a.steps,
                     "legs": {str(n): {"rounds_ms": [round(x, 3) for x in rows[n]], "median_ms": round(med[n], 3), "spread_ms": round(spread[n], 3),
                                       "ms_per_caption": round(cap[n], 5), "spread_per_caption": round(spread[n] / (n * b5), 5),
                                       "peak_GiB": round(peak[n], 3), **extra[n]} for n in samples}}
        print(f"{name} (B={B}, b5={b5}, {a.steps} timed steps per round, {a.warmup} warm-up steps after every switch)")
        for n in samples:
            e = extra[n]
            print(f"  n={n:2d}: " + " ".join(f"{x:8.3f}" for x in rows[n]) + f"   median {med[n]:8.3f} ms/step  spread {spread[n]:.3f}   "
                  f"{1e3 * cap[n]:8.2f} us per gradient-carrying caption ({n * b5} of them)   peak {peak[n]:.2f} GiB")
            print(f"        decoder forward{' + rollout' if n == 1 else ''} {e['decoder_forward_ms']:.3f} of a bracketed step of {e['bracketed_step_ms']:.3f} ms; "
                  f"ATen device kernels {e['aten_ms']:.3f} of {e['aten_step_ms']:.3f} ms ({100 * e['aten_ms'] / e['aten_step_ms']:.1f} %, synchronised): "
                  + (", ".join(f"{k} x{v}" for k, v in sorted(e["aten_kernels"].items())) or "none"))
        if 1 in samples and 2 in samples:
            gain = cap[1] - cap[2]
            need = spread[1] / b5 + spread[2] / (2 * b5)
            res[name]["verdict_n2"] = {"gain_us": round(1e3 * gain, 3), "spreads_us": round(1e3 * need, 3), "holds": bool(gain > need)}
            print(f"  a caption at n=2 costs {1e3 * cap[2]:.2f} us against {1e3 * cap[1]:.2f} us at n=1: {1e3 * gain:+.2f} us, the two spreads together are "
                  f"{1e3 * need:.2f} us -> {'below the two-pass step by more than the spreads' if gain > need else 'NOT below by more than the spreads'}")
        del step
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
