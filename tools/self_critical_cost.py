#!/usr/bin/env python3
"""Cost of a self-critical training step (`LossWrapper(..., sc_flag=True)`, subgc/selfcritical.py) on one box: interleaved A/B rounds,
cross-entropy against SCST, of the training step as bench.py builds and steps it (LossWrapper, total loss, GradBucketReducer at world
size 1, FlatAdam at lr 0 with the fused zero_grad), for the headline Sub_GC_Kar fp32 B=128, Full_GC_Kar bf16 B=256 and Flickr bf16 B=64.

    python tools/self_critical_cost.py [--configs kar,full_gc_kar,flickr] [--rounds 5] [--steps 10] [--warmup 3]

Both objectives run on ONE model and batch (one LossWrapper, sc_flag off / on); each round times both back to back, alternating which goes
first, and a switch is followed by its own warm-up steps.  The references are seeded random captions (5 per image, 4-16 words): the reward's
cost depends on their count and length, not on their words.  The SCST step also rebuilds the decode-time weight snapshots every step (the
optimizer has moved the weights), as real training does.  After the rounds a few more SCST steps run with the rollout and the reward
bracketed by device synchronisations, which gives their shares of the step (the brackets themselves cost the overlap they remove, so the
shares are upper bounds); "replay + rest" is what remains: encoder, sGPN, the teacher-forced replay forward and backward, the optimizer.
Nothing is asserted.  Prints one text table per config and a final JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from subgc import _lib, ops, parallel, selfcritical, synthetic  # noqa: E402
import subgc.models as models  # noqa: E402


def build(name, dev):
    cfg = bench.CONFIGS[name]
    B = cfg["batch"]
    torch.manual_seed(1234)
    model = models.setup(argparse.Namespace(**cfg["opt"])).to(dev).train()
    batch = {k: v.to(dev) for k, v in synthetic.make_train_batch(B, seed=1000, **cfg["data"]).items()}
    W = batch["labels"].size(1) - 2
    rng = np.random.default_rng(7)
    refs = [rng.integers(1, model.vocab_size + 1, (5, W)) * (np.arange(W) < rng.integers(4, W + 1, (5, 1))) for _ in range(B)]
    reward = selfcritical.SelfCriticalReward(selfcritical.RewardReferences(refs, vocab_size=model.vocab_size), 1.0, 0.0)
    lw = models.LossWrapper(model, None, sc_reward=reward)
    args = list(bench.lw_args(batch))
    args[6] = torch.arange(B, device=dev, dtype=torch.int32)
    adam = parallel.FlatAdam(model, lr=0.0)
    red = parallel.GradBucketReducer(model, optimizer=adam)
    one = ops.fill_(torch.empty((), device=dev, dtype=torch.float32), 1.0)

    def step(mode):
        red.prepare()
        out = lw(*args, sc_flag=(mode == "scst"))
        models.total_loss(out).backward(one)
        red.finish(average=False)
        adam.step(grad_scale=1.0, zero_grad=True)
        return out

    return step, B, reward


def timed(step, mode, steps, warmup):
    for _ in range(warmup):
        step(mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(mode)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def shares(step, reward, steps):
    """-> (rollout ms, reward ms, whole step ms) of SCST steps whose rollout and reward are bracketed by synchronisations."""
    spent = {"rollout": 0.0, "reward": 0.0}

    def bracket(fn, key):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            spent[key] += 1e3 * (time.perf_counter() - t0)
            return r
        return run

    real_rollout, real_enqueue = selfcritical.rollout, reward.enqueue
    selfcritical.rollout, reward.enqueue = bracket(real_rollout, "rollout"), bracket(real_enqueue, "reward")
    try:
        step("scst")
        spent["rollout"] = spent["reward"] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step("scst")
        torch.cuda.synchronize()
        whole = 1e3 * (time.perf_counter() - t0) / steps
    finally:
        selfcritical.rollout, reward.enqueue = real_rollout, real_enqueue
    return spent["rollout"] / steps, spent["reward"] / steps, whole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="kar,full_gc_kar,flickr")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "self_critical_cost.py measures the MI355X"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.lib()
    res = {}
    for name in a.configs.split(","):
        step, B, reward = build(name, dev)
        rows = {"ce": [], "scst": []}
        for r in range(a.rounds):
            for mode in (("ce", "scst") if r % 2 == 0 else ("scst", "ce")):
                rows[mode].append(timed(step, mode, a.steps, a.warmup))
        out = step("scst")
        losses = {"ce": float(step("ce")["lang_loss"].detach()), "scst": float(out["lang_loss"].detach())}
        mean_reward = float(out["reward"])
        med = {k: statistics.median(v) for k, v in rows.items()}
        ratio = med["scst"] / med["ce"]
        t_roll, t_rew, t_whole = shares(step, reward, max(3, a.steps // 2))
        res[name] = {"images": B, "steps": a.steps, "rounds": {k: [round(x, 3) for x in v] for k, v in rows.items()},
                     "median_ms": {k: round(v, 3) for k, v in med.items()}, "scst_over_ce": round(ratio, 3),
                     "bracketed_ms": {"rollout": round(t_roll, 3), "reward": round(t_rew, 3), "replay_and_rest": round(t_whole - t_roll - t_rew, 3),
                                      "step": round(t_whole, 3)},
                     "lang_loss": {k: round(v, 5) for k, v in losses.items()}, "mean_reward": round(mean_reward, 6)}
        print(f"{name} (B={B}, {a.steps} timed steps per round, {a.warmup} warm-up steps after every switch)")
        for mode, v in rows.items():
            print(f"  {mode:5s}: " + " ".join(f"{x:8.3f}" for x in v) + f"   median {med[mode]:8.3f} ms/step  spread {max(v) - min(v):.3f}"
                  f"   lang_loss {losses[mode]:.5f}")
        print(f"  self-critical step: {ratio:.2f} x the cross-entropy step (mean reward {mean_reward:+.5f})")
        print(f"  bracketed SCST step {t_whole:.3f} ms: rollout {t_roll:.3f} ({100 * t_roll / t_whole:.0f} %), reward {t_rew:.3f} "
              f"({100 * t_rew / t_whole:.0f} %), replay + rest {t_whole - t_roll - t_rew:.3f} ({100 * (t_whole - t_roll - t_rew) / t_whole:.0f} %)")
        del step
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
