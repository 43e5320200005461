#!/usr/bin/env python3
"""Stand-alone timing of the fused clip + optimizer sweep (subgc_clip_optim_step) for every rule of subgc.optim.build_optimizer on a
BASELINE config's flat bucket (default Full_GC_Kar: 76.1 M parameters, bf16 weight snapshot written in the sweep), beside the Adam rule
over the whole bucket (no live table: what parallel.FlatAdam launches).  Interleaved rounds: every round times each sweep back to back.

    python tools/optim_bench.py [--config full_gc_kar] [--rounds 5] [--iters 20]

Bytes per live parameter (fp32 masters, states and gradient, + 2 B of bf16 snapshot when the config has one): Adam / AdamW read
p, g, m, v and write them back (32 B); SGD with momentum, RMSprop and Adagrad keep one state (24 B).  Parameters torch skips move
nothing (FlatAdam's sweep updates them too, so its count is the whole bucket).  Prints a table and a final JSON line with the median
time of each sweep and its rate (not the achievable-HBM share: the MI355X sustains about 6.3 of its 8 TB/s)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT]
import torch  # noqa: E402

import bench  # noqa: E402
from subgc import ops, optim  # noqa: E402
import subgc.models as models  # noqa: E402

RULES = ["adam", "adamw", "sgd", "sgdm", "sgdmom", "rmsprop", "adagrad"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="full_gc_kar", choices=sorted(bench.CONFIGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs the MI355X")
    dev = "cuda:0"
    cfg = bench.CONFIGS[args.config]
    torch.manual_seed(0)
    m = models.setup(argparse.Namespace(**cfg["opt"])).to(dev).train()
    n = m.flat_params.numel()
    g = m.flatten_grads()
    g.normal_(std=0.5 / n ** 0.5)                  # norm ~0.5 < the clip: the sweeps leave the gradient as it is, run after run
    snap = m.weights_b16() if m.bf16_storage else None
    b16 = 2 if snap is not None else 0
    sumsq = torch.zeros(1, device=dev)
    ops.sumsq(g, sumsq)
    o = argparse.Namespace(learning_rate=0.0, optim_alpha=0.9, optim_beta=0.999, optim_epsilon=1e-8, weight_decay=0.0)

    sweeps = {}
    mo, vo = torch.zeros_like(m.flat_params), torch.zeros_like(m.flat_params)
    sweeps["adam, whole bucket (FlatAdam)"] = (lambda: ops.clip_optim_step("adam", m.flat_params, g, mo, vo, None, sumsq, 10.0, 1.0, 0.0, 0.9,
                                                                           0.999, 1e-8, 0.0, 5, p_bf16=snap), n * (32 + b16))
    for rule in RULES:
        o.optim = rule
        fo = optim.build_optimizer(m, o)
        kern, h0, h1, eps, nest = fo._rule(fo.param_groups[0])
        live = n if fo._live is None else int((fo._live[1::2] - fo._live[0::2]).sum())
        per = (32 if kern in ("adam", "adamw") else 24) + b16
        wd = fo.param_groups[0]["weight_decay"]
        sweeps[rule] = ((lambda fo=fo, kern=kern, h0=h0, h1=h1, eps=eps, nest=nest, wd=wd:
                         ops.clip_optim_step(kern, m.flat_params, g, fo._s1, fo._s2, fo._live, sumsq, 10.0, 1.0, 0.0, h0, h1, eps, wd, 5,
                                             nesterov=nest, first=False, p_bf16=snap)), live * per)

    times = {k: [] for k in sweeps}
    for fn, _ in sweeps.values():                  # warm-up: code objects, first touches
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        order = list(sweeps) if r % 2 == 0 else list(reversed(sweeps))
        for k in order:
            fn = sweeps[k][0]
            fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.iters)
    rows = {}
    print(f"{args.config}: {n / 1e6:.1f} M parameters in the bucket, bf16 snapshot {'on' if snap is not None else 'off'}; "
          f"{args.rounds} rounds x {args.iters} sweeps")
    print(f"{'sweep':30s} {'MB moved':>9s} {'median us':>10s} {'min us':>8s} {'max us':>8s} {'TB/s':>6s}")
    for k, (_, nbytes) in sweeps.items():
        med, lo, hi = statistics.median(times[k]), min(times[k]), max(times[k])
        rows[k] = dict(bytes=nbytes, median_us=round(med * 1e3, 1), min_us=round(lo * 1e3, 1), max_us=round(hi * 1e3, 1),
                       tb_s=round(nbytes / (med * 1e-3) / 1e12, 2))
        print(f"{k:30s} {nbytes / 1e6:9.1f} {med * 1e3:10.1f} {lo * 1e3:8.1f} {hi * 1e3:8.1f} {rows[k]['tb_s']:6.2f}")
    print(json.dumps(dict(config=args.config, params=n, bf16_snapshot=snap is not None, rounds=args.rounds, iters=args.iters, sweeps=rows)))


if __name__ == "__main__":
    main()
