#!/usr/bin/env python3
"""The opt-in bf16-batched decode regime (opt.decode_b16_batched) against the fp32 decode it replaces, on the decode shapes of
more than 32 rows under compute_dtype = bf16.

    python tools/decode_b16_bench.py [--out profiles/r20_decode_b16_bench.txt] [--rounds 5] [--reps 3] [--images 256] [--skip scst]

Legs `off` / `on` run on ONE model and ONE set of inputs (the option is a model attribute; weight snapshots and captured graphs are keyed
by it), interleaved inside every round so that drift hits both alike.  Method of tools/beam_att_bench.py: two warm-up calls per leg, then
per round `reps` timed calls per leg (host clock around the call plus a synchronise; the median of the round).  Reported: the median over
the rounds, the spread (max - min) of the round medians, and on / off.  `off` is the yardstick: it is what a model built without the
option runs.  No threshold is asserted.

Cases (bench.py's Sub_GC_Kar with compute_dtype = bf16 and random weights unless another model is named):
  greedy batch   sample_images over `images` images, NMS 0.75, <= 10 sub-graphs each
  beam 2 batch   the same images at beam_size = 2 (eager search)
  MRNN           one image per call, 1000 candidates, NMS 0.55, keep up to 1000, top-k sampling (k = 3, T = 0.6), 4 images
  forced 320     forced.forced_decode(return_att=True) of 64 images x 5 token rows of 17 words = 320 rows (tools/forced_bench.py's row count
                 on random token rows)
  SCST           tools/self_critical_cost.py's Full_GC_Kar bf16 B = 256 self-critical step, the rollout bracketed by synchronisations:
                 the rollout's ms and the whole step's ms"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_decode_b16_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out: greedy, beam, mrnn, forced, scst")
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))

    import numpy as np
    import torch
    import bench
    import subgc.models as models
    from subgc import forced, selfcritical, synthetic
    assert torch.cuda.is_available(), "decode_b16_bench needs the MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def legs_of(m, call):
        def leg(flag):
            def run():
                m.decode_b16_batched = flag
                return call()
            return run
        return leg(0), leg(1)

    def measure(legs):
        for fn in legs:
            fn(); fn()
        torch.cuda.synchronize()
        rounds = [[] for _ in legs]
        for _ in range(a.rounds):
            for k, fn in enumerate(legs):
                ms = []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ms.append(1e3 * (time.perf_counter() - t))
                rounds[k].append(statistics.median(ms))
        return [(statistics.median(r), max(r) - min(r)) for r in rounds]

    lines = [f"bf16-batched decode bench: {a.rounds} rounds x {a.reps} calls per leg, legs off / on interleaved on one model; "
             "median of the round medians, ms (spread = max - min of them)"]

    def report(title, res):
        (off, s_off), (on, s_on) = res
        lines.append(f"{title}\n    off  {off:9.3f}  (spread {s_off:.3f})\n    on   {on:9.3f}  (spread {s_on:.3f})    on / off {on / off:.3f}")
        print(lines[-1], flush=True)

    test = dict(test_LSTM=1, compute_dtype="bf16")
    if not {"greedy", "beam", "forced"} <= skip:
        kar = models.setup(argparse.Namespace(**dict(bench.KAR, gpn_nms_thres=0.75, gpn_max_subg=10, **test))).to(dev).eval()
        images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(50, seed=900 + i).items()} for i in range(a.images)]
        if "greedy" not in skip:
            rows = sum(r[0].size(0) for r in kar.sample_images(images, opt=dict(sample_max=1, beam_size=1)))
            report(f"Sub_GC_Kar bf16, greedy, one decode batch of {len(images)} images ({rows} rows), ms per batch",
                   measure(legs_of(kar, lambda: kar.sample_images(images, opt=dict(sample_max=1, beam_size=1)))))
        if "beam" not in skip:
            report(f"Sub_GC_Kar bf16, beam 2, one decode batch of {len(images)} images (eager), ms per batch",
                   measure(legs_of(kar, lambda: kar.sample_images(images, opt=dict(sample_max=1, beam_size=2)))))
        if "forced" not in skip:
            rng = np.random.default_rng(3)
            ims = images[:64]
            tokens = [rng.integers(1, kar.vocab_size + 1, (5, 17)) for _ in ims]
            report("Sub_GC_Kar bf16, forced decode with attention, 64 images x 5 rows x 17 words = 320 rows, ms per call",
                   measure(legs_of(kar, lambda: forced.forced_decode(kar, ims, tokens, return_att=True))))
        del kar, images
    if "mrnn" not in skip:
        mr = models.setup(argparse.Namespace(**dict(bench.KAR, gpn_nms_thres=0.55, gpn_max_subg=1000, use_topk_sampling=1, topk_temp=0.6, the_k=3,
                                                    **test))).to(dev).eval()
        cands = [{k: v.to(dev) for k, v in synthetic.make_test_batch(500, seed=900 + i).items()} for i in range(4)]
        kept = sum(mr(*synthetic.sample_args(b), opt=dict(sample_max=1, beam_size=1), mode="sample")[0].size(0) for b in cands) / len(cands)
        report(f"Sub_GC_S_MRNN shape bf16: 1000 candidates, top-k 3, one image per call ({kept:.0f} rows kept per image), ms per 4 images",
               measure(legs_of(mr, lambda: [mr(*synthetic.sample_args(b), opt=dict(sample_max=1, beam_size=1), mode="sample") for b in cands])))
        del mr, cands
    if "scst" not in skip:
        import self_critical_cost as scc
        step, B, reward = scc.build("full_gc_kar", dev)
        model = next(c.cell_contents for c in step.__closure__ if isinstance(c.cell_contents, models.LossWrapper)).model      # the step's model
        res = {0: [], 1: []}
        for flag in (0, 1):                                                       # warm both legs (snapshots, workspaces)
            model.decode_b16_batched = flag
            step("scst"); step("scst")
        for _ in range(a.rounds):
            for flag in (0, 1):
                model.decode_b16_batched = flag
                res[flag].append(scc.shares(step, reward, a.reps))                # (rollout ms, reward ms, whole step ms), rollout bracketed
        for what, col in (("rollout", 0), ("whole SCST step, rollout and reward bracketed", 2)):
            report(f"Full_GC_Kar bf16 B = {B}, self-critical step: {what}, ms",
                   [(statistics.median(x[col] for x in res[f]), max(x[col] for x in res[f]) - min(x[col] for x in res[f])) for f in (0, 1)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
