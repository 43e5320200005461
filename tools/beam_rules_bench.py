#!/usr/bin/env python3
"""What `eval_kwargs["beam_rules"]` (block_trigrams and the bad-ending ban per beam) costs in beam search: the key
absent against both rules on, on the two decode shapes test.sh's beam 2 runs in.

    python tools/beam_rules_bench.py [--out profiles/r24_beam_rules_bench.txt] [--rounds 5] [--reps 3] [--images 256] [--skip batch]

Method of tools/decode_rules_bench.py: legs run on ONE model and ONE set of inputs (captured searches are keyed by the rules),
interleaved inside every round so that drift hits both alike; two warm-up calls per leg, then per round `reps` timed calls per leg
(host clock around the call plus a synchronise; the median of the round).  Reported: the median over the rounds, the spread
(max - min) of the round medians, and on / off.  `off` is the yardstick: it is what a call without the key runs.  No threshold is
asserted.

Cases (bench.py's Sub_GC_Kar, fp32, random weights, beam 2):
  one image   the reference-shaped call, one graph replay per image, 16 images per timed call.  On top of `off` a ruled step has three
              launches: subgc_decode_rules on the logits rows, the history's row gather and the 2-D copy of the step's words.
  batch       sample_images over `images` images, NMS 0.75, <= 10 sub-graphs each (5120 beam rows at 256 images, V + 1 = 9488), eager"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_beam_rules_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out: one, batch")
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))

    import torch
    import bench
    import subgc.models as models
    from subgc import synthetic
    assert torch.cuda.is_available(), "beam_rules_bench needs the MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    OFF = dict(sample_max=1, beam_size=2)
    ON = dict(OFF, beam_rules=dict(block_trigrams=1, block_bad_endings=1, bad_ending_ids=list(range(1, 15))))

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

    lines = [f"beam rules bench: {a.rounds} rounds x {a.reps} calls per leg, legs interleaved on one model; "
             "median of the round medians, ms (spread = max - min of them)"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def report(title, res):
        (off, sp0), (on, sp1) = res
        say(f"{title}\n    off {off:9.3f}  (spread {sp0:.3f})\n    on  {on:9.3f}  (spread {sp1:.3f})    / off {on / off:.3f}    - off {on - off:+.3f} ms")
        return on - off

    kar = models.setup(argparse.Namespace(**dict(bench.KAR, gpn_nms_thres=0.75, gpn_max_subg=10, test_LSTM=1))).to(dev).eval()
    T = kar.seq_length
    images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(50, seed=900 + i).items()} for i in range(a.images)]
    if "one" not in skip:
        ims = [synthetic.sample_args(b) for b in images[:16]]
        rows = sum(kar(*b, opt=ON, mode="sample")[0].size(0) for b in ims)
        d = report(f"Sub_GC_Kar fp32, beam 2, one image per call (graph replay), ms per 16 images ({rows} sub-graphs in all)",
                   measure([lambda: [kar(*b, opt=OFF, mode="sample") for b in ims], lambda: [kar(*b, opt=ON, mode="sample") for b in ims]]))
        say(f"    per image and decoder step (T = {T} steps ruled, T history forks): {1e3 * d / 16 / T:.2f} us for the three added launches")
    if "batch" not in skip:
        hold = {"skip_att": True}
        kar.sample_images(images, opt=ON, batch_out=hold)
        n = hold["seq"].size(0)
        st = hold["rule_stats"].sum(0).tolist()
        say(f"(the ruled batch: {n} sub-graphs x beam 2 = {2 * n} rows; the winners' counters summed [trigram, -, bad ending, -] = {st}; the rules pass "
            f"moves 2 x {2 * n} x {kar.vocab_size + 1} x 4 B = {4 * n * (kar.vocab_size + 1) * 4 / 1e6:.0f} MB per step)")
        report(f"Sub_GC_Kar fp32, beam 2, one decode batch of {len(images)} images ({2 * n} rows, eager), ms per batch",
               measure([lambda: kar.sample_images(images, opt=OFF), lambda: kar.sample_images(images, opt=ON)]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
