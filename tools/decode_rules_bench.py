#!/usr/bin/env python3
"""What the decode rules (subgc.decode_rules) cost in the token loop: rules off against all four rules on, on the decode
shapes a user runs.

    python tools/decode_rules_bench.py [--out profiles/r23_decode_rules_bench.txt] [--rounds 5] [--reps 3] [--images 256] [--skip mrnn]

Legs run on ONE model and ONE set of inputs (the rules are a key of the `eval_kwargs` dict; captured graphs are keyed by them),
interleaved inside every round so that drift hits all alike.  Method of tools/decode_b16_bench.py: two warm-up calls per leg, then per
round `reps` timed calls per leg (host clock around the call plus a synchronise; the median of the round).  Reported: the median over
the rounds, the spread (max - min) of the round medians, and on / off.  `off` is the yardstick: it is what a call without the keys runs.
No threshold is asserted.

Cases (bench.py's Sub_GC_Kar, fp32, random weights):
  greedy batch   sample_images over `images` images, NMS 0.75, <= 10 sub-graphs each (2560 rows at 256 images, V + 1 = 9488)
  MRNN           one image per call, 1000 candidates, NMS 0.55, keep up to 1000, top-k sampling (k = 3, T = 0.6), 4 images
  one image      the reference-shaped call, one graph replay per image, 16 images per timed call.  THREE legs: off (the fused greedy
                 loop), off with decode_fused_pick = 0 (the generic step -> pick loop the ruled loop builds on), on.  generic - fused is
                 what the ruled loop gives up by leaving the fused pick; on - generic is the rules launch itself.
  kernel         subgc_decode_rules alone on [rows, 9488] fp32 logits, all four rules with counters, device events around 20 launches:
                 us per launch and the bytes it moves (one read and one write of the rows) per second"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tools")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_decode_rules_bench.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out: greedy, mrnn, one, kernel")
    a = ap.parse_args()
    skip = set(filter(None, a.skip.split(",")))

    import torch
    import bench
    import subgc.models as models
    from subgc import ops, synthetic
    from subgc.decode_rules import DecodeRules
    assert torch.cuda.is_available(), "decode_rules_bench needs the MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    OFF = dict(sample_max=1, beam_size=1)
    ON = dict(OFF, block_trigrams=1, suppress_unk=1, decoding_constraint=1, block_bad_endings=1, bad_ending_ids=list(range(1, 15)))

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

    lines = [f"decode rules bench: {a.rounds} rounds x {a.reps} calls per leg, legs interleaved on one model; "
             "median of the round medians, ms (spread = max - min of them)"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def report(title, names, res):
        base = res[0][0]
        say(title + "".join(f"\n    {nm:<14}{ms:9.3f}  (spread {sp:.3f})" + ("" if i == 0 else f"    / {names[0]} {ms / base:.3f}    - {names[0]} {ms - base:+.3f} ms")
                            for i, (nm, (ms, sp)) in enumerate(zip(names, res))))

    test = dict(test_LSTM=1)
    if not {"greedy", "one"} <= skip:
        kar = models.setup(argparse.Namespace(**dict(bench.KAR, gpn_nms_thres=0.75, gpn_max_subg=10, **test))).to(dev).eval()
        images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(50, seed=900 + i).items()} for i in range(a.images)]
        if "greedy" not in skip:
            hold = {"skip_att": True}
            kar.sample_images(images, opt=ON, batch_out=hold)
            rows, T = hold["seq"].shape
            st = hold["rule_stats"].sum(0).tolist()
            steps = min(T, int((hold["seq"] > 0).any(0).sum().item()) + 1)
            say(f"(the ruled batch: {rows} rows, counters summed over the rows [trigram, repeat, bad ending, arg-max moved] = {st}; about {steps} of {T} steps run; "
                f"the pass moves 2 x {rows} x {kar.vocab_size + 1} x 4 B = {2 * rows * (kar.vocab_size + 1) * 4 / 1e6:.0f} MB per step)")
            report(f"Sub_GC_Kar fp32, greedy, one decode batch of {len(images)} images ({rows} rows), ms per batch", ("off", "on"),
                   measure([lambda: kar.sample_images(images, opt=OFF), lambda: kar.sample_images(images, opt=ON)]))
        if "one" not in skip:
            ims = [synthetic.sample_args(b) for b in images[:16]]

            def one(opt, fused):
                def run():
                    kar.decode_fused_pick = fused
                    return [kar(*b, opt=opt, mode="sample") for b in ims]
                return run
            res = measure([one(OFF, True), one(OFF, False), one(ON, True)])
            kar.decode_fused_pick = True
            report("Sub_GC_Kar fp32, greedy, one image per call (graph replay), ms per 16 images", ("off (fused)", "off (generic)", "on"), res)
            say(f"    giving up the fused pick: {res[1][0] - res[0][0]:+.3f} ms; the rules launches on top of the generic loop: {res[2][0] - res[1][0]:+.3f} ms "
                f"(per 16 images; {1e3 * (res[2][0] - res[1][0]) / 16 / kar.seq_length:.2f} us per step and image)")
        del kar, images
    if "mrnn" not in skip:
        mr = models.setup(argparse.Namespace(**dict(bench.KAR, gpn_nms_thres=0.55, gpn_max_subg=1000, use_topk_sampling=1, topk_temp=0.6, the_k=3,
                                                    **test))).to(dev).eval()
        cands = [synthetic.sample_args({k: v.to(dev) for k, v in synthetic.make_test_batch(500, seed=900 + i).items()}) for i in range(4)]
        kept = sum(mr(*b, opt=OFF, mode="sample")[0].size(0) for b in cands) / len(cands)
        report(f"Sub_GC_S_MRNN shape fp32: 1000 candidates, top-k 3, one image per call ({kept:.0f} rows kept per image), ms per 4 images", ("off", "on"),
               measure([lambda: [mr(*b, opt=OFF, mode="sample") for b in cands], lambda: [mr(*b, opt=ON, mode="sample") for b in cands]]))
        del mr, cands
    if "kernel" not in skip:
        rules = DecodeRules.from_options(ON)
        V, T, t = 9488, 20, 10
        bad = torch.tensor(rules.bad_ids, device=dev, dtype=torch.int32)
        for rows in (10, 2560):
            x0 = torch.randn(rows, V, device=dev) * 4
            seq = torch.randint(1, 40, (rows, T), device=dev)
            stats = torch.zeros(rows, 4, device=dev, dtype=torch.int32)
            bufs = [x0.clone() for _ in range(4)]                                  # (the pass is in place: rotate copies, a log-softmaxed row is input like any other)
            for b in bufs:
                ops.decode_rules(b, seq, t, rules.flags, rules.trigram_pen, bad, stats)
            torch.cuda.synchronize()
            us = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(20):
                    ops.decode_rules(bufs[i % 4], seq, t, rules.flags, rules.trigram_pen, bad, stats)
                e1.record()
                torch.cuda.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 20)
            med = statistics.median(us)
            say(f"subgc_decode_rules alone, [{rows}, {V}] fp32, all four rules with counters, step {t}: {med:.2f} us per launch "
                f"(spread {max(us) - min(us):.2f}), {2 * rows * V * 4 / med / 1e3:.1f} GB/s of the {2 * rows * V * 4 / 1e6:.1f} MB it moves")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
