#!/usr/bin/env python3
"""Controllability scores of the kept rows of an `sct` decode (subgc.controllability: subgc_control_noun_iou + the accuracy launches with
the upload and the copy back) next to the decode that produces the rows, and the reference's CPU time over the same pairs.

    python tools/controllability_bench.py [--out profiles/r13_controllability_bench.txt] [--reps 30] [--images 100]
    python tools/controllability_bench.py --script-only [--images 100]           (no GPU; where the reference lies)

Shape: `images` images x 10 region sets (test.sh's controllability runs decode every candidate sub-graph; the first half is kept), 5
ground-truth captions per region set with 2-6 vector words among 6-14 words, 300-d vectors for 400 words of a 1000-word vocabulary.  The
scored rows have the decode's row layout, but their words are drawn over that vocabulary (a randomly initialised decoder emits word
salad), half of a row's vector words taken from its group so that the assignment has something to find.
Method: warmed up, then timed `reps` times; device time = HIP events around the upload and the launches, wall = host clock around upload
+ launches + the device -> host copy + unpack; median, min and max are reported.  The decode is timed in the same process, same box: host
clock around sample_images(sct=1) over the images + synchronise.
--script-only runs the reference's own `NounIoU.score` (imported from where the reference lies, on a temporary pickle of the vectors)
over the same pairs, and its pycocoevalcap Bleu / Rouge / Cider over the same groups.  `munkres` is not installed there, so a stand-in
module built on scipy.optimize.linear_sum_assignment solves the assignments -- compiled code in the place of the pure-Python solver, which
UNDERSTATES the reference; METEOR, SPICE and the PTB tokenizer (Java) are left out, which understates it further."""
import argparse
import contextlib
import io
import os
import pickle
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

REF = "/root/reference"
V, N_NOUN, D, T, SETS, N_CAPS = 1000, 400, 300, 16, 10, 5
STUB = ("import numpy as np\nfrom scipy.optimize import linear_sum_assignment\n"
        "def make_cost_matrix(profit):\n    profit = np.asarray(profit)\n    return profit.max() - profit\n"
        "class Munkres:\n    def compute(self, cost):\n        r, c = linear_sum_assignment(np.asarray(cost))\n"
        "        return [(int(a), int(b)) for a, b in zip(r, c)]\n")


def make_case(rows, seed):
    """-> (vocabulary, {word: vector}, ground-truth groups as strings, token rows [rows, T])."""
    rng = np.random.default_rng(seed)
    vocab = {str(i): f"w{i}" for i in range(1, V + 1)}
    nouns = np.arange(1, N_NOUN + 1)
    vectors = {f"w{i}": rng.standard_normal(D).astype(np.float32) for i in nouns}
    groups, seq = [], np.zeros((rows, T), np.int64)
    for r in range(rows):
        caps, mine = [], []
        for _ in range(N_CAPS):
            ws = [int(x) for x in rng.choice(nouns, size=int(rng.integers(2, 7)))]
            mine += ws
            ws += [int(x) for x in rng.integers(N_NOUN + 1, V + 1, size=int(rng.integers(4, 9)))]
            caps.append(" ".join(f"w{ws[i]}" for i in rng.permutation(len(ws))))
        groups.append(caps)
        n = int(rng.integers(1, 6))
        ws = [int(rng.choice(mine)) if rng.random() < 0.5 else int(rng.choice(nouns)) for _ in range(n)]
        ws += [int(x) for x in rng.integers(N_NOUN + 1, V + 1, size=int(rng.integers(3, T - n + 1)))]
        ws = [ws[i] for i in rng.permutation(len(ws))]
        seq[r, :len(ws)] = ws
    return vocab, vectors, groups, seq


def script_time(rows, seed):
    vocab, vectors, groups, seq = make_case(rows, seed)
    preds = [" ".join(vocab[str(int(x))] for x in row if x > 0) for row in seq]
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "munkres.py"), "w") as f:
            f.write(STUB)
        with open(os.path.join(tmp, "vectors.pkl"), "wb") as f:
            pickle.dump(vectors, f)
        sys.path[:0] = [tmp, os.path.join(REF, "misc", "controllability"), os.path.join(REF, "misc", "coco-caption")]
        sys.dont_write_bytecode = True
        from noun_iou import NounIoU
        from pycocoevalcap.bleu.bleu import Bleu
        from pycocoevalcap.cider.cider import Cider
        from pycocoevalcap.rouge.rouge import Rouge
        scorer = NounIoU(pre_comp_file=os.path.join(tmp, "vectors.pkl"))
        t0 = time.perf_counter()
        scores = []
        for cap, caps in zip(preds, groups):                                # controllability_score.py:40-52
            s = 0.
            for c in caps:
                s += scorer.score(c, cap)
            scores.append(s / len(caps))
        t_iou = time.perf_counter() - t0
        gts, gen = dict(enumerate(groups)), {i: [c] for i, c in enumerate(preds)}
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            b = Bleu(4).compute_score(gts, gen)[0]
            ro = Rouge().compute_score(gts, gen)[0]
            ci = Cider().compute_score(gts, gen)[0]
        t_coco = time.perf_counter() - t0
    return (f"reference on this CPU: {rows} generated captions x {N_CAPS} ground-truth captions ({rows * N_CAPS} pairs): NounIoU.score {t_iou:.2f} s, "
            f"Bleu + Rouge + Cider {t_coco:.2f} s (Noun IoU {np.mean(scores):.4f}, Bleu_1 {b[0]:.4f}, ROUGE_L {ro:.4f}, CIDEr {ci:.4f}) -- with "
            "scipy.optimize.linear_sum_assignment in the place of the pure-Python munkres solver (not installed here) and without METEOR, SPICE and "
            "the PTB tokenizer (Java): this understates the reference")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_controllability_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--script-only", action="store_true", help="only time the reference's scorers on the CPU (needs no GPU, needs the reference)")
    a = ap.parse_args()
    rows = a.images * SETS
    if a.script_only:
        assert os.path.isdir(REF), "--script-only needs the reference"
        line = script_time(rows, 100)
        print(line)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        return

    import torch
    import bench
    import subgc.models as models
    from subgc import controllability, ops, synthetic
    assert torch.cuda.is_available(), "controllability_bench needs the MI355X (or --script-only)"
    dev = torch.device("cuda:0")
    q = lambda x: f"median {statistics.median(x):.3f} (min {min(x):.3f}, max {max(x):.3f})"  # noqa: E731
    torch.manual_seed(0)
    m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, sct=1))).to(dev).eval()
    images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(SETS, seed=700 + i).items()} for i in range(a.images)]
    sopt = dict(sample_max=1, beam_size=1, sct=1)
    with torch.no_grad():
        for _ in range(2):
            res = m.sample_images(images, opt=sopt)
        torch.cuda.synchronize()
        kept = sum(r[2].size(0) // 2 for r in res)
        assert kept == rows, (kept, rows)
        dec = []
        for _ in range(max(5, a.reps // 4)):
            t = time.perf_counter()
            m.sample_images(images, opt=sopt)
            torch.cuda.synchronize()
            dec.append(1e3 * (time.perf_counter() - t))
    vocab, vectors, groups, seq_h = make_case(rows, 100)
    refs = controllability.ControlReferences(groups, controllability.NounVectors(vectors, vocab, device=None), vocab, device=dev)
    sc = controllability.ControlScorer(refs)
    seq = torch.from_numpy(seq_h).to(dev)
    index = list(range(rows))
    plan = sc.plan(index)
    arena = torch.empty(sc.arena_words(plan), dtype=torch.int32, device=dev)
    table = plan["idx"].tolist() + plan["pair_off"].tolist() + list(range(rows + 1)) + index

    def once():
        tab = ops.upload(table, torch.int32, dev)
        sc.enqueue_noun_iou(seq, tab, 0, arena, plan)
        sc.acc.enqueue(seq, tab[2 * rows + 1:3 * rows + 2], rows, tab[3 * rows + 2:4 * rows + 2], None, 0, sc.views(arena, plan)[0])

    def noun_only():
        sc.enqueue_noun_iou(seq, d_tab, 0, arena, plan)

    for _ in range(3):
        once()
        per = sc.unpack(arena.cpu().numpy(), plan)
    d_tab = ops.upload(table, torch.int32, dev).clone()
    ev, ev_noun, wall = [], [], []
    for _ in range(a.reps):
        for fn, into in ((once, ev), (noun_only, ev_noun)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            into.append(e0.elapsed_time(e1))
        t = time.perf_counter()
        per = sc.score(seq, index)
        wall.append(1e3 * (time.perf_counter() - t))
    s = controllability.summarize(per)
    mn = np.concatenate([e["pair_mn"] for e in per])
    lines = [f"controllability bench: Noun IoU + BLEU / ROUGE-L / CIDEr over the kept rows of an sct decode; {a.images} images x {SETS} region sets "
             f"({rows} rows), {N_CAPS} ground-truth captions each ({plan['P']} pairs; m mean {mn[:, 0].mean():.2f} max {mn[:, 0].max()}, n mean "
             f"{mn[:, 1].mean():.2f} max {mn[:, 1].max()}), d = {D}",
             f"    decode (sample_images with sct=1, per image, wall ms, {len(dec)} runs): {q(dec)}",
             f"    subgc_control_noun_iou alone, device ms (events, {a.reps} runs):          {q(ev_noun)}",
             f"    upload + Noun IoU + accuracy launches, device ms (events, {a.reps} runs): {q(ev)}",
             f"    ControlScorer.score: upload + launches + host copy + unpack, wall ms:    {q(wall)}",
             f"    scoring / decode (medians): device {statistics.median(ev) / statistics.median(dec):.5f}, wall "
             f"{statistics.median(wall) / statistics.median(dec):.4f};  summary: " + ", ".join(f"{k} {float(s[k]):.4g}" for k in controllability.NAMES)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
