#!/usr/bin/env python3
"""Accuracy and oracle scores of one decode batch (cook + subgc_accuracy_rows + subgc_accuracy_oracle, subgc.accuracy) next to the decode
that produces the batch, and the reference scorers' CPU time over the same captions.

    python tools/accuracy_bench.py [--out profiles/r11_accuracy_bench.txt] [--reps 30]
    python tools/accuracy_bench.py --script-only [--sizes kar=10x256 ...]        (no GPU; where the reference lies)

Shapes (those of consensus_bench.py): 256 images x <= 10 captions (test.sh, Karpathy), 8 images x <= 100 and 8 images x <= 1000 (the
MRNN setting); every image has 5 reference captions, oracle_num = the nominal caption count.  The captions that are scored have the
decode batch's row layout but are cut from the image's references over a 30-word vocabulary with a word changed here and there, so
n-grams match (a randomly initialised decoder emits word salad).
Method: every shape is warmed up, then timed `reps` times; device time = HIP events around the three launches (with the upload of the
boundaries), wall = host clock around score() incl. its device -> host copy; median, min and max are reported.  The decode is timed in
the same process, same box: host clock around sample_images + synchronise.
--script-only runs the reference's own `Bleu(4)`, `Rouge()` and `Cider()` (imported from where the reference lies) once per caption
position over captions of the same generator and sizes, short images padded with their first caption, as misc/sentence_utils.py:
language_eval loops -- without its json round trip through the COCO API and without the PTB tokenizer, METEOR and SPICE (all Java), so
this understates the reference."""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

REF_SCORERS = "/root/reference/misc/coco-caption"
V, T, N_REFS = 30, 16, 5
NOMINAL = {"kar": [10] * 256, "mrnn100": [100] * 8, "mrnn1000": [1000] * 8}


def make_case(sizes, seed):
    """Per image its reference captions and its candidate captions (id lists, <= T words); deterministic in (sizes, seed)."""
    rng = np.random.default_rng(seed)
    refs, caps = [], []
    for n in sizes:
        mine = [[int(x) for x in rng.integers(1, V + 1, size=int(rng.integers(7, T + 1)))] for _ in range(N_REFS)]
        out = []
        for _ in range(n):
            t = mine[int(rng.integers(N_REFS))]
            a = int(rng.integers(0, 3))
            c = list(t[a:a + int(rng.integers(1, len(t) + 1))])
            if rng.random() < 0.6:
                c[int(rng.integers(len(c)))] = int(rng.integers(1, V + 1))
            out.append(c)
        refs.append(mine)
        caps.append(out)
    return refs, caps


def sent(c):
    return " ".join(f"w{x}" for x in c)


def script_time(name, sizes, seed):
    """Wall seconds of the reference's three scorers, once per caption position, over these captions."""
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.cider.cider import Cider
    from pycocoevalcap.rouge.rouge import Rouge
    refs, caps = make_case(sizes, seed)
    gts = {i: [sent(r) for r in mine] for i, mine in enumerate(refs)}
    spent = {"Bleu": 0.0, "Cider": 0.0, "Rouge": 0.0}
    for p in range(max(sizes)):
        res = {i: [sent(mine[p] if p < len(mine) else mine[0])] for i, mine in enumerate(caps)}
        for key, scorer in (("Bleu", Bleu(4)), ("Cider", Cider()), ("Rouge", Rouge())):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                scorer.compute_score(gts, res)
            spent[key] += time.perf_counter() - t0
    return (f"reference scorers on this CPU, {name}: {len(sizes)} images, {sum(sizes)} captions, {max(sizes)} positions, {N_REFS} references per image: "
            f"{sum(spent.values()):.2f} s (Bleu {spent['Bleu']:.2f}, Cider {spent['Cider']:.2f}, Rouge {spent['Rouge']:.2f}; "
            "without the COCO json round trip, the PTB tokenizer, METEOR and SPICE: this understates the reference)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_accuracy_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--script-only", action="store_true", help="only time the reference's scorers on the CPU (needs no GPU, needs the reference)")
    ap.add_argument("--sizes", nargs="*", default=[], help="script-only: name=a,b,c or name=NxI caption counts per image (default: the nominal shapes)")
    a = ap.parse_args()
    if a.script_only:
        assert os.path.isdir(REF_SCORERS), "--script-only needs the reference's misc/coco-caption"
        sys.path.insert(0, REF_SCORERS)
        shapes = dict(NOMINAL)
        for s in a.sizes:
            name, v = s.split("=")
            shapes[name] = [int(v.split("x")[0])] * int(v.split("x")[1]) if "x" in v else [int(x) for x in v.split(",")]
        lines = [script_time(name, sizes, 100 + j) for j, (name, sizes) in enumerate(sorted(shapes.items()))]
        print("\n".join(lines))
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return

    import torch
    import bench
    import subgc.models as models
    from subgc import accuracy, ops, synthetic
    assert torch.cuda.is_available(), "accuracy_bench needs the MI355X (or --script-only)"
    dev = torch.device("cuda:0")
    vocab = {str(i): f"w{i}" for i in range(1, V + 1)}
    lines = [f"accuracy bench: cook + rows + oracle over one decode batch; {N_REFS} references per image, oracle_num = the nominal caption count"]
    mrnn = dict(gpn_nms_thres=0.55, use_topk_sampling=1, topk_temp=0.6, the_k=3)
    shapes = [("256 images x <= 10", 256, 50, dict(gpn_nms_thres=0.75, gpn_max_subg=10), 10),
              ("8 images x <= 100", 8, 100, dict(mrnn, gpn_max_subg=100), 100),
              ("8 images x <= 1000", 8, 500, dict(mrnn, gpn_max_subg=1000), 1000)]
    sopt = dict(sample_max=1, beam_size=1)
    q = lambda x: f"median {statistics.median(x):.3f} (min {min(x):.3f}, max {max(x):.3f})"  # noqa: E731
    for j, (name, I, Mc, over, oracle_num) in enumerate(shapes):
        torch.manual_seed(0)
        m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, **over))).to(dev).eval()
        images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(Mc, seed=700 + i).items()} for i in range(I)]
        for _ in range(2):
            hold = {"skip_att": True}
            m.sample_images(images, opt=sopt, batch_out=hold)
        torch.cuda.synchronize()
        dec = []
        for _ in range(max(5, a.reps // 4)):
            t = time.perf_counter()
            m.sample_images(images, opt=sopt, batch_out={"skip_att": True})
            torch.cuda.synchronize()
            dec.append(1e3 * (time.perf_counter() - t))
        bounds = [int(x) for x in hold["bounds"]]
        rows = bounds[-1]
        sizes = [b - x for x, b in zip(bounds, bounds[1:])]
        refs_ids, caps = make_case(sizes, 100 + j)
        host_rows = np.zeros((rows, T), np.int64)
        r = 0
        for mine in caps:
            for c in mine:
                host_rows[r, :len(c)] = c
                r += 1
        seq = torch.from_numpy(host_rows).to(dev)
        refs = accuracy.AccuracyReferences([[[f"w{x}" for x in c] for c in mine] for mine in refs_ids], vocab, device=dev)
        scorer = accuracy.AccuracyScorer(refs, oracle_num)
        index = list(range(I))
        arena = torch.empty(scorer.arena_words(rows, I), dtype=torch.int32, device=dev)
        for _ in range(3):
            per = scorer.score(seq, bounds, index)
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tab = ops.upload(bounds + index, torch.int32, dev)
            scorer.enqueue(seq, tab, I, tab[I + 1:], None, 0, arena)
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
            t = time.perf_counter()
            scorer.score(seq, bounds, index)
            wall.append(1e3 * (time.perf_counter() - t))
        s = accuracy.summarize(per)
        lines.append(f"{name}: decode batch {rows} rows"
                     f" (sizes: {','.join(str(x) for x in sizes) if len(set(sizes)) > 1 else f'{sizes[0]}x{len(sizes)}'})")
        lines.append(f"    decode (sample_images, wall ms, {len(dec)} runs):     {q(dec)}")
        lines.append(f"    scoring device ms (events, {a.reps} runs):           {q(ev)}")
        lines.append(f"    scoring wall ms incl. the host copy ({a.reps} runs): {q(wall)}")
        lines.append(f"    scoring / decode (medians): {statistics.median(wall) / statistics.median(dec):.4f};  summary: "
                     + ", ".join(f"{k} {s[k]:.4g}" for k in accuracy.NAMES) + "; oracle " + ", ".join(f"{k} {s['oracle'][k]:.4g}" for k in accuracy.NAMES))
        del m
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
