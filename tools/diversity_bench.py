#!/usr/bin/env python3
"""Diversity scores of one decode batch (select + distinct + best, subgc.diversity) next to the decode that produces the batch, and
the reference script's CPU time over the same captions.

    python tools/diversity_bench.py [--out profiles/r10_diversity_bench.txt] [--reps 30]
    python tools/diversity_bench.py --script-only [--sizes kar=10x256 ...]        (no GPU; where the reference lies)

Shapes: 256 images x <= 10 captions (test.sh, Karpathy), 8 images x <= 1000 captions with top_n 20 / 100 (the MRNN setting), and the
same 8 images with every draw the whole image (top_n = 1000: the counting rank, the hash table and the distinct scan at full length).
The captions that are scored have the decode batch's row layout but are cut from a few templates per image over a 30-word
vocabulary, so captions repeat and n-grams overlap (a randomly initialised decoder emits word salad); 1/7 of them are training captions.
Method: every shape is warmed up, then timed `reps` times; device time = HIP events around the three launches (with the upload of
the set table), wall = host clock around score() incl. its device -> host copy; median, min and max are reported.  The decode is
timed in the same process, same box: host clock around sample_images + synchronise.
--script-only runs misc/diversity/diversity_score.py itself (runpy, with and without --evaluate_mB4) over captions of the same
generator and sizes, with a stand-in tokenizer that returns the strings unchanged: that UNDERSTATES the reference, whose mBLEU-4 makes
ten tokenizer calls per image and top_n, each starting a Java process."""
import argparse
import contextlib
import io
import os
import pickle
import runpy
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

REF_SCRIPT_DIR = "/root/reference/misc/diversity"
V, T = 30, 16
NOMINAL = {"kar": [10] * 256, "mrnn": [1000] * 8}


def make_captions(sizes, seed):
    """Per image its captions (id lists, <= T words) and fp32 scores; deterministic in (sizes, seed)."""
    rng = np.random.default_rng(seed)
    caps, scores = [], []
    for n in sizes:
        pool = [rng.integers(1, V + 1, size=int(rng.integers(7, T + 1))) for _ in range(4)]
        mine = []
        for _ in range(n):
            t = pool[int(rng.integers(len(pool)))]
            a = int(rng.integers(0, 3))
            c = t[a:a + int(rng.integers(1, len(t) + 1))].copy()
            if rng.random() < 0.4:
                c[int(rng.integers(len(c)))] = int(rng.integers(1, V + 1))
            mine.append([int(x) for x in c])
        caps.append(mine)
        scores.append(np.sort(rng.random(n).astype(np.float32))[::-1].copy())
    return caps, scores


def sent(c):
    return " ".join(f"w{x}" for x in c)


def train_strings(caps):
    return [sent(c) for mine in caps for c in mine[::7]]


def script_time(name, sizes, seed):
    """Wall seconds of the reference script over these captions, without and with --evaluate_mB4."""
    caps, scores = make_captions(sizes, seed)
    preds = [{"image_id": i, "caption": [sent(c) for c in mine], "subgraph_score": sc} for i, (mine, sc) in enumerate(zip(caps, scores))]
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for d in ("misc/diversity", "data", "stub"):
            os.makedirs(os.path.join(tmp, d))
        with open(os.path.join(tmp, "stub", "ptbtokenizer.py"), "w") as f:
            f.write("class PTBTokenizer:\n    def tokenize(self, d):\n        return {k: [c['caption'] for c in v] for k, v in d.items()}\n")
        np.save(os.path.join(tmp, "data", "MRNN_split_dict.npy"), {1: "train"})
        with open(os.path.join(tmp, "misc", "diversity", "all_caption_dict.pkl"), "wb") as f:
            pickle.dump({"1": train_strings(caps)}, f)
        np.save(os.path.join(tmp, "captions.npy"), preds)
        sys.path[:0] = [os.path.join(tmp, "stub"), REF_SCRIPT_DIR]
        argv, cwd = sys.argv, os.getcwd()
        os.chdir(os.path.join(tmp, "misc", "diversity"))
        try:
            for flag in ([], ["--evaluate_mB4"]):
                sys.argv = ["diversity_score.py", "--input_file", os.path.join(tmp, "captions.npy")] + flag
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    runpy.run_path(os.path.join(REF_SCRIPT_DIR, "diversity_score.py"), run_name="__main__")
                out.append(time.perf_counter() - t0)
        finally:
            sys.argv = argv
            os.chdir(cwd)
            del sys.path[:2]
    return (f"reference script on this CPU, {name}: {len(sizes)} images, {sum(sizes)} captions: {out[0]:.2f} s without mBLEU-4, {out[1]:.2f} s with it "
            "(stand-in tokenizer: the Java start-up of its ten tokenizer calls per image and top_n is absent, so this understates the reference)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_diversity_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--script-only", action="store_true", help="only time the reference script on the CPU (needs no GPU, needs the reference)")
    ap.add_argument("--sizes", nargs="*", default=[], help="script-only: name=a,b,c or name=NxI caption counts per image (default: the nominal shapes)")
    a = ap.parse_args()
    if a.script_only:
        assert os.path.isdir(REF_SCRIPT_DIR), "--script-only needs the reference's misc/diversity"
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
    from subgc import diversity, ops, synthetic
    assert torch.cuda.is_available(), "diversity_bench needs the MI355X (or --script-only)"
    dev = torch.device("cuda:0")
    vocab = {str(i): f"w{i}" for i in range(1, V + 1)}
    lines = ["diversity bench: select + distinct + best over one decode batch; n_best = 5, all four metrics, a novelty index of 1/7 of the captions"]
    mrnn = dict(gpn_nms_thres=0.55, gpn_max_subg=1000, use_topk_sampling=1, topk_temp=0.6, the_k=3)
    shapes = [("kar", "256 images x <= 10, top_n 20 / 100", 256, 50, dict(gpn_nms_thres=0.75, gpn_max_subg=10), (20, 100)),
              ("mrnn", "8 images x <= 1000, top_n 20 / 100", 8, 500, mrnn, (20, 100)),
              ("mrnn", "8 images x <= 1000, every draw the whole image", 8, 500, mrnn, (1000,))]
    sopt = dict(sample_max=1, beam_size=1)
    q = lambda x: f"median {statistics.median(x):.3f} (min {min(x):.3f}, max {max(x):.3f})"  # noqa: E731
    for j, (key, name, I, Mc, over, top_n) in enumerate(shapes):
        torch.manual_seed(0)
        m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, **over))).to(dev).eval()
        images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(Mc, seed=700 + i).items()} for i in range(I)]
        hold = {"skip_att": True}
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
        caps, scores = make_captions(sizes, 100 + (0 if key == "kar" else 1))
        host_rows = np.zeros((rows, T), np.int64)
        r = 0
        for mine in caps:
            for c in mine:
                host_rows[r, :len(c)] = c
                r += 1
        seq = torch.from_numpy(host_rows).to(dev)
        score = torch.from_numpy(np.concatenate(scores)).to(dev)
        ix = diversity.NoveltyIndex(train_strings(caps), vocab, device=dev)
        scorer = diversity.DiversityScorer(ix, 5)
        draws = diversity.per_image_draws(sizes, list(range(I)), top_n, 2019)
        plan = scorer.plan(draws, sizes)
        seg = torch.tensor(bounds, dtype=torch.int32).to(dev)
        out_i = torch.empty(plan["n_sets"], ops.DIV_COLS + 5, dtype=torch.int32, device=dev)
        out_d = torch.empty(plan["n_sets"], 6, dtype=torch.float64, device=dev)
        for _ in range(3):
            per = scorer.score(seq, bounds, score, draws)
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            scorer.enqueue(seq, score, seg, I, plan, 0, out_i, out_d)
            e1.record()
            e1.synchronize()
            ev.append(e0.elapsed_time(e1))
            t = time.perf_counter()
            scorer.score(seq, bounds, score, draws)
            wall.append(1e3 * (time.perf_counter() - t))
        s = diversity.summarize(per)
        lines.append(f"{name}: decode batch {rows} rows, {plan['n_sets']} sets, {plan['n_draw']} drawn rows"
                     f" (sizes: {key}={','.join(str(x) for x in sizes) if len(set(sizes)) > 1 else f'{sizes[0]}x{len(sizes)}'})")
        lines.append(f"    decode (sample_images, wall ms, {len(dec)} runs):     {q(dec)}")
        lines.append(f"    scoring device ms (events, {a.reps} runs):           {q(ev)}")
        lines.append(f"    scoring wall ms incl. the host copy ({a.reps} runs): {q(wall)}")
        lines.append(f"    scoring / decode (medians): {statistics.median(wall) / statistics.median(dec):.4f};  summary: "
                     + ", ".join(f"{k} {['%.4g' % x for x in v]}" for k, v in s.items() if k != "printed"))
        del m
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
