#!/usr/bin/env python3
"""Grounding scores of one decode batch (subgc_grounding_material + subgc_grounding_score with the upload of the boxes and the copy back,
subgc.grounding) next to the decode that produces the batch, and the reference evaluator's CPU time over the same material.

    python tools/grounding_bench.py [--out profiles/r12_grounding_bench.txt] [--reps 30]
    python tools/grounding_bench.py --script-only [--images 256]                 (no GPU; where the reference lies)

Shape: 256 images x <= 10 captions (test.sh, Karpathy sub-graph setting), 36 boxes and 5 annotated reference captions of <= 4 objects per
image.  The chosen caption of every image has the decode batch's row layout but its words are drawn over a 40-word vocabulary in which
three words in four name one of 30 detection classes, and every word attends to a random box (a randomly initialised decoder emits word
salad).  Reference objects copy a box of the image, shifted now and then, so hits, misses, excused and hallucinated words all occur.
Method: warmed up, then timed `reps` times; device time = HIP events around the uploads and the two launches, wall = host clock around
uploads + launches + the device -> host copy + unpack; median, min and max are reported.  The decode is timed in the same process, same
box: host clock around sample_images(return_att=1) + synchronise.
--script-only runs the reference's own `FlickrGrdEval.grd_eval` (imported from where the reference lies) in modes 'all' and 'loc' over
the same material written as JSON files, with a DICTIONARY stand-in for Stanford CoreNLP: this leaves out the Java calls -- one per
token of every reference caption and one per predicted class word without a match, in both runs -- so it understates the reference
by far."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

REF_GROUNDING = "/root/reference/misc/grounding"
V, C, T, N_BOX, N_REFS = 40, 30, 20, 36, 5
STUB = ("import json\nclass StanfordCoreNLP:\n    def __init__(self, *a, **k):\n        pass\n    def annotate(self, text, properties=None):\n"
        "        return json.dumps({'sentences': [{'tokens': [{'lemma': text[:-1] if text.endswith('s') else text}]}]})\n"
        "    def close(self):\n        pass\n")


def world():
    vocab = {str(i): f"w{i}" for i in range(1, V + 1)}
    wd_to_lemma = {f"w{i}": f"l{i}" for i in range(1, V + 1)}
    lemma_det = {f"l{i}": i for i in range(1, C + 1)}
    det_wd = {i: (f"c{i}s" if i % 5 == 0 else f"c{i}") for i in range(1, C + 1)}
    lemmatize = lambda t: t[:-1] if t.endswith("s") else t  # noqa: E731
    return vocab, wd_to_lemma, lemma_det, det_wd, lemmatize


def make_case(sizes, seed):
    """Per image: boxes, the ranked token rows of its captions, the arg-max box of every word of caption 0, and its annotations."""
    rng = np.random.default_rng(seed)
    det_wd = world()[3]
    boxes, rows, nodes, anns = [], [], [], []
    for i, n in enumerate(sizes):
        xy = rng.random((N_BOX, 2)) * 300
        b = np.concatenate([xy, xy + 10 + rng.random((N_BOX, 2)) * 200], 1).astype(np.float32)
        boxes.append(b)
        mine = np.zeros((n, T), np.int64)
        for r in range(n):
            L = int(rng.integers(4, T + 1))
            mine[r, :L] = rng.integers(1, V + 1, size=L)
        rows.append(mine)
        nodes.append(rng.integers(0, N_BOX, size=T + 1).astype(np.int32))
        caps = []
        for _ in range(N_REFS):
            n_tok = int(rng.integers(6, 15))
            pos = sorted(int(x) for x in rng.permutation(n_tok)[:int(rng.integers(0, 5))])
            toks = [f"c{int(rng.integers(1, C + 1))}" if rng.random() < 0.2 else f"t{int(rng.integers(1, 50))}" for _ in range(n_tok)]
            obj = [b[int(rng.integers(N_BOX))].astype(np.float64) + (0 if rng.random() < 0.6 else 35) for _ in pos]
            caps.append({"tokens": toks, "process_idx": pos, "process_clss": [det_wd[int(rng.integers(1, C + 1))] for _ in pos],
                         "process_bnd_box": [o.tolist() for o in obj]})
        anns.append({"image_id": 1000 + i, "captions": caps})
    return boxes, rows, nodes, anns


def host_material(rows, nodes, boxes):
    """The {'clss','idx_in_sent','bbox'} entry of caption 0, as misc/grd_utils.py:49-60 fills it."""
    _, wd_to_lemma, lemma_det, det_wd, _ = world()
    out = {"clss": [], "idx_in_sent": [], "bbox": []}
    if len(rows) == 0:
        return out
    for j, x in enumerate(rows[0]):
        if x <= 0:
            break
        lemma = wd_to_lemma[f"w{int(x)}"]
        if lemma in lemma_det:
            out["clss"].append(det_wd[lemma_det[lemma]]); out["idx_in_sent"].append(j); out["bbox"].append(boxes[int(nodes[j])].astype(np.float64).tolist())
    return out


def script_time(n_images, seed):
    sizes = [10] * n_images
    boxes, rows, nodes, anns = make_case(sizes, seed)
    results = {str(a["image_id"]): [host_material(rows[i], nodes[i], boxes[i])] for i, a in enumerate(anns)}
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "stanfordcorenlp.py"), "w") as f:
            f.write(STUB)
        sys.path[:0] = [REF_GROUNDING, tmp]
        sys.dont_write_bytecode = True
        from eval_grd_flickr30k_entities import FlickrGrdEval
        paths = [os.path.join(tmp, n) for n in ("reference.json", "split.json", "submission.json")]
        for p, obj in zip(paths, ({"annotations": anns}, {"val": [str(a["image_id"]) for a in anns]}, {"results": results})):
            with open(p, "w") as f:
                json.dump(obj, f)
        spent, numbers = {}, {}
        for mode in ("all", "loc"):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                ev = FlickrGrdEval(reference_file=paths[0], submission_file=paths[2], split_file=paths[1], val_split=["val"], iou_thresh=0.5)
                numbers[mode] = [float(x) for x in ev.grd_eval(mode=mode)]
            spent[mode] = time.perf_counter() - t0
    n_obj = sum(len(c["process_idx"]) for a in anns for c in a["captions"])
    n_pred = sum(len(r[0]["clss"]) for r in results.values())
    return (f"reference evaluator on this CPU: {n_images} images, {N_REFS} reference captions each ({n_obj} objects), {n_pred} predicted words: "
            f"{sum(spent.values()):.2f} s (mode all {spent['all']:.2f}, mode loc {spent['loc']:.2f}; F1_all {numbers['all'][2]:.4f}, F1_loc "
            f"{numbers['loc'][2]:.4f}) -- with a dictionary in the place of Stanford CoreNLP: the Java calls (one per reference token and per unmatched "
            "class word, in both runs) are left out, so this understates the reference")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_grounding_bench.txt"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--script-only", action="store_true", help="only time the reference's evaluator on the CPU (needs no GPU, needs the reference)")
    a = ap.parse_args()
    if a.script_only:
        assert os.path.isdir(REF_GROUNDING), "--script-only needs the reference's misc/grounding"
        line = script_time(a.images, 100)
        print(line)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        return

    import torch
    import bench
    import subgc.models as models
    from subgc import grounding, ops, synthetic
    assert torch.cuda.is_available(), "grounding_bench needs the MI355X (or --script-only)"
    dev = torch.device("cuda:0")
    vocab, wd_to_lemma, lemma_det, det_wd, lemmatize = world()
    I = a.images
    q = lambda x: f"median {statistics.median(x):.3f} (min {min(x):.3f}, max {max(x):.3f})"  # noqa: E731
    torch.manual_seed(0)
    m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, gpn_nms_thres=0.75, gpn_max_subg=10))).to(dev).eval()
    images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(50, seed=700 + i).items()} for i in range(I)]
    sopt = dict(sample_max=1, beam_size=1, return_att=1)
    for _ in range(2):
        hold = {}
        m.sample_images(images, opt=sopt, batch_out=hold)
    torch.cuda.synchronize()
    dec = []
    for _ in range(max(5, a.reps // 4)):
        t = time.perf_counter()
        m.sample_images(images, opt=sopt, batch_out={})
        torch.cuda.synchronize()
        dec.append(1e3 * (time.perf_counter() - t))
    bounds = [int(x) for x in hold["bounds"]]
    sizes = [b - x for x, b in zip(bounds, bounds[1:])]
    boxes, rows, nodes, anns = make_case(sizes, 100)
    refs = grounding.GroundingReferences(anns, [x["image_id"] for x in anns], det_wd, wd_to_lemma, lemma_det, vocab, lemmatize, device=dev)
    sc = grounding.GroundingScorer(refs)
    index = list(range(I))
    plan = sc.plan(index)
    seq = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(dev)
    node = torch.from_numpy(np.stack(nodes)).to(dev)
    n_words = torch.from_numpy(np.array([int((r[0] > 0).sum()) if len(r) else 0 for r in rows], np.int32)).to(dev)
    box_off = np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int32)
    flat = np.concatenate(boxes).ravel()
    arena = torch.empty(sc.arena_words(plan), dtype=torch.int32, device=dev)

    def once():
        tab = ops.upload(np.concatenate([np.asarray(bounds, np.int32), plan["table"], box_off]), torch.int32, dev)
        d_box = ops.upload(flat, torch.float32, dev)
        sc.enqueue(seq, tab, None, I, node, T + 1, n_words, tab[I + 1:], d_box, len(flat) // 4, 0, arena, plan)

    for _ in range(3):
        once()
        per = sc.unpack(arena.cpu().numpy(), plan)
    want = [host_material(rows[i], nodes[i], boxes[i]) for i in range(I)]
    assert all([refs.class_names[c] for c in p["clss"]] == w["clss"] and p["idx_in_sent"].tolist() == w["idx_in_sent"] for p, w in zip(per, want))
    ev, wall = [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        once()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
        t = time.perf_counter()
        once()
        per = sc.unpack(arena.cpu().numpy(), plan)
        wall.append(1e3 * (time.perf_counter() - t))
    s = grounding.summarize(per, refs)
    lines = [f"grounding bench: material + score over one decode batch; {I} images x <= 10 captions ({bounds[-1]} rows), {N_BOX} boxes and {N_REFS} "
             f"reference captions per image ({plan['P']} pairs, {plan['n_rec']} objects, {sum(len(p['clss']) for p in per)} predicted words)",
             f"    decode (sample_images with return_att, wall ms, {len(dec)} runs): {q(dec)}",
             f"    uploads + two launches, device ms (events, {a.reps} runs):       {q(ev)}",
             f"    uploads + launches + host copy + unpack, wall ms ({a.reps} runs): {q(wall)}",
             f"    scoring / decode (medians): {statistics.median(wall) / statistics.median(dec):.4f};  summary: "
             + ", ".join(f"{k} {s[k]:.4g}" for k in grounding.NAMES) + f"; num_vocab {s['num_vocab']}"]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
