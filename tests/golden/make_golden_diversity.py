#!/usr/bin/env python
"""Write the diversity fixture by RUNNING THE REFERENCE's own program, misc/diversity/diversity_score.py (run with runpy where the
reference lies, never copied): diversity_case.npz + diversity_meta.json.  Data only: synthetic captions as id rows, scores, training
caption strings, the draws, per-image expectations, the sentence BLEU-4 values and the numbers the script prints.

    python tests/golden/make_golden_diversity.py

The script is run twice, with and without --evaluate_mB4, on a generated captions file and generated MRNN_split_dict.npy /
all_caption_dict.pkl in a temporary directory laid out as its relative paths expect.  Its Java tokenizer is replaced by a stand-in
`ptbtokenizer` module put first on sys.path that returns every caption string unchanged -- sound because the model's captions are
lower-case words joined by single spaces already.  Word i is the string "w<i>", ids 1 .. V are the model's vocabulary.

What is recorded besides the printed numbers: the draws (the same legacy numpy stream, same seed and call order; checked below against
the per-image arrays the script leaves in its globals), per image the integer counts behind every ratio, and per image the sentence
BLEU-4 values from the reference's `Bleu(4).compute_score` called directly (their means are checked against the script's `img_b4`)."""
import contextlib
import io
import json
import os
import pickle
import re
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SCRIPT_DIR = os.path.join(REF, "misc", "diversity")

V, T, N_BEST, TOP_N, SEED = 14, 16, 5, (20, 100), 2019
SUBS = [5, 7, 2, 3, 20, 21, 100, 120, 400, 5, 20, 100]
STUB = "class PTBTokenizer:\n    def tokenize(self, d):\n        return {k: [c['caption'] for c in v] for k, v in d.items()}\n"


def sent(ids):
    return " ".join(f"w{int(x)}" for x in ids)


def make_captions(rng):
    pool = [[int(x) for x in rng.integers(1, V + 1, size=int(rng.integers(7, 12)))] for _ in range(5)]
    images, scores = [], []
    for i, n in enumerate(SUBS):
        mine = [pool[int(j)] for j in rng.choice(len(pool), 2, replace=False)]
        caps = []
        for _ in range(n):
            t = mine[int(rng.integers(2))]
            a = int(rng.integers(0, 3))
            c = list(t[a:a + int(rng.integers(1, len(t) + 1))])
            if rng.random() < 0.3:
                c[int(rng.integers(len(c)))] = int(rng.integers(1, V + 1))
            caps.append(c)
        images.append(caps)
        while True:
            sc = rng.random(n).astype(np.float32)
            if len(np.unique(sc)) == n:                          # pairwise distinct: ties are the device's to define
                break
        scores.append(sc)
    edges = {}
    # image 0 (5 captions: every draw is the whole image and the selection is all of it)
    images[0] = [[], [3], [int(x) for x in rng.integers(1, V + 1, size=T)], [3, 1, 2], [3, 1, 2, 5, 6]]
    edges["empty_caption_selected"] = [0, 0]
    edges["one_word_caption"] = [0, 1]
    edges["full_length_caption"] = [0, 2]
    edges["closest_length_tie"] = [0, 3]                       # 3 words against references of 1 and 5 (and 0, 16): the shorter, 1
    # image 1 (7 captions, the draw is the whole image): the best five have 4, 6, 7, 8, 9 words out of one template
    t = [2, 4, 6, 8, 10, 12, 1, 3, 5]
    images[1] = [t[:4], t[:6], t[:7], t[:8], t[:9], t[:6], [7, 7]]
    scores[1] = np.asarray([0.9, 0.8, 0.7, 0.6, 0.5, 0.2, 0.1], np.float32)
    edges["shorter_than_every_reference"] = [1, 0]             # 4 words, closest reference 6: brevity factor on a non-zero value
    edges["closest_length_tie_2"] = [1, 2]                     # 7 words against 6 and 8
    edges["duplicates_in_a_draw"] = [1, 1, 5]
    # image 2 (2 captions)
    images[2] = [[1, 2], [4, 5, 6]]
    edges["equals_double_space_train_caption_if_split_wrongly"] = [2, 0]
    train = {
        "101": [sent([3, 1, 2]), "W3 W1 w2 W5 w6.", ".", "w1  w2", "w4 w5 zebra", "w4 w5 w6 "],
        "102": [sent(images[4][0]), sent(images[6][3]).upper() + "."],
        "103": [sent(c) for c in images[8][:40]],
        "900": [sent([4, 5, 6]), sent(t[:7])],                   # a validation image: its captions are NOT training captions
    }
    split = {101: "train", 102: "train", 103: "train", 900: "val"}
    edges["train_equal"] = sent([3, 1, 2])
    edges["train_equal_after_lower_and_dot"] = ["W3 W1 w2 W5 w6.", sent([3, 1, 2, 5, 6])]
    edges["train_empty_after_dot"] = "."
    edges["train_double_space_dropped"] = "w1  w2"
    edges["train_out_of_vocabulary_dropped"] = "w4 w5 zebra"
    edges["train_trailing_space_dropped"] = "w4 w5 w6 "
    edges["only_in_a_validation_image"] = sent([4, 5, 6])
    return images, scores, train, split, edges


def run_script(tmp, captions_file, with_mb4):
    argv, cwd = sys.argv, os.getcwd()
    sys.argv = ["diversity_score.py", "--input_file", captions_file] + (["--evaluate_mB4"] if with_mb4 else [])
    os.chdir(os.path.join(tmp, "misc", "diversity"))
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            g = runpy.run_path(os.path.join(SCRIPT_DIR, "diversity_score.py"), run_name="__main__")
    finally:
        sys.argv = argv
        os.chdir(cwd)
    printed = [float(m.group(1)) for m in re.finditer(r"^(?:m-BLEU-4|1-gram|2-gram|Novel|Distinct)[^\n]*sentences: (\S+)$", buf.getvalue(), flags=re.M)]
    assert len(printed) == (10 if with_mb4 else 8), buf.getvalue()[-2000:]
    return printed, g


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    rng = np.random.default_rng(20241017)
    images, scores, train, split, edges = make_captions(rng)
    strings = [[sent(c) for c in caps] for caps in images]
    preds = [{"image_id": 5000 + i, "caption": strings[i], "subgraph_score": scores[i]} for i in range(len(SUBS))]
    train_set = set(s.lower().replace(".", "") for k, v in split.items() if v == "train" for s in train[str(k)])
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "misc", "diversity"))
        os.makedirs(os.path.join(tmp, "data"))
        os.makedirs(os.path.join(tmp, "stub"))
        with open(os.path.join(tmp, "stub", "ptbtokenizer.py"), "w") as f:
            f.write(STUB)
        np.save(os.path.join(tmp, "data", "MRNN_split_dict.npy"), split)
        with open(os.path.join(tmp, "misc", "diversity", "all_caption_dict.pkl"), "wb") as f:
            pickle.dump(train, f)
        cap_file = os.path.join(tmp, "captions.npy")
        np.save(cap_file, preds)
        sys.path[:0] = [os.path.join(tmp, "stub"), SCRIPT_DIR]
        runs = {}
        for name, with_mb4 in (("mb4", True), ("plain", False)):
            runs[name] = run_script(tmp, cap_file, with_mb4)
        from bleu import Bleu

        arrays, meta_runs = {}, {}
        nt, n_img = len(TOP_N), len(SUBS)
        for name, with_mb4 in (("mb4", True), ("plain", False)):
            printed, g = runs[name]
            rs = np.random.RandomState(SEED)
            exp = np.zeros((n_img, nt, 7), np.int64)              # drawn, distinct, words, unigrams, bigrams, novel, novel_of
            bleu = np.full((n_img, nt, N_BEST), np.nan)
            chosen = np.full((n_img, nt, N_BEST), -1, np.int64)
            for metric in (4, 3, 2, 1):
                if metric == 4 and not with_mb4:
                    continue
                flat, off = [], [0]
                for i, n in enumerate(SUBS):
                    for t, k in enumerate(TOP_N):
                        ind = rs.choice(n, min(k, n), replace=False)
                        flat.append(ind)
                        off.append(off[-1] + len(ind))
                        best = ind[np.argsort(scores[i][ind])[::-1][:N_BEST]]
                        sel = [strings[i][j] for j in best]
                        if metric == 1:
                            drawn = [strings[i][j] for j in ind]
                            exp[i, t, 0], exp[i, t, 1] = len(drawn), len(set(drawn))
                            assert g["uniqueness"][t, i] == exp[i, t, 1] / float(exp[i, t, 0])
                        elif metric == 2:
                            exp[i, t, 5], exp[i, t, 6] = sum(1 for s in sel if s not in train_set), len(sel)
                        elif metric == 3:
                            sp = [s.split(" ") for s in sel]
                            words = [w for l in sp for w in l]
                            pairs = [(l[j], l[j + 1]) for l in sp for j in range(len(l) - 1)]
                            exp[i, t, 2], exp[i, t, 3], exp[i, t, 4] = len(words), len(set(words)), len(set(pairs))
                            assert g["n_gram"][t, 0, i] == exp[i, t, 3] / float(exp[i, t, 2])
                            assert g["n_gram"][t, 1, i] == exp[i, t, 4] / float(exp[i, t, 2])
                        else:
                            chosen[i, t, :len(best)] = best
                            for q, s in enumerate(sel):
                                with contextlib.redirect_stdout(io.StringIO()):
                                    _, per, _ = Bleu(4).compute_score({"x": [r for j, r in enumerate(sel) if j != q]}, {"x": [s]})
                                bleu[i, t, q] = per[3][0]
                            assert g["img_b4"][t][i] == np.mean(np.array(list(bleu[i, t, :len(sel)])))
                arrays[f"draws_{name}_{metric}"] = np.concatenate(flat).astype(np.int32)
                arrays[f"draws_off_{name}_{metric}"] = np.asarray(off, np.int32)
            assert [int(exp[:, t, 5].sum()) for t in range(nt)] == [int(x) for x in g["novel_cnt"]]
            arrays[f"exp_{name}"] = exp
            if with_mb4:
                arrays["bleu4"], arrays["selected"] = bleu, chosen
            meta_runs[name] = {"printed": printed}
        p = runs["mb4"][0]
        assert p[0] > 0.05 and p[1] > 0.05, ("mBLEU means", p[:2])
        assert p[8] < 1 and p[9] < 1, ("Distinct ratios", p[8:])
        assert runs["mb4"][0][2:] != runs["plain"][0]            # the draws of metrics 3, 2, 1 depend on --evaluate_mB4
    rows = sum(SUBS)
    seq = np.zeros((rows, T), np.int16)
    r = 0
    for caps in images:
        for c in caps:
            seq[r, :len(c)] = c
            r += 1
    np.savez_compressed(os.path.join(HERE, "diversity_case.npz"), seq=seq, bounds=np.concatenate([[0], np.cumsum(SUBS)]).astype(np.int64),
                        score=np.concatenate(scores).astype(np.float32), **arrays)
    with open(os.path.join(HERE, "diversity_meta.json"), "w") as f:
        json.dump({"V": V, "T": T, "n_best": N_BEST, "top_n": list(TOP_N), "seed": SEED, "sub_nums": SUBS, "runs": meta_runs,
                   "train": [s for k, v in split.items() for s in train[str(k)] if v == "train"], "edges": edges}, f, indent=1)
    print("wrote diversity_case.npz / diversity_meta.json:", rows, "captions;", {k: v["printed"] for k, v in meta_runs.items()})


if __name__ == "__main__":
    main()
