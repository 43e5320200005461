#!/usr/bin/env python
"""Write the accuracy fixture by RUNNING THE REFERENCE's own scorers where the reference lies (never copied): accuracy_case.npz +
accuracy_meta.json.  Data only: synthetic captions and references as id rows, per row the BLEU material and the six values, per image
and oracle_num the oracle picks and maxima, the corpus numbers, and the host tables (document frequencies, BLEU max counts).

    python tests/golden/make_golden_accuracy.py

What runs: pycocoevalcap's `Bleu(4).compute_score`, `Rouge().compute_score` and `Cider().compute_score` once per caption position on the
captions of that position, short images padded with their first caption -- exactly the loop of misc/sentence_utils.py:language_eval
behind eval_utils.py:176-189 -- then `np.argmax` / `np.max` / `np.mean` over the positions and misc/sentence_utils.py:cal_bleu over the
picks, as language_eval does.  `CiderScorer` and `cook_refs` are also called directly for the document frequencies and the max counts.
Word i is the string "w<i>"; ids 1 .. V are the model's vocabulary, larger ids occur in references only (numbered by first appearance,
as subgc.consensus.build_id_map numbers them).

The device takes its arg-max over its own fp64 values, so the fixture must hold no near-tie: for every image, BLEU order and
oracle_num the best sentence value and the best DIFFERENT value are asserted to lie more than 1e-9 relative apart (a zero best value
means every value is zero and the pick is row 0; exact duplicates give equal bits on both sides and the lower index).  The smallest
gap is recorded in the meta file."""
import contextlib
import io
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

V, T, SEED = 40, 64, 20241018
ORACLE_NUMS = (1, 5, 20, 1000)
N_IMG = 40


def sent(ids):
    return " ".join(f"w{int(x)}" for x in ids)


def make_case(rng):
    zipf = 1.0 / np.arange(1, V - 4)                                       # words 2 .. V - 4; 1 goes into every image; V-2 .. V never into a reference
    zipf /= zipf.sum()

    def draw(n):
        return [int(x) + 2 for x in rng.choice(len(zipf), size=n, p=zipf)]

    refs, cands, edges = [], [], {}
    for i in range(N_IMG):
        R = int(rng.integers(2, 6))
        mine = [draw(int(rng.integers(6, 15))) for _ in range(R)]
        # a few words outside the model's vocabulary
        for r in mine:
            if rng.random() < 0.3:
                r[int(rng.integers(len(r)))] = V + 1 + int(rng.integers(0, 12))
        n = int(rng.integers(4, 31))
        caps = []
        for _ in range(n):
            src = mine[int(rng.integers(R))]
            a = int(rng.integers(0, 3))
            c = [w if w <= V else 2 for w in src[a:a + int(rng.integers(2, len(src) + 1))]]
            u = rng.random()
            if u < 0.35:
                c[int(rng.integers(len(c)))] = int(rng.integers(2, V + 1))
            elif u < 0.5:
                p = int(rng.integers(len(c)))
                c[p:p] = [c[p]] * int(rng.integers(1, 3))                  # repeated words: clipping bites
            elif u < 0.6:
                c = c + draw(int(rng.integers(1, 6)))
            caps.append(c[:T])
        refs.append(mine)
        cands.append(caps)
    # image 0: the empty, the one-word and the 64-word candidate; an empty reference among the references
    refs[0] = [[], draw(9), draw(12)]
    cands[0] = [refs[0][1][:5], [], [refs[0][1][0]], (refs[0][2] * 6)[:T], refs[0][2][2:9]]
    edges["empty_candidate"], edges["one_word_candidate"], edges["full_length_candidate"], edges["empty_reference"] = [0, 1], [0, 2], [0, 3], [0, 0]
    # image 1: ONE reference, and a candidate shorter than it
    refs[1] = [draw(10)]
    cands[1] = [refs[1][0][2:6], refs[1][0][:10], refs[1][0][1:8] + [V]]
    edges["one_reference"], edges["shorter_than_every_reference"] = 1, [1, 0]
    # image 2: SEVEN references; a 7-word candidate against references of 6 and 8 words (closest-length tie: the shorter)
    base = draw(12)
    refs[2] = [base[:6], base[:8], base[2:12], draw(11), draw(13), draw(12), draw(10)]
    cands[2] = [base[:7], base[1:8] + [V], [V - 1, V, V - 2, V - 1], base[:5] + [V]]
    edges["seven_references"], edges["closest_length_tie"], edges["unseen_ngrams"] = 2, [2, 0], [2, 2]
    # image 3: references of 70 (> 64) and of exactly 256 words
    long70, long256 = draw(70), draw(256)
    refs[3] = [long70, long256, draw(9)]
    cands[3] = [long70[:T], long256[100:130], long70[3:20] + [V], (long256[:8] * 8)[:T]]
    edges["reference_over_64_words"], edges["reference_256_words"] = [3, 0], [3, 1]
    # image 4: one candidate; image 5: three (fewer than oracle_num = 5); image 6: 130
    cands[4] = cands[4][:1]
    cands[5] = cands[5][:3]
    pool = cands[6]
    big = []
    for q in range(130):
        c = list(pool[q % len(pool)])
        if q >= len(pool):
            c[int(rng.integers(len(c)))] = int(rng.integers(2, V + 1))
            if rng.random() < 0.5:
                c = c[:max(1, len(c) - int(rng.integers(0, 3)))]
        big.append(c)
    cands[6] = big
    edges["one_candidate"], edges["fewer_than_oracle_num"], edges["many_candidates"] = 4, 5, 6
    # image 7: exact duplicates, among them the best candidate
    cands[7] = [cands[7][0], list(refs[7][0][:9]), cands[7][1], list(refs[7][0][:9]), cands[7][0]] + cands[7][2:]
    refs[7][0] = [w if w <= V else 3 for w in refs[7][0]]
    cands[7][1] = cands[7][3] = list(refs[7][0][:9])
    edges["duplicate_candidates"] = [7, 1, 3]
    # image 8: repeated words against a reference that holds the word twice
    refs[8][0] = [5, 5, 6, 7, 8, 9, 10]
    cands[8][0] = [5, 5, 5, 5, 6, 7]
    edges["clipped_repeats"] = [8, 0]
    # a unigram in every image: log df = log(#images), weight 0
    for i in range(N_IMG):
        refs[i][-1].append(1)                                              # draw() never yields word 1; no last reference is the 256-word one
    edges["word_in_every_image"] = 1
    cands[9][0] = [1] + cands[9][0][:6]
    # number the reference-only words by first appearance above V
    fresh = {}
    for caps in refs:
        for cap in caps:
            for p, w in enumerate(cap):
                if w > V:
                    cap[p] = fresh.setdefault(w, V + 1 + len(fresh))
    return refs, cands, edges


def key_of(ngram):
    k = 0
    for j, w in enumerate(ngram):
        k |= int(w[1:]) << (48 - 16 * j)
    return k


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    rng = np.random.default_rng(SEED)
    case = make_case(rng)
    separate(case, rng)
    assert attempt(SEED, case), "a near-tie is left"


def sentence_bleu(c, refs):
    """The four sentence values of one candidate, written out here only to FIND near-ties quickly (the recorded numbers all come from the
    reference's scorers below, which also check that none is left)."""
    def grams(x):
        out = {}
        for k in range(1, 5):
            for i in range(len(x) - k + 1):
                out[tuple(x[i:i + k])] = out.get(tuple(x[i:i + k]), 0) + 1
        return out
    cc, rc = grams(c), [grams(r) for r in refs]
    correct = [0] * 4
    for g, n in cc.items():
        correct[len(g) - 1] += min(n, max(r.get(g, 0) for r in rc))
    reflen = min((abs(len(r) - len(c)), len(r)) for r in refs)[1]
    vals, prod = [], 1.0
    for k in range(4):
        prod *= (correct[k] + 1e-15) / (max(0, len(c) - k) + 1e-9)
        vals.append(prod ** (1.0 / (k + 1)))
    ratio = (len(c) + 1e-15) / (reflen + 1e-9)
    return [v * math.exp(1 - 1 / ratio) for v in vals] if ratio < 1 else vals


def separate(case, rng):
    """Where the best sentence BLEU of an image and the best different one lie within 1e-7 relative, the runner-up gets unseen words."""
    refs, cands, _ = case
    for i in range(N_IMG):
        for _ in range(400):
            vals = np.array([sentence_bleu(c, refs[i]) for c in cands[i]])
            bad = None
            for N in ORACLE_NUMS:
                for k in range(4):
                    col = vals[:N, k]
                    others = col[col != col.max()]
                    if col.max() > 0 and len(others) and (col.max() - others.max()) / col.max() <= 1e-7:
                        bad = int(np.flatnonzero(col == others.max())[0])
            if bad is None:
                break
            assert i > 8 or i == 6, ("near-tie in a planted image", i)
            c = cands[i][bad]
            c[int(rng.integers(len(c)))] = V - int(rng.integers(0, 3))
            cands[i][bad] = (c + [V - 1])[:T]
        else:
            raise AssertionError(("cannot separate image", i))


def attempt(seed, case):
    sys.path[:0] = [os.path.join(REF, "misc", "coco-caption"), REF]
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.bleu.bleu_scorer import cook_refs
    from pycocoevalcap.cider.cider import Cider
    from pycocoevalcap.cider.cider_scorer import CiderScorer
    from pycocoevalcap.rouge.rouge import Rouge
    from misc.sentence_utils import cal_bleu

    refs, cands, edges = case
    sizes = [len(c) for c in cands]
    gts = {1000 + i: [sent(r) for r in refs[i]] for i in range(N_IMG)}
    n_pos = max(sizes)
    names = ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "CIDEr", "ROUGE_L"]
    all_scores = {m: np.zeros((n_pos, N_IMG)) for m in names}
    material = []
    for p in range(n_pos):                                                  # language_eval's loop over the caption positions
        res = {1000 + i: [sent(cands[i][p] if p < sizes[i] else cands[i][0])] for i in range(N_IMG)}
        with contextlib.redirect_stdout(io.StringIO()):
            _, b, mat = Bleu(4).compute_score(gts, res)
            _, c = Cider().compute_score(gts, res)
            _, r = Rouge().compute_score(gts, res)
        for k in range(4):
            all_scores[names[k]][p] = np.array(b[k])
        all_scores["CIDEr"][p], all_scores["ROUGE_L"][p] = c, r
        material.append(mat)
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = int(bounds[-1])
    row_i, row_d = np.zeros((rows, 10), np.int32), np.zeros((rows, 6))
    for i in range(N_IMG):
        for p in range(sizes[i]):
            m = material[p]
            row_i[bounds[i] + p] = [m["testlen"][i], m["reflen"][i]] + [m["guess"][k][i] for k in range(4)] + [m["correct"][k][i] for k in range(4)]
            row_d[bounds[i] + p] = [all_scores[n][p, i] for n in names]
    # top-1: position 0 of every image, the scorers' own corpus numbers
    res0 = {1000 + i: [sent(cands[i][0])] for i in range(N_IMG)}
    with contextlib.redirect_stdout(io.StringIO()):
        b0, _, _ = Bleu(4).compute_score(gts, res0)
        c0, _ = Cider().compute_score(gts, res0)
        r0, _ = Rouge().compute_score(gts, res0)
    top1 = np.array(list(b0) + [c0, r0])
    picks = np.zeros((len(ORACLE_NUMS), N_IMG, 4), np.int32)
    pick_mat = np.zeros((len(ORACLE_NUMS), N_IMG, 4, 10), np.int32)
    best = np.zeros((len(ORACLE_NUMS), N_IMG, 6))
    oracle = np.zeros((len(ORACLE_NUMS), 6))
    gap = np.inf
    for q, N in enumerate(ORACLE_NUMS):
        top_k = min(N, n_pos)                                               # positions past the longest image hold first captions only
        for k in range(4):
            sc = all_scores[names[k]][:top_k]
            best_ind = np.argmax(sc, axis=0)
            oracle[q, k] = cal_bleu(best_ind, material[:top_k])[k]
            picks[q, :, k] = best_ind
            for i in range(N_IMG):
                assert best_ind[i] < sizes[i]
                pick_mat[q, i, k] = row_i[bounds[i] + best_ind[i]]
                col = sc[:, i]
                hi = col.max()
                if hi == 0.0:
                    assert (col == 0.0).all() and best_ind[i] == 0
                    continue
                others = col[col != hi]
                if len(others):
                    g = (hi - others.max()) / hi
                    if not g > 1e-9:
                        print("seed", seed, "near-tie", N, names[k], i, hi, others.max())
                        return False
                    gap = min(gap, g)
        for k, n in enumerate(names):
            best[q, :, k] = np.max(all_scores[n][:top_k], axis=0)
        oracle[q, 4] = np.mean(np.max(all_scores["CIDEr"][:top_k], axis=0))
        oracle[q, 5] = np.mean(np.max(all_scores["ROUGE_L"][:top_k], axis=0))
    # host tables from the reference's own objects
    cs = CiderScorer(n=4, sigma=6.0)
    for i in range(N_IMG):
        cs += (res0[1000 + i][0], gts[1000 + i])
    cs.compute_score()
    df = sorted((key_of(g), float(v)) for g, v in cs.document_frequency.items() if v > 0)
    bkeys, bmax, boff = [], [], [0]
    for i in range(N_IMG):
        _, maxcounts = cook_refs(gts[1000 + i])
        for kk, c in sorted((key_of(g), c) for g, c in maxcounts.items()):
            bkeys.append(kk)
            bmax.append(c)
        boff.append(len(bkeys))
    seq = np.zeros((rows, T), np.int16)
    r = 0
    for caps in cands:
        for c in caps:
            assert len(c) <= T and all(1 <= w <= V for w in c)
            seq[r, :len(c)] = c
            r += 1
    flat = [cap for caps in refs for cap in caps]
    assert max(len(c) for c in flat) == 256 and max(w for c in flat for w in c) < 32768
    np.savez_compressed(
        os.path.join(HERE, "accuracy_case.npz"), seq=seq, bounds=bounds,
        ref_words=np.asarray([w for c in flat for w in c], np.int16),
        ref_woff=np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int32),
        ref_cap_off=np.concatenate([[0], np.cumsum([len(c) for c in refs])]).astype(np.int32),
        row_i=row_i, row_d=row_d, top1=top1, picks=picks, pick_mat=pick_mat, best=best, oracle=oracle,
        df_keys=np.asarray([k for k, _ in df], np.uint64), df=np.asarray([v for _, v in df]), ref_len=np.asarray(float(cs.ref_len)),
        bkeys=np.asarray(bkeys, np.uint64), bmax=np.asarray(bmax, np.int32), boff=np.asarray(boff, np.int32))
    with open(os.path.join(HERE, "accuracy_meta.json"), "w") as f:
        json.dump({"V": V, "T": T, "seed": seed, "oracle_nums": list(ORACLE_NUMS), "sizes": sizes, "names": names, "edges": edges,
                   "smallest_relative_gap": float(gap)}, f, indent=1)
    print("seed", seed)
    print("wrote accuracy_case.npz / accuracy_meta.json:", rows, "rows;", "top-1", top1.tolist(), "oracle", oracle.tolist(), "gap", gap)
    return True


if __name__ == "__main__":
    main()
