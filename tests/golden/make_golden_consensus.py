#!/usr/bin/env python
"""Write the consensus re-ranking fixture by RUNNING THE REFERENCE's CiderScorer (pure Python + numpy; imported from where the
reference lies, never copied): consensus_case.npz + consensus_meta.json.  Data only: a synthetic corpus as id arrays, candidate token
rows, neighbour lists, k, m, and the reference's pair scores, sums and orders in float64.

    python tests/golden/make_golden_consensus.py

The scorer is built directly (`scorer += (refs[0], refs)` per corpus image, then `compute_doc_freq()`): eval_pair_cider.py and
consensus_reranking.py pull in the Java tokenizer, pycocotools and scipy, so the neighbour / sort / sum-top-m / argsort loop of
`consensus_rerank` (consensus_reranking.py:152-174) is restated below.  Word i is the string "w<i>"; ids 1 .. V are the model's
vocabulary, larger ids are words only the corpus knows.  Corpus ids are Zipf-distributed so n-grams repeat."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "misc", "consensus_reranking", "external", "coco_caption_patch_mRNN_cr"))

V, OOV_HI = 200, 260          # model vocabulary 1 .. V; corpus-only words V+1 .. OOV_HI
CORPUS_LO_HI = 149            # corpus draws model words from 1 .. 149: 150 .. 200 never occur in it
N_IMG, T, K, M = 300, 20, 30, 125


def zipf_ids(rng, n, pool):
    r = np.minimum(rng.zipf(1.3, size=n), len(pool)) - 1
    return [int(pool[i]) for i in r]


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    from cider_scorer_compute_sentence import CiderScorer
    rng = np.random.default_rng(20240917)
    pool = np.concatenate([np.arange(2, CORPUS_LO_HI + 1), np.arange(V + 1, OOV_HI + 1)])
    pool = pool[rng.permutation(len(pool))]
    corpus = []
    for i in range(N_IMG):
        ncap = 3 if i < 40 else int(rng.integers(3, 8))          # images 0 .. 39 have exactly 3 captions (the "< m" neighbourhood)
        caps = []
        for c in range(ncap):
            L = int(rng.integers(0, 31))
            s = zipf_ids(rng, L, pool)
            if c == 0:
                s = [1] + s[:29]                                     # word 1 occurs in every image: its unigram weight is 0
            caps.append(s)
        corpus.append(caps)
    corpus[50][1] = []                                               # an empty neighbour caption
    corpus[50][2] = [7]                                              # a one-word caption
    corpus[51][1] = zipf_ids(rng, 57, pool)                          # long captions (COCO has 50+ word ones)
    corpus[52][2] = zipf_ids(rng, 64, pool)

    # the images to re-rank: (candidates, neighbour list)
    sizes = [10, 7, 1, 12, 5, 8]
    nn = np.zeros((len(sizes), K + 4), np.int64)                     # lists longer than k: only the first k count
    for i in range(len(sizes)):
        nn[i] = rng.choice(np.arange(60, N_IMG), K + 4, replace=False)
    nn[0, :3] = [50, 51, 52]
    nn[2] = rng.choice(np.arange(0, 40), K + 4, replace=False)       # 30 neighbours x 3 captions = 90 < m
    cands = []
    for i, n in enumerate(sizes):
        rows = []
        neigh = [c for j in nn[i, :K] for c in corpus[j] if len(c) >= 4]
        for c in range(n):
            src = [w for w in neigh[int(rng.integers(len(neigh)))] if w <= V]
            a = int(rng.integers(0, max(1, len(src) - 3)))
            s = src[a:a + int(rng.integers(3, 12))] + zipf_ids(rng, int(rng.integers(0, 6)), np.arange(1, CORPUS_LO_HI + 1))
            rows.append(s[:T])
        cands.append(rows)
    edges = {}
    cands[0][0] = []; edges["empty_candidate"] = [0, 0]
    cands[0][1] = [7]; edges["one_word_candidate"] = [0, 1]
    cands[0][5] = list(cands[0][2]); edges["duplicate_candidates"] = [0, 2, 5]
    cands[0][3] = [150, 151, 152, 153, 154] + cands[0][3][:6]; edges["unseen_ngrams_candidate"] = [0, 3]
    cands[0][4] = [1] + cands[0][4][:10]; edges["weight_zero_unigram_candidate"] = [0, 4]
    cands[3][7] = list(cands[3][1]); cands[3][9] = list(cands[3][1])
    edges["fewer_than_m_image"] = 2
    edges["empty_neighbour_caption"] = [0, 50, 1]                    # image, corpus image, caption
    edges["one_word_neighbour_caption"] = [0, 50, 2]
    edges["long_captions"] = [[51, 1], [52, 2]]

    scorer = CiderScorer(n=4, sigma=6.0)
    for caps in corpus:
        refs = [" ".join(f"w{x}" for x in c) for c in caps]
        scorer += (refs[0], refs)
    scorer.compute_doc_freq()

    rows = sum(sizes)
    max_caps = 0
    pair_rows, sums, orders = [], [], []
    for i, n in enumerate(sizes):
        ret = []
        for j in range(K):
            ret += corpus[int(nn[i, j])]
        max_caps = max(max_caps, len(ret))
        sim = []
        for c in cands[i]:
            b = [scorer.compute_cider_sen_pair(" ".join(f"w{x}" for x in c), " ".join(f"w{x}" for x in r)) for r in ret]
            pair_rows.append(list(b))
            b.sort(reverse=True)
            sim.append(sum(b[:M]))
        sums += sim
        orders += np.argsort(-np.array(sim)).tolist()
    pairs = np.full((rows, max_caps), -1.0)
    for r, b in enumerate(pair_rows):
        pairs[r, :len(b)] = b
    seq = np.zeros((rows, T), np.int64)
    r = 0
    for rows_i in cands:
        for c in rows_i:
            seq[r, :len(c)] = c
            r += 1
    flat = [w for caps in corpus for c in caps for w in c]
    lens = [len(c) for caps in corpus for c in caps]
    np.savez_compressed(os.path.join(HERE, "consensus_case.npz"),
                        corpus_words=np.asarray(flat, np.int32), corpus_woff=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                        corpus_cap_off=np.concatenate([[0], np.cumsum([len(c) for c in corpus])]).astype(np.int64),
                        cand=seq, bounds=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), nn=nn,
                        pairs=pairs, sums=np.asarray(sums, np.float64), orders=np.asarray(orders, np.int64),
                        df_check=np.asarray([scorer.document_frequency[("w1",)], scorer.document_frequency[("w150",)]], np.float64))
    with open(os.path.join(HERE, "consensus_meta.json"), "w") as f:
        json.dump({"V": V, "k": K, "m": M, "T": T, "n_img": N_IMG, "edges": edges,
                   "spot": {"empty_vs_123": scorer.compute_cider_sen_pair("", "w1 w2 w3"), "w7_vs_w7": scorer.compute_cider_sen_pair("w7", "w7"),
                            "12_vs_empty": scorer.compute_cider_sen_pair("w1 w2", "")}}, f, indent=1)
    print("wrote consensus_case.npz / consensus_meta.json:", rows, "candidates,", max_caps, "neighbour captions at most")


if __name__ == "__main__":
    main()
