#!/usr/bin/env python
"""Write the fixture of consensus re-ranking, method 'bleu', by RUNNING THE REFERENCE's own `calculate_bleu_sentence`
(misc/consensus_reranking/concensus_reranking_utils/bleu_score_util.py:15-61; imported from where the reference lies, never copied):
consensus_bleu_case.npz + consensus_bleu_meta.json.  Data only: a synthetic corpus as id arrays, candidate token rows, neighbour lists,
the parameter sets, and the reference's pair scores, sums and orders in float64.

    python tests/golden/make_golden_consensus_bleu.py

`nltk` is NOT installed where this fixture is made and bleu_score_util.py imports `nltk.util.ngrams`, so a STAND-IN module is registered
before the import (the way make_golden_controllability.py stands in for `munkres`): `ngrams(sequence, n)` = the sliding window of
n-tuples over the sequence, which is what nltk's function yields without padding.  consensus_reranking.py itself pulls in the Java
tokenizer, pycocotools and scipy, so the neighbour / sort / sum-top-m / argsort loop of `consensus_rerank` (:152-172) is restated below,
as make_golden_consensus.py does.  Word i is the string "w<i>"; ids 1 .. V are the model's vocabulary, larger ids are words only the
corpus knows.  Corpus ids are Zipf-distributed so n-grams repeat.

Two parameter sets over the same inputs: A = the defaults of conf_cr.py:45-48 at fixture size (n = 4, fpr = 1.0, m = 175) and
B = (n = 2, fpr = 0.5, m = 20); k = 30 in both.

The generator asserts, and records in the meta, that every adjacent gap in each image's sorted sums is either exactly 0 -- between
identical candidate rows only -- or larger than 1e-6 relative, and that the reference's `np.argsort(-sim)` order differs from the stable
one (lower index first among equal sums) among identical rows only, so a test can judge every position of every order."""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

V, OOV_HI = 200, 260          # model vocabulary 1 .. V; corpus-only words V+1 .. OOV_HI
CORPUS_LO_HI = 149            # corpus draws model words from 2 .. 149: 150 .. 200 never occur in it
N_IMG, T, K = 300, 20, 30
SETS = {"A": {"n": 4, "fpr": 1.0, "m": 175}, "B": {"n": 2, "fpr": 0.5, "m": 20}}
GAP = 1e-6
SEED = 20261019


def stand_in_nltk():
    def ngrams(sequence, n):
        seq = list(sequence)
        return [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    nltk, util = types.ModuleType("nltk"), types.ModuleType("nltk.util")
    util.ngrams = ngrams
    nltk.util = util
    sys.modules["nltk"], sys.modules["nltk.util"] = nltk, util


def zipf_ids(rng, n, pool):
    r = np.minimum(rng.zipf(1.3, size=n), len(pool)) - 1
    return [int(pool[i]) for i in r]


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    stand_in_nltk()
    sys.path.insert(0, os.path.join(REF, "misc", "consensus_reranking", "concensus_reranking_utils"))
    from bleu_score_util import calculate_bleu_sentence
    sys.path.insert(0, os.path.join(ROOT, "sub-gc_amd"))
    from subgc.consensus import bleu_rerank_restatement

    rng = np.random.default_rng(SEED)
    pool = np.concatenate([np.arange(2, CORPUS_LO_HI + 1), np.arange(V + 1, OOV_HI + 1)])
    pool = pool[rng.permutation(len(pool))]
    corpus = []
    for i in range(N_IMG):
        if i < 40:
            ncap = 3                                                  # 30 neighbours x 3 captions = 90: fewer than m = 175
        elif i < 58:
            ncap = 1                                                  # ...
        elif i < 80:
            ncap = 0                                                  # ... at most 18 captions among 30 of the images 40 .. 79: fewer than m = 20
        elif i < 130:
            ncap = 7                                                  # 30 x 7 = 210: more than either m
        else:
            ncap = int(rng.integers(3, 8))
        caps = []
        for c in range(ncap):
            L = int(rng.integers(6, 31)) if 40 <= i < 58 else int(rng.integers(0, 31))
            caps.append(zipf_ids(rng, L, pool))
        corpus.append(caps)
    edges = {}
    corpus[80][1] = []; edges["empty_neighbour_caption"] = [0, 80, 1]                  # image, corpus image, caption
    corpus[80][2] = [7, 8, 9]; edges["three_word_neighbour_caption"] = [0, 80, 2]      # n - 1 words in set A
    corpus[80][3] = [7]; edges["one_word_neighbour_caption"] = [0, 80, 3]              # n - 1 words in set B
    corpus[80][4] = [20, 21, 22, 23, 24, 25]; edges["clip_caption"] = [0, 80, 4]       # holds word 20 once
    corpus[80][5] = [30, 31, 32, 33, 34]; edges["distinct_words_caption"] = [0, 80, 5]
    corpus[81][1] = zipf_ids(rng, 57, pool)
    corpus[82][2] = zipf_ids(rng, 64, pool)
    corpus[83][3] = zipf_ids(rng, 200, pool)
    edges["long_captions"] = [[81, 1, 57], [82, 2, 64], [83, 3, 200]]

    sizes = [10, 7, 1, 12, 5, 8]
    nn = np.zeros((len(sizes), K + 4), np.int64)                                       # lists longer than k: only the first k count
    nn[0] = rng.choice(np.arange(84, 130), K + 4, replace=False)
    nn[0, :4] = [80, 81, 82, 83]
    nn[1] = rng.choice(np.arange(130, N_IMG), K + 4, replace=False)
    nn[2] = rng.choice(np.arange(0, 40), K + 4, replace=False)
    nn[3] = rng.choice(np.arange(130, N_IMG), K + 4, replace=False)
    nn[4] = rng.choice(np.arange(40, 80), K + 4, replace=False)
    nn[5] = rng.choice(np.arange(84, N_IMG), K + 4, replace=False)
    edges["neighbour_list_entries"] = K + 4
    model_words = np.arange(1, CORPUS_LO_HI + 1)
    cands = []
    for i, n in enumerate(sizes):
        rows = []
        neigh = [c for j in nn[i, :K] for c in corpus[j] if len([w for w in c if w <= V]) >= 6]
        for c in range(n):
            src = [w for w in neigh[int(rng.integers(len(neigh)))] if w <= V]
            a = int(rng.integers(0, len(src) - 4))
            s = src[a:a + int(rng.integers(5, 12))] + zipf_ids(rng, int(rng.integers(0, 6)), model_words)
            rows.append(s[:T])
        cands.append(rows)

    def from_neighbour(i, n_words):
        src = next(c for j in nn[i, :K] for c in corpus[j] if len(c) >= 6 and all(w <= V for w in c[:n_words]))
        return list(src[:n_words])

    cands[0][0] = []; edges["empty_candidate"] = [0, 0]
    cands[0][1] = [20, 20, 21, 22, 23, 20]; edges["repeated_word_candidate"] = [0, 1]  # word 20 three times against clip_caption's one
    cands[0][5] = list(cands[0][2]); edges["duplicate_candidates"] = [0, 2, 5]
    cands[0][3] = [34, 33, 32, 31, 30]; edges["unigrams_only_candidate"] = [0, 3]      # distinct_words_caption reversed: no common bigram
    cands[0][4] = [30, 31, 32, 33, 34]; edges["identical_candidate"] = [0, 4]          # distinct_words_caption itself: pair score 1.0
    cands[0][6] = from_neighbour(0, 4); edges["four_word_candidate"] = [0, 6]          # exactly n words in set A
    cands[1][0] = from_neighbour(1, 3); edges["three_word_candidate"] = [1, 0]         # n - 1 words in set A: scores 0 everywhere there
    cands[3][0] = [7]; edges["one_word_candidate"] = [3, 0]                            # n - 1 words in set B
    cands[3][7] = list(cands[3][1]); cands[3][9] = list(cands[3][1]); edges["triplicate_candidates"] = [3, 1, 7, 9]
    cands[4][0] = from_neighbour(4, 2); edges["two_word_candidate"] = [4, 0]           # exactly n words in set B
    cands[5][0] = [150, 151, 152, 153, 154]; edges["no_common_word_candidate"] = [5, 0]
    edges["more_captions_than_m_image"] = {"A": 0, "B": 0}
    edges["fewer_captions_than_m_image"] = {"A": 2, "B": 4}

    rows = sum(sizes)
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rets = []
    for i in range(len(sizes)):
        ret = []
        for j in range(K):
            ret += corpus[int(nn[i, j])]
        rets.append(ret)
    max_caps = max(len(r) for r in rets)
    words = lambda ids: [f"w{x}" for x in ids]
    out, record = {}, {}
    for name, p in SETS.items():
        pairs = np.full((rows, max_caps), -1.0)
        sums, orders = [], []
        min_gap, worst_pair, worst_sum = np.inf, 0.0, 0.0
        for i, n in enumerate(sizes):
            sim = []
            for a, c in enumerate(cands[i]):
                b = [calculate_bleu_sentence(words(c), words(r), p["n"], fpr=p["fpr"]) for r in rets[i]]
                pairs[bounds[i] + a, :len(b)] = b
                b.sort(reverse=True)
                sim.append(sum(b[:p["m"]]))
            order = np.argsort(-np.array(sim))
            stable = np.argsort(-np.array(sim), kind="stable")                  # np.argsort's default kind leaves equal sums in any order:
            for x, y in zip(order, stable):                                     # it may differ from the stable order among identical rows only
                assert x == y or cands[i][x] == cands[i][y], (name, i)
            srt = np.array(sim)[order]
            for x in range(len(srt) - 1):
                if srt[x] == srt[x + 1]:
                    assert cands[i][order[x]] == cands[i][order[x + 1]], (name, i, "an exact tie between different candidates: change SEED")
                else:
                    gap = (srt[x] - srt[x + 1]) / srt[x]
                    assert gap > GAP, (name, i, gap, "change SEED")
                    min_gap = min(min_gap, gap)
            sums += sim
            orders += order.tolist()
            rp, rs, ro = bleu_rerank_restatement(cands[i], corpus, nn[i], K, p["m"], p["n"], p["fpr"])
            ref_p = pairs[bounds[i]:bounds[i + 1], :len(rets[i])]
            assert ((rp == 0) == (ref_p == 0)).all() and ro.tolist() == stable.tolist()
            nz = ref_p != 0
            worst_pair = max(worst_pair, float(np.max(np.abs(rp - ref_p)[nz] / ref_p[nz], initial=0.0)))
            nzs = np.array(sim) != 0
            worst_sum = max(worst_sum, float(np.max(np.abs(rs - np.array(sim))[nzs] / np.array(sim)[nzs], initial=0.0)))
        ncaps = [len(r) for r in rets]
        assert ncaps[edges["more_captions_than_m_image"][name]] > p["m"] > ncaps[edges["fewer_captions_than_m_image"][name]]
        out["pairs_" + name], out["sums_" + name], out["orders_" + name] = pairs, np.asarray(sums, np.float64), np.asarray(orders, np.int64)
        record[name] = dict(p, min_nonzero_gap=min_gap, restatement_worst_rel_pair_in_u=worst_pair * 2.0 ** 53,
                            restatement_worst_rel_sum_in_u=worst_sum * 2.0 ** 53)
    seq = np.zeros((rows, T), np.int64)
    r = 0
    for rows_i in cands:
        for c in rows_i:
            assert len(c) <= T and all(1 <= w <= V for w in c)
            seq[r, :len(c)] = c
            r += 1
    flat = [w for caps in corpus for c in caps for w in c]
    lens = [len(c) for caps in corpus for c in caps]
    assert max(flat) > V
    np.savez_compressed(os.path.join(HERE, "consensus_bleu_case.npz"),
                        corpus_words=np.asarray(flat, np.int32), corpus_woff=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                        corpus_cap_off=np.concatenate([[0], np.cumsum([len(c) for c in corpus])]).astype(np.int64),
                        cand=seq, bounds=bounds, nn=nn, n_caps=np.asarray([len(r) for r in rets], np.int64), **out)
    with open(os.path.join(HERE, "consensus_bleu_meta.json"), "w") as f:
        json.dump({"V": V, "k": K, "T": T, "n_img": N_IMG, "seed": SEED, "sets": record, "edges": edges, "gap_rule": GAP,
                   "order_rule": "orders_* hold the reference's np.argsort(-sim); it differs from the stable order among identical candidate rows only",
                   "nltk": "stand-in: nltk.util.ngrams(sequence, n) = the sliding window of n-tuples (nltk is not installed where the fixture is made)",
                   "numpy": np.__version__, "python": sys.version.split()[0]}, f, indent=1)
    print("wrote consensus_bleu_case.npz / consensus_bleu_meta.json:", rows, "candidates,", max_caps, "neighbour captions at most;", record)


if __name__ == "__main__":
    main()
