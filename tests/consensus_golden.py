"""Helpers of the consensus re-ranking tests: the fixture written by tests/golden/make_golden_consensus.py (the reference's own
CiderScorer run on a synthetic corpus) and a plain-numpy restatement of the scorer and of the re-ranking loop for sizes the fixture
does not cover.  Sentences are lists of word ids here; the restatement keys its dictionaries by id tuples, which is what the reference
does with word tuples once every distinct word has its own id."""
import json
import os
from collections import defaultdict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    """-> (meta dict, arrays dict) of the committed fixture."""
    with open(os.path.join(GOLDEN, "consensus_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "consensus_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def word(i):
    return f"w{int(i)}"


def corpus_sentences(arr):
    """The fixture's corpus as `ref_sentences` (per image a list of captions, each a list of words) and as id lists."""
    words, woff, cap_off = arr["corpus_words"], arr["corpus_woff"], arr["corpus_cap_off"]
    ids = [[[int(x) for x in words[woff[c]:woff[c + 1]]] for c in range(cap_off[i], cap_off[i + 1])] for i in range(len(cap_off) - 1)]
    return [[[word(x) for x in cap] for cap in caps] for caps in ids], ids


def rows_to_ids(rows):
    out = []
    for r in np.asarray(rows):
        s = []
        for x in r:
            if x <= 0:
                break
            s.append(int(x))
        out.append(s)
    return out


def ngram_counts(sent, n=4):
    c = defaultdict(int)
    for k in range(1, n + 1):
        for i in range(len(sent) - k + 1):
            c[tuple(sent[i:i + k])] += 1
    return c


class Scorer:
    """CIDEr between two sentences with the document frequencies of a corpus: tf-idf vectors per n-gram order, clipped cosine,
    Gaussian penalty on the difference of the BIGRAM counts, 10 x the mean of the four orders."""

    def __init__(self, ref_ids, n=4, sigma=6.0):
        self.n, self.sigma = n, sigma
        self.df = defaultdict(float)
        for caps in ref_ids:
            seen = set()
            for cap in caps:
                seen.update(ngram_counts(cap, n).keys())
            for g in seen:
                self.df[g] += 1
        self.ref_len = np.log(float(len(ref_ids)))
        self._cache = {}

    def vec(self, sent):
        key = tuple(sent)
        hit = self._cache.get(key)
        if hit is not None:
            return hit
        vec = [dict() for _ in range(self.n)]
        norm = [0.0] * self.n
        length = 0
        for g, tf in ngram_counts(sent, self.n).items():
            o = len(g) - 1
            w = float(tf) * (self.ref_len - np.log(max(1.0, self.df.get(g, 0.0))))
            vec[o][g] = w
            norm[o] += pow(w, 2)
            if o == 1:
                length += tf
        out = self._cache[key] = (vec, [np.sqrt(x) for x in norm], length)
        return out

    def pair(self, hyp, ref):
        vh, nh, lh = self.vec(hyp)
        vr, nr, lr = self.vec(ref)
        delta = float(lh - lr)
        val = np.zeros(self.n)
        for o in range(self.n):
            for g, w in vh[o].items():
                r = vr[o].get(g, 0.0)
                val[o] += min(w, r) * r
            if nh[o] != 0 and nr[o] != 0:
                val[o] /= nh[o] * nr[o]
            val[o] *= np.e ** (-(delta ** 2) / (2 * self.sigma ** 2))
        return float(np.mean(val) * 10.0)


def rerank(scorer, cands, ref_ids, nn, k, m):
    """One image: candidates (id lists) against the captions of its first k neighbours -> (pair scores [cands, captions], sums,
    stable descending order of the sums: lower candidate index first among equals)."""
    caps = []
    for j in range(k):
        caps += ref_ids[int(nn[j])]
    pairs = np.zeros((len(cands), len(caps)))
    sums = np.zeros(len(cands))
    for a, c in enumerate(cands):
        for b, r in enumerate(caps):
            pairs[a, b] = scorer.pair(c, r)
        s = sorted(pairs[a].tolist(), reverse=True)
        sums[a] = sum(s[:m])
    return pairs, sums, np.argsort(-sums, kind="stable")


def close(got, want, rel):
    """|got - want| <= rel * |want| + 1e-300, elementwise."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want) + 1e-300))
