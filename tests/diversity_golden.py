"""Helpers of the diversity tests: the fixture written by tests/golden/make_golden_diversity.py (the reference's own
diversity_score.py run on synthetic captions) and a plain set-and-dict restatement of one set -- a draw of one image -- for sizes the
fixture does not cover.  Captions are lists of word ids here; the restatement keys its sets and dictionaries by id tuples, which is what
the reference does with strings once every distinct word has its own id."""
import json
import math
import os
from collections import Counter

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD_ENDINGS = ("with", "in", "on", "of", "a", "at", "to", "for", "an", "this", "his", "her", "that", "the")


def load():
    """-> (meta dict, arrays dict) of the committed fixture."""
    with open(os.path.join(GOLDEN, "diversity_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "diversity_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def word(i):
    return f"w{int(i)}"


def vocab(V):
    return {str(i): word(i) for i in range(1, V + 1)}


def fixture_draws(meta, arr, run):
    """{metric: [per image [per top_n: indices]]} as recorded for `run` ('mb4' / 'plain')."""
    nt, n_img = len(meta["top_n"]), len(meta["sub_nums"])
    out = {}
    for metric in (4, 3, 2, 1):
        key = f"draws_{run}_{metric}"
        if key not in arr:
            continue
        flat, off = arr[key], arr[f"draws_off_{run}_{metric}"]
        out[metric] = [[flat[off[i * nt + t]:off[i * nt + t + 1]].astype(np.int64) for t in range(nt)] for i in range(n_img)]
    return out


def fixture_per_image(meta, arr, run):
    """The fixture's per-image expectations in the shape DiversityScorer.unpack returns."""
    exp = arr[f"exp_{run}"]
    out = []
    for i in range(exp.shape[0]):
        e = {"drawn": exp[i, :, 0], "distinct": exp[i, :, 1], "words": exp[i, :, 2], "unigrams": exp[i, :, 3], "bigrams": exp[i, :, 4],
             "novel": exp[i, :, 5], "novel_of": exp[i, :, 6]}
        if run == "mb4":
            b = arr["bleu4"][i]
            e["bleu4"] = b
            e["mbleu4"] = np.array([np.mean(np.array([x for x in row if not np.isnan(x)])) for row in b])
            e["mbleu4_valid"] = np.array([int((~np.isnan(row)).sum()) >= 2 for row in b])
        out.append(e)
    return out


def rows_to_ids(rows, bad=None):
    """Token rows -> id lists: the ids before the first id <= 0; `bad` (a set of ids): without the trailing ids in it, unless all are."""
    out = []
    for r in np.asarray(rows):
        s = []
        for x in r:
            if x <= 0:
                break
            s.append(int(x))
        if bad:
            keep = len(s)
            while keep > 0 and s[keep - 1] in bad:
                keep -= 1
            if keep > 0:
                s = s[:keep]
        out.append(s)
    return out


def _ngrams(s):
    return Counter(tuple(s[i:i + k]) for k in range(1, 5) for i in range(len(s) - k + 1))


def sentence_bleu4(test, refs):
    most = {}
    for r in refs:
        for g, c in _ngrams(r).items():
            most[g] = max(most.get(g, 0), c)
    correct = [0] * 4
    for g, c in _ngrams(test).items():
        correct[len(g) - 1] += min(most.get(g, 0), c)
    reflen = min((abs(len(r) - len(test)), len(r)) for r in refs)[1]
    bleu = 1.0
    for k in range(4):
        bleu *= (float(correct[k]) + 1e-15) / (float(max(0, len(test) - k)) + 1e-9)
    b4 = bleu ** (1.0 / 4)
    ratio = (len(test) + 1e-15) / (reflen + 1e-9)
    if ratio < 1:
        b4 *= math.exp(1 - 1 / ratio)
    return b4


def restate(caps, score, draw, n_best, train=None):
    """One set: `caps` the image's captions (id lists), `score` its float32 scores, `draw` the drawn indices -> the dict of everything the
    device returns for it.  Selection: a stable ascending sort of the drawn scores, reversed (equal scores: later in the draw first)."""
    draw = np.asarray(draw, np.int64)
    drawn = [tuple(caps[j]) for j in draw]
    best = draw[np.argsort(np.asarray(score, np.float32)[draw], kind="stable")[::-1][:n_best]] if len(draw) else draw
    sel = [list(caps[j]) for j in best]
    sp = [s if s else [0] for s in sel]                          # split(' '): an empty caption is one word, the empty word
    words = [w for s in sp for w in s]
    pairs = [(s[j], s[j + 1]) for s in sp for j in range(len(s) - 1)]
    out = {"drawn": len(drawn), "distinct": len(set(drawn)), "selected": [int(x) for x in best], "words": len(words), "unigrams": len(set(words)),
           "bigrams": len(set(pairs)), "novel": None if train is None else sum(1 for s in sel if tuple(s) not in train)}
    if len(sel) >= 2:
        out["bleu4"] = [sentence_bleu4(s, [r for j, r in enumerate(sel) if j != q]) for q, s in enumerate(sel)]
        out["mbleu4"] = float(np.mean(np.array(out["bleu4"])))
    return out


def close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want)))


def worst_rel(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0
