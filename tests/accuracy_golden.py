"""The accuracy fixture (tests/golden/make_golden_accuracy.py: written by the reference's own scorers) and a plain restatement of the
three scorers and the oracle, written from scratch with Counters and Python floats, for sizes the fixture does not cover."""
import json
import math
import os
from collections import Counter

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLEU_TOL, CIDER_TOL, ROUGE_TOL = 1e-12, 1e-11, 1e-14      # relative; derived in DESIGN 4.I


def load():
    with open(os.path.join(GOLDEN, "accuracy_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "accuracy_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def vocab(V):
    return {str(i): f"w{i}" for i in range(1, V + 1)}


def fixture_refs(arr):
    """-> per image the reference captions as lists of the words "w<id>"."""
    w, off, cap = arr["ref_words"], arr["ref_woff"], arr["ref_cap_off"]
    return [[[f"w{int(x)}" for x in w[off[s]:off[s + 1]]] for s in range(cap[j], cap[j + 1])] for j in range(len(cap) - 1)]


def rows_to_ids(seq):
    out = []
    for row in np.asarray(seq):
        ids = []
        for x in row:
            if x <= 0:
                break
            ids.append(int(x))
        out.append(ids)
    return out


def rel(got, want):
    """The largest relative difference; a reference 0.0 must be met exactly (-> inf otherwise)."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    worst = 0.0
    for g, w in zip(got, want):
        if w == 0.0:
            worst = max(worst, 0.0 if g == 0.0 else math.inf)
        else:
            worst = max(worst, abs(g - w) / abs(w))
    return worst


def ngrams(ids):
    c = Counter()
    for k in range(1, 5):
        for i in range(len(ids) - k + 1):
            c[tuple(ids[i:i + k])] += 1
    return c


def log_df(ref_ids):
    """-> ({n-gram: log(number of images one of whose references holds it)}, log(number of images))."""
    df = Counter()
    for caps in ref_ids:
        for g in set(g for cap in caps for g in ngrams(cap)):
            df[g] += 1
    return {g: float(np.log(max(1.0, float(v)))) for g, v in df.items()}, float(np.log(float(len(ref_ids))))


def lcs(a, b):
    """The quadratic table of the longest common subsequence, one row at a time (a row is non-decreasing, so the running maximum of
    "diagonal + 1 where the words match, the cell above elsewhere" is the row)."""
    b = np.asarray(b, np.int64)
    prev = np.zeros(len(b) + 1, np.int64)
    for x in a:
        cur = np.zeros(len(b) + 1, np.int64)
        cur[1:] = np.maximum.accumulate(np.where(b == x, prev[:-1] + 1, prev[1:]))
        prev = cur
    return int(prev[-1])


def tfidf(c, ldf, ref_len):
    v = {g: float(n) * (ref_len - ldf.get(g, 0.0)) for g, n in c.items()}
    norm = [math.sqrt(sum(x * x for g, x in sorted(v.items()) if len(g) == k + 1)) for k in range(4)]
    return v, norm, sum(n for g, n in c.items() if len(g) == 2)


def prepare(refs, ldf, ref_len):
    """What a candidate needs of its image's references (id lists): lengths, n-gram counts, tf-idf vectors."""
    rc = [ngrams(r) for r in refs]
    return {"refs": refs, "counts": rc, "vecs": [tfidf(c, ldf, ref_len) for c in rc]}


def restate_row(cand, prep, ldf, ref_len, sigma=6.0):
    """One candidate (id list) against its image's prepared references -> (material [10], values [6])."""
    refs, rc = prep["refs"], prep["counts"]
    cc = ngrams(cand)
    testlen = len(cand)
    reflen = min((abs(len(r) - testlen), len(r)) for r in refs)[1]
    guess = [max(0, testlen - k) for k in range(4)]
    correct = [0] * 4
    for g, n in cc.items():
        correct[len(g) - 1] += min(n, max(c.get(g, 0) for c in rc))
    vals, prod = [], 1.0
    for k in range(4):
        prod *= (float(correct[k]) + 1e-15) / (float(guess[k]) + 1e-9)
        vals.append(prod ** (1.0 / (k + 1)))
    ratio = (testlen + 1e-15) / (reflen + 1e-9)
    if ratio < 1:
        vals = [v * math.exp(1 - 1 / ratio) for v in vals]
    hv, hn, hl = tfidf(cc, ldf, ref_len)
    score = [0.0] * 4
    for rv, rn, rl in prep["vecs"]:
        val = [0.0] * 4
        for g, x in sorted(hv.items()):
            if g in rv:
                val[len(g) - 1] += min(x, rv[g]) * rv[g]
        for k in range(4):
            if hn[k] != 0 and rn[k] != 0:
                val[k] /= hn[k] * rn[k]
            val[k] *= math.e ** (-(float(hl - rl) ** 2) / (2 * sigma ** 2))
            score[k] += val[k]
    cider = (((score[0] + score[1]) + score[2]) + score[3]) / 4.0 / len(refs) * 10.0
    a = cand if cand else [0]                                              # split(" "): the empty caption is the one-word caption of the empty word
    prec, rec = [], []
    for r in refs:
        b = r if r else [0]
        n = lcs(a, b)
        prec.append(n / float(len(a)))
        rec.append(n / float(len(b)))
    p, r = max(prec), max(rec)
    rouge = ((1 + 1.2 ** 2) * p * r) / float(r + 1.2 ** 2 * p) if p != 0 and r != 0 else 0.0
    return [testlen, reflen] + guess + correct, vals + [cider, rouge]


def trim(ids, bad_ids):
    n = len(ids)
    while n and ids[n - 1] in bad_ids:
        n -= 1
    return ids if n == 0 else ids[:n]


def restate_rows(cands, bounds, image_index, ref_ids):
    """Every row's (material, values): the part that does not depend on oracle_num."""
    ldf, ref_len = log_df(ref_ids)
    prep = {}
    out = []
    for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
        j = image_index[i]
        if j not in prep:
            prep[j] = prepare(ref_ids[j], ldf, ref_len)
        out += [restate_row(c, prep[j], ldf, ref_len) for c in cands[a:b]]
    return out


def restate(cands, bounds, image_index, ref_ids, oracle_num, first=None, rows=None):
    """-> per image {"material", "values", "oracle_rows", "oracle_material", "oracle_values", "top1_row", ...} like AccuracyScorer.unpack."""
    rows = restate_rows(cands, bounds, image_index, ref_ids) if rows is None else rows
    out = []
    for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
        mat = np.array([m for m, _ in rows[a:b]], np.int64).reshape(-1, 10)
        val = np.array([v for _, v in rows[a:b]], np.float64).reshape(-1, 6)
        m = min(b - a, oracle_num)
        picks = [int(np.argmax(val[:m, k])) for k in range(4)]
        f = 0 if first is None else int(first[i])
        out.append({"n": b - a, "considered": m, "material": mat, "values": val, "oracle_rows": np.array(picks), "oracle_material": mat[picks],
                    "oracle_values": val[:m].max(0), "top1_row": f, "top1_material": mat[f], "top1_values": val[f]})
    return out


def fixture_per_image(meta, arr, q):
    """The fixture's recorded per-row and per-image data as `unpack`-style entries for oracle_nums[q]."""
    b, N = arr["bounds"], meta["oracle_nums"][q]
    out = []
    for i in range(len(b) - 1):
        mat, val = arr["row_i"][b[i]:b[i + 1]].astype(np.int64), arr["row_d"][b[i]:b[i + 1]]
        out.append({"n": int(b[i + 1] - b[i]), "considered": min(int(b[i + 1] - b[i]), N), "material": mat, "values": val,
                    "oracle_rows": arr["picks"][q, i].astype(np.int64), "oracle_material": arr["pick_mat"][q, i].astype(np.int64),
                    "oracle_values": arr["best"][q, i], "top1_row": 0, "top1_material": mat[0], "top1_values": val[0]})
    return out


def compare(got, want, exact_values=False):
    """Per-image entries against expected ones: integers and picks ==, values within the bounds -> the largest relative differences
    (BLEU, CIDEr, ROUGE-L)."""
    worst = [0.0, 0.0, 0.0]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["n"] == w["n"] and g["considered"] == w["considered"] and g["top1_row"] == w["top1_row"], i
        np.testing.assert_array_equal(g["material"], w["material"], err_msg=f"image {i}")
        np.testing.assert_array_equal(g["oracle_rows"], w["oracle_rows"], err_msg=f"image {i}")
        np.testing.assert_array_equal(g["oracle_material"], w["oracle_material"], err_msg=f"image {i}")
        np.testing.assert_array_equal(g["top1_material"], w["top1_material"], err_msg=f"image {i}")
        for key, cols in (("values", None), ("top1_values", None), ("oracle_values", None)):
            gv, wv = np.asarray(g[key]).reshape(-1, 6), np.asarray(w[key]).reshape(-1, 6)
            worst[0] = max(worst[0], rel(gv[:, :4], wv[:, :4]))
            worst[1] = max(worst[1], rel(gv[:, 4], wv[:, 4]))
            worst[2] = max(worst[2], rel(gv[:, 5], wv[:, 5]))
    return worst
