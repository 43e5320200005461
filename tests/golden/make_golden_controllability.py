#!/usr/bin/env python
"""Write the controllability fixture by RUNNING THE REFERENCE's own code where the reference lies (never copied):
controllability_case.npz + controllability_meta.json.  Data only: fabricated word vectors, ground-truth groups and generated captions as
id arrays, and what the reference computed for them.

    python tests/golden/make_golden_controllability.py

What runs: misc/controllability/noun_iou.py `NounIoU.score`, UNMODIFIED, on a temporary pickle of the vectors, once per (generated
caption, ground-truth caption) pair, then the group loop of controllability_score.py:47-52,74 (`score_iou += score`,
`score_iou / len(group)`, `np.mean`), restated here line by line because the script itself is one `__main__` block that needs `speaksee`.
`munkres` is NOT installed where this fixture is made, so a STAND-IN module is written to a temporary directory (the way
make_golden_grounding.py stands in for `stanfordcorenlp`): `make_cost_matrix(profit)` = `max - profit` and `Munkres().compute(cost)` = the
(row, column) list of `scipy.optimize.linear_sum_assignment`.  Only the VALUE of the assignment enters the score, so which optimal
assignment a solver returns under ties is nothing to reproduce.  `speaksee`'s Bleu / Rouge / Cider are the COCO classes; the reference's
own misc/coco-caption/pycocoevalcap copies run in their place, exactly as in make_golden_accuracy.py (PTB tokenisation is out of scope:
captions are split at white space).

Word i is the string VOCAB[i] for the model's ids 1 .. V ("w<i>", a few of them bad endings) and "w<i>" above V (reference-only words).
Generated captions are token rows turned into strings by `subgc.eval_glue.decode_sequence`, which tests/test_eval_glue.py pins against
strings of the reference's own decode_sequence.

Sets: `rnd` (random normal vectors, d = 300), `exact` (integer vector components in [-8, 8], d = 50: every dot product is exact in any
order), `edge` / `edge_rbe` (the planted cases, without / with bad endings removed; see `edges` in the meta), `edge_d1` (d = 1) and
`sct_subgc` (the kept rows of tests/golden/subgc_sct_out.npz, read, not rewritten, against fabricated groups and vectors).

The meta records, per set, the worst difference between the reference's pair scores and an fp64 evaluation of the same definition (brute
force over all assignments where min(m, n) <= 7 and there are at most 200000 of them, scipy on the fp64 matrix otherwise), the versions of numpy / torch / scipy, and that
the assignment solver is a stand-in."""
import contextlib
import io
import itertools
import json
import math
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

STUB = '''import numpy as np
from scipy.optimize import linear_sum_assignment
def make_cost_matrix(profit):
    profit = np.asarray(profit)
    return profit.max() - profit
class Munkres:
    def compute(self, cost):
        r, c = linear_sum_assignment(np.asarray(cost))
        return [(int(a), int(b)) for a, b in zip(r, c)]
'''

V, SEED = 50, 20261019
# |device - reference| (worst pair, worst row) as tests/test_controllability_gpu.py printed it on an MI355X, written into the meta beside the
# derived bounds of DESIGN 4.K (controllability_golden.pair_bound / row_bound); a record, not an input of any test
OBSERVED = {"rnd": (2.9802322387695312e-08, 2.9802322387695312e-08), "exact": (1.7881393432617188e-07, 5.960464477539063e-08),
            "edge": (5.960464477539063e-08, 5.960464477539063e-08), "edge_rbe": (5.960464477539063e-08, 5.960464477539063e-08),
            "edge_d1": (0.0, 0.0), "sct_subgc": (0.0, 0.0)}
U = 2.0 ** -24


def pair_bound(d, m, n):
    k = min(m, n)
    return 0.0 if k == 0 else (2 * (d + 6) + 4 * (k - 1) + 6) * U
BAD = {7: "the", 9: "of", 13: "with"}
VOCAB = {str(i): BAD.get(i, f"w{i}") for i in range(1, V + 1)}


def word(i):
    return VOCAB[str(i)] if i <= V else f"w{i}"


def sentence(ids):
    return " ".join(word(int(i)) for i in ids)


def fp64_pair(gt, pred, vecs):
    """The definition in fp64: -> (iou, k = min(m, n), how the optimum was found)."""
    a = [vecs[w] for w in gt if w in vecs]
    b = [vecs[w] for w in pred if w in vecs]
    m, n = len(a), len(b)
    if m == 0:
        return 1.0, 0, "trivial"
    if n == 0:
        return 0.0, 0, "trivial"
    A, B = np.array(a, np.float64), np.array(b, np.float64)
    den = np.maximum(np.sqrt((A * A).sum(1))[:, None] * np.sqrt((B * B).sum(1))[None, :], 1e-8)
    S = ((A @ B.T) / den + 1.0) / 2.0
    if m > n:
        S = S.T
    k, c = S.shape
    if k <= 7 and math.perm(c, k) <= 200000:
        perms = np.array(list(itertools.permutations(range(c), k)), np.int64)
        best = float(S[np.arange(k)[None, :], perms].sum(1).max())
        how = "brute force"
    else:
        from scipy.optimize import linear_sum_assignment
        rr, cc = linear_sum_assignment(-S)
        best = float(S[rr, cc].sum())
        how = "scipy on the fp64 matrix"
    return best / (m + n - best), k, how


def random_set(rng, n_rows, d, integer, T=20):
    """Groups of 1-6 captions, m and n in 0 .. 8; vector words among the model's ids and above them."""
    nouns = [int(x) for x in rng.permutation(np.arange(1, V + 1))[:18]] + list(range(V + 1, V + 9))
    if 7 not in nouns:
        nouns[0] = 7                                                         # a bad ending that has a vector
    fill_model = [i for i in range(1, V + 1) if i not in nouns]
    fill_ref = list(range(V + 9, V + 15))
    vec = rng.integers(-8, 9, size=(len(nouns), d)).astype(np.float32) if integer else rng.standard_normal((len(nouns), d)).astype(np.float32)
    model_nouns = [i for i in nouns if i <= V]
    seq = np.zeros((n_rows, T), np.int16)
    groups = []
    for r in range(n_rows):
        caps = []
        for _ in range(int(rng.integers(1, 7))):
            m = int(rng.integers(0, 9))
            ws = [int(x) for x in rng.choice(nouns, size=m)] + [int(x) for x in rng.choice(fill_model + fill_ref, size=int(rng.integers(1, 6)))]
            caps.append([ws[i] for i in rng.permutation(len(ws))])
        groups.append(caps)
        n = int(rng.integers(0, 9))
        near = [w for c in caps for w in c if w in model_nouns]
        ws = [int(rng.choice(near)) if near and rng.random() < 0.5 else int(rng.choice(model_nouns)) for _ in range(n)]
        ws += [int(x) for x in rng.choice(fill_model, size=int(rng.integers(0, T - n - 1)))]
        ws = [ws[i] for i in rng.permutation(len(ws))]
        seq[r, :len(ws)] = ws
    return {"seq": seq, "row_group": np.arange(n_rows, dtype=np.int32), "groups": groups, "nouns": nouns, "vec": vec, "rbe": 0}


def edge_set(rng, rbe):
    """The planted cases; integer vectors, d = 50, T = 64.  Vector words: 1 .. 6 and 7 ("the") of the model, 51 .. 54 above it;
    20 = a word whose vector is -vec(1), 21 = a second word with vec(1), 22 = the zero vector."""
    d, T = 50, 64
    nouns = [1, 2, 3, 4, 5, 6, 7, 51, 52, 53, 54, 20, 21, 22]
    vec = rng.integers(-8, 9, size=(len(nouns), d)).astype(np.float32)
    vec[nouns.index(20)] = -vec[nouns.index(1)]
    vec[nouns.index(21)] = vec[nouns.index(1)]
    vec[nouns.index(22)] = 0
    cyc = lambda k, pool: [pool[i % len(pool)] for i in range(k)]
    rows, edges = [], {}

    def add(name, pred, caps, group=True):
        edges[name] = len(rows)
        rows.append((pred, caps, group))
    add("m_is_0", [1, 2, 30], [[30, 31, 60]])
    add("n_is_0", [30, 31], [[1, 2, 30]])
    add("both_0", [30], [[31, 60]])
    add("empty_prediction", [], [[1, 2], [30]])
    add("m_64_n_64", cyc(64, [1, 2, 3, 4, 5, 6, 20, 21]), [cyc(64, [51, 52, 53, 54, 1, 2, 3, 22, 20])])
    add("m_64_n_1", [30, 3, 31], [cyc(64, [51, 52, 53, 54, 1, 2, 3, 4, 5])])
    add("m_1_n_64", cyc(64, [1, 2, 3, 4, 5, 6, 20]), [[30, 52, 31]])
    add("all_ties", [4, 4, 4], [[4, 4, 4, 4], [4, 4]])
    add("repeated_on_both_sides", [1, 2, 1, 3, 1], [[1, 5, 1, 51], [2, 2, 1]])
    add("antiparallel", [20, 30], [[1, 31]])
    add("identical_vectors", [21, 2], [[1, 30, 2]])
    add("zero_vector", [22, 1], [[2, 3], [22], [22, 22, 1]])
    add("bad_endings_with_a_vector", [1, 2, 30, 7, 9, 7], [[1, 2, 7], [7, 51]])
    add("only_bad_endings", [7, 9, 7], [[7, 1]])
    add("trivial_and_real_pairs", [1, 2, 3], [[30], [1, 2, 3], [31, 60], [3, 2, 1, 51]])
    add("no_group", [1, 2, 3], None, group=False)
    add("six_captions", [5, 6, 1], [[5], [6, 6], [1, 5, 6], [51, 52], [30], [53, 54, 5, 6, 1, 2]])
    seq = np.zeros((len(rows), T), np.int16)
    groups, row_group = [], []
    for r, (pred, caps, has) in enumerate(rows):
        seq[r, :len(pred)] = pred
        row_group.append(len(groups) if has else -1)
        if has:
            groups.append(caps)
    return {"seq": seq, "row_group": np.array(row_group, np.int32), "groups": groups, "nouns": nouns, "vec": vec, "rbe": rbe}, edges


def d1_set():
    nouns = [1, 2, 3, 4, 51]
    vec = np.array([[2.0], [-3.0], [0.0], [5.0], [-1.0]], np.float32)
    preds = [[1, 2, 30], [3, 4], [2, 2, 2, 1], [4]]
    groups = [[[1, 51], [2]], [[3, 1, 2]], [[4, 4, 51, 51, 2], [30]], [[51]]]
    seq = np.zeros((4, 8), np.int16)
    for r, p in enumerate(preds):
        seq[r, :len(p)] = p
    return {"seq": seq, "row_group": np.arange(4, dtype=np.int32), "groups": groups, "nouns": nouns, "vec": vec, "rbe": 0}


def sct_set(rng):
    with np.load(os.path.join(HERE, "subgc_sct_out.npz")) as z:
        full = z["seq"]
    seq = full[:full.shape[0] // 2].astype(np.int16)                         # rank_subgraphs(sct_mode=True): the first half, input order
    used = sorted({int(x) for x in seq.ravel() if x > 0})
    nouns = used[::2] + [V + 1, V + 2]
    vec = rng.standard_normal((len(nouns), 300)).astype(np.float32)
    groups = []
    for r in range(len(seq)):
        mine = [int(x) for x in seq[r] if x > 0]
        caps = []
        for _ in range(int(rng.integers(1, 5))):
            c = [w for w in mine if rng.random() < 0.7] + [int(x) for x in rng.choice(nouns, size=int(rng.integers(0, 4)))]
            caps.append([c[i] for i in rng.permutation(len(c))] or [int(nouns[0])])
        groups.append(caps)
    return {"seq": seq, "row_group": np.arange(len(seq), dtype=np.int32), "groups": groups, "nouns": nouns, "vec": vec, "rbe": 0}


def run_set(case, tmp, tag):
    """-> (arrays of the set, its meta)."""
    sys.path.insert(0, os.path.join(ROOT, "sub-gc_amd"))
    from subgc.eval_glue import decode_sequence
    from noun_iou import NounIoU
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.cider.cider import Cider
    from pycocoevalcap.rouge.rouge import Rouge
    vecs = {word(i): case["vec"][k].copy() for k, i in enumerate(case["nouns"])}
    pkl = os.path.join(tmp, f"{tag}.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(vecs, f)
    scorer = NounIoU(pre_comp_file=pkl)
    preds = decode_sequence(VOCAB, case["seq"].astype(np.int64).tolist(), case["rbe"])
    gt_captions = [[sentence(c) for c in caps] for caps in case["groups"]]
    live = [r for r, g in enumerate(case["row_group"]) if g >= 0]
    # controllability_score.py:40-52
    gen, gts, scores_iou, pair_ref, pair_mn, pair_64, worst, hows = {}, {}, [], [], [], [], 0.0, set()
    for i, r in enumerate(live):
        pred_cap = preds[r]
        gts[i] = gt_captions[case["row_group"][r]]
        gen[i] = [pred_cap]
        score_iou = 0.
        for c in gts[i]:
            score = scorer.score(c, pred_cap)
            score_iou += score
            pair_ref.append(score)
            pair_mn.append([len(scorer.prep_seq(c)), len(scorer.prep_seq(pred_cap))])
            x, k, how = fp64_pair(c.split(" "), pred_cap.split(" "), vecs)
            hows.add(how)
            pair_64.append(x)
            worst = max(worst, abs(float(score) - x))
        scores_iou.append(score_iou / len(gts[i]))
    corpus = np.mean(scores_iou)                                             # :74
    all_f32 = all(isinstance(s, np.float32) for s in scores_iou)
    with contextlib.redirect_stdout(io.StringIO()):
        b, bs, mat = Bleu(4).compute_score(gts, gen)
        ro, rs = Rouge().compute_score(gts, gen)
        ci, cs = Cider().compute_score(gts, gen)
    row_i = np.array([[mat["testlen"][i], mat["reflen"][i]] + [mat["guess"][k][i] for k in range(4)] + [mat["correct"][k][i] for k in range(4)]
                      for i in range(len(live))], np.int32).reshape(len(live), 10)
    row_d = np.array([[bs[k][i] for k in range(4)] + [cs[i], rs[i]] for i in range(len(live))], np.float64).reshape(len(live), 6)
    flat = [c for caps in case["groups"] for c in caps]
    row_ref = np.full(len(case["row_group"]), np.nan)
    row_ref[live] = [float(s) for s in scores_iou]
    arrays = {"seq": case["seq"], "row_group": case["row_group"], "vec": case["vec"], "nouns": np.array(case["nouns"], np.int32),
              "gcap_off": np.concatenate([[0], np.cumsum([len(c) for c in case["groups"]])]).astype(np.int32),
              "gwoff": np.concatenate([[0], np.cumsum([len(c) for c in flat])]).astype(np.int32),
              "gwords": np.array([w for c in flat for w in c], np.int32),
              "pair_iou": np.array([float(s) for s in pair_ref], np.float64), "pair_mn": np.array(pair_mn, np.int32).reshape(-1, 2),
              "pair_fp64": np.array(pair_64, np.float64), "row_iou": row_ref, "corpus_iou": np.array(float(corpus)),
              "corpus_iou_f32": np.array(np.mean(np.array([float(s) for s in scores_iou], np.float32))),
              "acc_row_i": row_i, "acc_row_d": row_d, "acc_corpus": np.array(list(b) + [ci, ro], np.float64)}
    meta = {"rows": int(len(case["row_group"])), "live_rows": len(live), "pairs": len(pair_ref), "d": int(case["vec"].shape[1]),
            "remove_bad_endings": case["rbe"], "every_row_score_is_float32": bool(all_f32), "noun_iou_return_types":
            sorted({type(s).__name__ for s in pair_ref}), "worst_difference_reference_vs_fp64": worst, "fp64_evaluation": sorted(hows),
            "max_m": int(max([p[0] for p in pair_mn] + [0])), "max_n": int(max([p[1] for p in pair_mn] + [0])),
            "device_vs_reference": {"derived_pair_bound_max": max([pair_bound(int(case["vec"].shape[1]), m, n) for m, n in pair_mn] + [0.0]),
                                    "observed_worst_pair": OBSERVED[tag][0], "observed_worst_row": OBSERVED[tag][1]},
            "corpus": {"Noun_IoU": float(corpus), "Bleu": [float(x) for x in b], "ROUGE_L": float(ro), "CIDEr": float(ci)}}
    return arrays, meta


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    import scipy
    import torch
    rng = np.random.default_rng(SEED)
    cases = {"rnd": random_set(rng, 40, 300, False), "exact": random_set(rng, 40, 50, True)}
    edge_rng = np.random.default_rng(SEED + 1)
    cases["edge"], edges = edge_set(edge_rng, 0)
    cases["edge_rbe"], _ = edge_set(np.random.default_rng(SEED + 1), 1)
    cases["edge_d1"] = d1_set()
    cases["sct_subgc"] = sct_set(rng)
    out, meta = {}, {"V": V, "bad_endings": {str(k): v for k, v in BAD.items()}, "seed": SEED, "edges": edges,
                     "edge_notes": {"int64_tokens": "the edge sets are run with int32 AND int64 token rows by the tests",
                                    "bad_endings": "edge (kept) and edge_rbe (removed) hold the same rows",
                                    "d_is_1": "the set edge_d1", "row_without_group": "row `no_group` of edge / edge_rbe: row_group = -1"},
                     "versions": {"numpy": np.__version__, "torch": torch.__version__, "scipy": scipy.__version__},
                     "assignment_solver": "STAND-IN for munkres (not installed here): make_cost_matrix = max - profit, Munkres().compute = "
                                          "scipy.optimize.linear_sum_assignment; noun_iou.py itself runs unmodified",
                     "coco_scorers": "the reference's misc/coco-caption/pycocoevalcap Bleu / Rouge / Cider stand where speaksee's (the same COCO "
                                     "classes) stand in controllability_score.py; no PTB tokenisation",
                     "excused_from_bit_exactness": [], "sets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "stub"))
        with open(os.path.join(tmp, "stub", "munkres.py"), "w") as f:
            f.write(STUB)
        sys.path[:0] = [os.path.join(tmp, "stub"), os.path.join(REF, "misc", "controllability"), os.path.join(REF, "misc", "coco-caption")]
        for tag, case in cases.items():
            arrays, m = run_set(case, tmp, tag)
            for k, v in arrays.items():
                out[f"{tag}_{k}"] = v
            meta["sets"][tag] = m
            print(tag, json.dumps(m["corpus"]), "worst vs fp64", m["worst_difference_reference_vs_fp64"], m["noun_iou_return_types"])
    np.savez_compressed(os.path.join(HERE, "controllability_case.npz"), **out)
    with open(os.path.join(HERE, "controllability_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote controllability_case.npz / controllability_meta.json:", os.path.getsize(os.path.join(HERE, "controllability_case.npz")), "bytes")


if __name__ == "__main__":
    main()
