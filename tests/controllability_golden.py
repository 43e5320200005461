"""The controllability fixture (tests/golden/make_golden_controllability.py: written by the reference's own NounIoU and COCO scorers)
and a plain numpy restatement of the arithmetic that include/subgc_controllability_hip.h states, for the tests only."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = ["rnd", "exact", "edge", "edge_rbe", "edge_d1", "sct_subgc"]
U = 2.0 ** -24
F = np.float32


def load():
    with open(os.path.join(GOLDEN, "controllability_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "controllability_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def vocab(meta):
    bad = {int(k): v for k, v in meta["bad_endings"].items()}
    return {str(i): bad.get(i, f"w{i}") for i in range(1, meta["V"] + 1)}


def word(meta, i):
    v = vocab(meta)
    return v[str(i)] if i <= meta["V"] else f"w{i}"


def vectors(meta, arr, tag):
    """-> the {word: vector} dictionary the reference unpickled."""
    return {word(meta, int(i)): arr[tag + "_vec"][k] for k, i in enumerate(arr[tag + "_nouns"])}


def groups(meta, arr, tag):
    """-> the ground-truth groups as lists of caption strings (`sct_gt_captions.npy`'s shape)."""
    w, off, cap = arr[tag + "_gwords"], arr[tag + "_gwoff"], arr[tag + "_gcap_off"]
    names = {int(i): word(meta, int(i)) for i in set(w.tolist())}
    return [[" ".join(names[int(x)] for x in w[off[s]:off[s + 1]]) for s in range(cap[g], cap[g + 1])] for g in range(len(cap) - 1)]


def cook(meta, arr, tag, device=None):
    from subgc import controllability as C
    nouns = C.NounVectors(vectors(meta, arr, tag), vocab(meta), device=None)
    return C.ControlReferences(groups(meta, arr, tag), nouns, vocab(meta), device=device)


def predicted_rows(seq_row, tok_noun, bad_ids, rbe):
    """The word rule of the header on the host: ids before the first id <= 0, minus trailing bad endings unless every word is one, then
    the vector rows of the words that have one."""
    ids = []
    for x in seq_row:
        if x <= 0:
            break
        ids.append(int(x))
    if rbe:
        n = len(ids)
        while n and ids[n - 1] in bad_ids:
            n -= 1
        ids = ids if n == 0 else ids[:n]
    return [int(tok_noun[i]) for i in ids if i < len(tok_noun) and tok_noun[i] >= 0]


def pairs_of(refs, arr, tag, meta):
    """-> per pair (row, ground-truth vector rows, predicted vector rows), in the order of the device's pair slots."""
    seq, rg = arr[tag + "_seq"], arr[tag + "_row_group"]
    bad = {int(k) for k in meta["bad_endings"]}
    out = []
    for r, g in enumerate(rg):
        if g < 0:
            continue
        pw = predicted_rows(seq[r], refs.tok_noun, bad, meta["sets"][tag]["remove_bad_endings"])
        for c in range(refs.gcap_off[g], refs.gcap_off[g + 1]):
            out.append((r, refs.gn[refs.gn_off[c]:refs.gn_off[c + 1]].tolist(), pw))
    return out


def matrix(vec, norm, gt, pred):
    """The stated arithmetic: fp64 dot products accumulated over k = 0 .. d-1 in order, cos = dot / max(norm_a * norm_b, 1e-8) in fp64
    rounded once to fp32, s = (cos + 1) / 2 in fp32.  -> fp32 [m, n]."""
    a, b = vec[gt].astype(np.float64), vec[pred].astype(np.float64)
    acc = np.zeros((len(gt), len(pred)), np.float64)
    for k in range(vec.shape[1]):
        acc = acc + a[:, k, None] * b[None, :, k]
    den = norm[gt][:, None] * norm[pred][None, :]
    cos = (acc / np.maximum(den, 1e-8)).astype(F)
    return (cos + F(1)) / F(2)


def pair_value(S, assign):
    """I = the sequential fp32 sum of the chosen entries over the ground-truth words in ascending order; iou = I / ((m + n) - I) in fp32."""
    m, n = S.shape
    if m == 0:
        return F(1)
    if n == 0:
        return F(0)
    I = F(0)
    for i in range(m):
        if assign[i] >= 0:
            I = F(I + S[i, assign[i]])
    return F(I / F(F(m + n) - I))


def row_value(values):
    s = F(0)
    for x in values:
        s = F(s + F(x))
    return F(s / F(len(values))) if len(values) else F(0)


def scipy_assign(S):
    """An optimal assignment of the fp32 matrix (solved in fp64) -> (assign [m], its fp64 value)."""
    from scipy.optimize import linear_sum_assignment
    m, n = S.shape
    assign = np.full(m, -1, np.int64)
    if m == 0 or n == 0:
        return assign, 0.0
    rr, cc = linear_sum_assignment(-S.astype(np.float64))
    assign[rr] = cc
    return assign, float(S.astype(np.float64)[rr, cc].sum())


def restate_set(refs, arr, tag, meta):
    """The whole set on the host with scipy's assignment -> (pair values fp32, pair (m, n), row values fp32 [rows])."""
    nv = refs.nouns
    pv, mn, per_row = [], [], {}
    for r, gt, pw in pairs_of(refs, arr, tag, meta):
        S = matrix(nv.vec, nv.norm, gt, pw)
        x = pair_value(S, scipy_assign(S)[0])
        pv.append(x)
        mn.append([len(gt), len(pw)])
        per_row.setdefault(r, []).append(x)
    rows = np.array([row_value(per_row.get(r, [])) for r in range(len(arr[tag + "_row_group"]))], F)
    return np.array(pv, F), np.array(mn, np.int32).reshape(-1, 2), rows


def pair_bound(d, m, n):
    """|device - reference| of one pair <= (2 (d + 6) + 4 (k - 1) + 6) * 2^-24, k = min(m, n); 0 for the trivial pairs."""
    k = min(m, n)
    return 0.0 if k == 0 else (2 * (d + 6) + 4 * (k - 1) + 6) * U


def row_bound(d, mn):
    """... of a group mean over the pairs `mn`: the largest pair bound + 2 (L + 1) * 2^-24."""
    return max([pair_bound(d, m, n) for m, n in mn] + [0.0]) + 2 * (len(mn) + 1) * U


def accuracy_entries(arr, tag):
    """The fixture's BLEU material and values of the live rows as `AccuracyScorer.unpack`-style entries (one candidate per group)."""
    out = []
    for mat, val in zip(arr[tag + "_acc_row_i"].astype(np.int64), arr[tag + "_acc_row_d"]):
        out.append({"n": 1, "considered": 1, "material": mat[None], "values": val[None], "oracle_rows": np.zeros(4, np.int64),
                    "oracle_material": np.repeat(mat[None], 4, 0), "oracle_values": val, "top1_row": 0, "top1_material": mat, "top1_values": val})
    return out


def reference_entries(arr, tag):
    """The fixture's per-row reference values as `ControlScorer.unpack`-style entries (rows without a group included)."""
    acc = iter(accuracy_entries(arr, tag))
    out = []
    for g, x in zip(arr[tag + "_row_group"], arr[tag + "_row_iou"]):
        out.append({"group": int(g), "noun_iou": F(x) if g >= 0 else F(0), "accuracy": next(acc) if g >= 0 else None})
    return out
