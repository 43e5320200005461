"""Helpers of the nearest-image search tests: the fixture written by tests/golden/make_golden_neighbours.py (the reference's own
`find_NNimg` run on synthetic features) and the tie rule the lists are judged by.

Inputs.  Full-mantissa random features do not compress, and the fixture must stay far below a megabyte, so only the small cases store
their feature matrices (float64, `<name>_te` / `<name>_tr`).  The larger cases store a RECIPE in the meta -- the seed of a
`numpy.random.RandomState` (the legacy generator, whose streams numpy guarantees never to change), the distribution and a list of
edits -- plus the SHA-256 of the float32 matrices the recipe yields; `features` rebuilds them and refuses a mismatch.  Values are
float32 (exact in float64), so the summation is rounded at every step and a wrong order of additions shows.  The reference's outputs
(lists, the cdist matrix) are always stored."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEY_MASK = np.uint64(0x7FFFFFFFFFFFFFFF)


def load():
    """-> (meta dict, arrays dict) of the committed fixture."""
    with open(os.path.join(GOLDEN, "neighbours_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "neighbours_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def build(recipe):
    """A recipe -> (te, tr) float32.  kind 'normal': standard normal; 'relu': max(normal, 0), non-negative like ResNet pool features.
    Edits, in order: ['dup_train', dst, src]: train row dst becomes a copy of train row src; ['query_is_train', i, j]: query i becomes
    train row j."""
    Q, N, D = recipe["shape"]
    rs = np.random.RandomState(recipe["seed"])
    te = rs.standard_normal((Q, D)).astype(np.float32)
    tr = rs.standard_normal((N, D)).astype(np.float32)
    if recipe["kind"] == "relu":
        te, tr = np.maximum(te, 0), np.maximum(tr, 0)
    for op, a, b in recipe.get("edits", []):
        if op == "dup_train":
            tr[a] = tr[b]
        elif op == "query_is_train":
            te[a] = tr[b]
        else:
            raise ValueError(op)
    return te, tr


def digest(te, tr):
    return hashlib.sha256(np.ascontiguousarray(te).tobytes() + np.ascontiguousarray(tr).tobytes()).hexdigest()


_CACHE = {}


def features(meta, arr, name):
    """-> (te, tr) float64 of case `name`: stored matrices, or the recipe's, checked against the recorded digest.  Built once."""
    if name not in _CACHE:
        case = meta["cases"][name]
        if "recipe" in case:
            te, tr = build(case["recipe"])
            if digest(te, tr) != case["sha256"]:
                raise AssertionError(f"neighbours fixture: the recipe of case {name} no longer yields the recorded features")
        else:
            te, tr = arr[name + "_te"], arr[name + "_tr"]
        te, tr = np.ascontiguousarray(te, np.float64), np.ascontiguousarray(tr, np.float64)
        te.setflags(write=False); tr.setflags(write=False)
        _CACHE[name] = (te, tr)
    return _CACHE[name]


def keys(dist):
    return np.ascontiguousarray(dist, np.float64).view(np.uint64) & KEY_MASK


def tie_positions(dist_row, k):
    """Boolean [k]: list position p lies inside a group of exactly equal keys of the row's FULL ascending order (a group that straddles
    the k-th cut counts for its positions inside the list)."""
    s = np.sort(keys(dist_row))
    same = s[1:] == s[:-1]
    tied = np.zeros(len(s), bool)
    tied[1:] |= same
    tied[:-1] |= same
    return tied[:k]


def compare_lists(got, ref, dist, k):
    """The tie rule: `got` [Q, k] against the reference lists `ref` [Q, >= k] given the reference distances `dist` [Q, N].  Outside
    exact-tie groups every position must hold the reference's index; a tie group that lies wholly inside the list must hold the
    reference's SET of indices; inside any tie group `got` must be in ascending index.  -> the number of positions left out as ties."""
    got, ref = np.asarray(got)[:, :k], np.asarray(ref)[:, :k]
    left_out = 0
    for i in range(got.shape[0]):
        ky = keys(dist[i])
        tied = tie_positions(dist[i], k)
        assert (got[i][~tied] == ref[i][~tied]).all(), (i, np.flatnonzero((got[i] != ref[i]) & ~tied)[:5])
        left_out += int(tied.sum())
        full = np.sort(ky)
        p = 0
        while p < k:
            if not tied[p]:
                p += 1
                continue
            e = p
            while e < len(full) and full[e] == full[p]:
                e += 1                                                   # the group [p, e) of the full order
            end = min(e, k)
            assert (ky[got[i][p:end]] == full[p]).all(), (i, p)          # every listed index does carry the group's distance
            assert (np.diff(got[i][p:end]) > 0).all(), (i, p, "equal distances must come in ascending index")
            if e <= k:
                assert set(got[i][p:e].tolist()) == set(ref[i][p:e].tolist()), (i, p)
            else:
                members = np.flatnonzero(ky == full[p])                  # across the cut: the lowest indices of the group are kept
                assert got[i][p:end].tolist() == members[:end - p].tolist(), (i, p)
            p = end
    return left_out
