#!/usr/bin/env python
"""Write the fixture of the nearest-image search by RUNNING THE REFERENCE's own `Consensus_Reranking.find_NNimg`
(misc/consensus_reranking/concensus_reranking_utils/consensus_reranking.py:59-119; imported from where the reference lies, never
copied): neighbours_case.npz + neighbours_meta.json.  Data only: synthetic feature matrices (or the recipe that yields them, see
tests/neighbours_golden.py), the reference's neighbour lists, and the float64 matrix of the `cdist` call the method makes.

    python tests/golden/make_golden_neighbours.py

consensus_reranking.py imports pycocotools / pycocoevalcap (COCO evaluation, not used by find_NNimg) and bleu_score_util.py imports
nltk; none is installed where this fixture is made, so STAND-IN modules with those names are registered before the import, the way
make_golden_consensus_bleu.py stands in for nltk.  scipy and numpy are the real ones.  For every case the method runs twice, with
`cal_distance_all` True (one cdist, :105-108) and False (one row at a time, :110-117), on temporary `dct_feat` / annotation data in a
temporary directory; `num_NNimg` is the case's largest k (shorter lists are prefixes: `[:, :num_NNimg]`).  If the module cannot be
imported even with the stand-ins, the lists are written by the two calls the method makes (cdist, np.argsort) and the meta says so.

Cases (Q, N, D), each aimed at one way of going wrong:
  plain      (5, 97, 7)      k = 1, 10, 97       nothing special; every size off every tile
  dup        (65, 600, 300)  k = 100             non-negative ReLU-like features; 10 duplicated train rows, so exact tie groups lie inside
                                                 the lists and one lies across the k-th cut
  wide       (3, 1001, 2048) k = 1000            the reference's own D and (nearly) its num_NNimg
  long       (1, 4099, 64)   k = 1024            more than one pass of every row loop; a query equal to a train row (distance 0)
  nonfinite  (4, 70, 9)      k = 70              a train row of 1e200 (distance +inf); a query with inf against a train row with inf in
                                                 the same column (NaN, sorted last)
  alldup     (3, 40, 5)      k = 7, 40           every train row the same: every distance of a row equal
The meta records per case whether tests' numpy restatement (subgc.neighbours.find_nn_restatement) gives scipy's distances bit for bit,
whether the two branches agree, and how many list positions lie inside exact-tie groups."""
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "sub-gc_amd")]


def stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    unused = type("Unused", (), {})
    mod("pycocotools"); mod("pycocotools.coco", COCO=unused)
    mod("pycocoevalcap"); mod("pycocoevalcap.eval", COCOEvalCap=unused); mod("pycocoevalcap.eval_pair_cider", COCOEvalCapPairCider=unused)
    nltk = mod("nltk"); nltk.util = mod("nltk.util", ngrams=lambda seq, n: [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)])
    return ["pycocotools.coco.COCO", "pycocoevalcap.eval.COCOEvalCap", "pycocoevalcap.eval_pair_cider.COCOEvalCapPairCider", "nltk.util.ngrams"]


def import_reference():
    stood = stand_ins()
    sys.path.insert(0, os.path.join(REF, "misc", "consensus_reranking"))
    try:
        from concensus_reranking_utils.consensus_reranking import Consensus_Reranking
        return Consensus_Reranking, stood
    except Exception as e:                                               # noqa: BLE001 -- recorded in the meta
        print("the reference module does not import even with stand-ins:", repr(e))
        return None, stood


def run_reference(CR, te, tr, k, all_rows):
    """find_NNimg on temporary files -> (lists, the arranged float64 arrays the method saved)."""
    from scipy.spatial import distance
    if CR is None:
        d = distance.cdist(te, tr, "euclidean")
        return np.argsort(d, axis=1)[:, :k].tolist(), te, tr
    with tempfile.TemporaryDirectory(prefix="nn_golden_") as tmp:
        ids_tr, ids_te = [f"tr{j:05d}" for j in range(len(tr))], [f"te{i:03d}" for i in range(len(te))]
        dct = {**{n: tr[j] for j, n in enumerate(ids_tr)}, **{n: te[i] for i, n in enumerate(ids_te)}}
        np.save(os.path.join(tmp, "dct_feat.npy"), dct, allow_pickle=True)
        cr = CR(types.SimpleNamespace(dataset="flickr30k", split="karpathy", converted_file="none.npy", output_folder=tmp))
        assert cr.conf.distance_metric == "euclidean"
        cr.conf.fname_dct_feat = os.path.join(tmp, "dct_feat.npy")
        cr.conf.dim_image_feat, cr.conf.num_NNimg, cr.conf.cal_distance_all = te.shape[1], k, all_rows
        cr.anno_list_ref = [{"id": n} for n in ids_tr]
        cr.anno_list_hypo = [{"id": n} for n in ids_te]
        cr.find_NNimg()
        cache = os.path.join(tmp, cr.conf.name_cache)
        return cr.NNimg_list, np.load(os.path.join(cache, "101_arr_te.npy")), np.load(os.path.join(cache, "101_arr_tr.npy"))


def dup_recipe():
    """The duplicate case: nine duplicates of rows that sit near the head of many lists, and a tenth chosen so that, for query 1, a tie
    group lies across the cut at k = 100 (positions 99 and 100 of the full order)."""
    import neighbours_golden as G
    from scipy.spatial import distance
    base = {"shape": [65, 600, 300], "kind": "relu", "seed": 20261021, "edits": []}
    te, tr = G.build(base)
    edits = [["query_is_train", 3 + 2 * j, 11 * j + 4] for j in range(9)]               # some queries ARE train rows: distance 0, twice
    edits += [["dup_train", 590 + j, 11 * j + 4] for j in range(9)]
    te0, tr0 = G.build(dict(base, edits=edits))
    order = np.argsort(distance.cdist(te0[1:2].astype(np.float64), tr0.astype(np.float64)), axis=1, kind="stable")[0]
    for src_rank in range(90, 110):
        src = int(order[src_rank])
        if src >= 590:
            continue
        trial = dict(base, edits=edits + [["dup_train", 599, src]])
        te1, tr1 = G.build(trial)
        d = distance.cdist(te1[1:2].astype(np.float64), tr1.astype(np.float64))[0]
        s = np.sort(d)
        if s[99] == s[100] and s[98] != s[99] and s[100] != s[101]:
            return trial
    raise AssertionError("no duplicate puts a tie across the cut: change the seed")


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    import scipy
    from scipy.spatial import distance
    import neighbours_golden as G
    from subgc.neighbours import find_nn_restatement
    CR, stood = import_reference()

    rs = np.random.RandomState(7)
    cases = {
        "plain": {"ks": [1, 10, 97], "stored": (rs.standard_normal((5, 7)), rs.standard_normal((97, 7)))},
        "dup": {"ks": [100], "recipe": dup_recipe(), "duplicates": True},
        "wide": {"ks": [1000], "recipe": {"shape": [3, 1001, 2048], "kind": "relu", "seed": 20261022, "edits": []}},
        "long": {"ks": [1024], "recipe": {"shape": [1, 4099, 64], "kind": "normal", "seed": 20261023, "edits": [["query_is_train", 0, 4097]]}},
    }
    te, tr = rs.standard_normal((4, 9)), rs.standard_normal((70, 9))
    tr[3] = 1e200
    te[2, 4] = np.inf; tr[5, 4] = np.inf
    cases["nonfinite"] = {"ks": [70], "stored": (te, tr), "nonfinite": True}
    cases["alldup"] = {"ks": [7, 40], "stored": (rs.standard_normal((3, 5)), np.tile(rs.standard_normal((1, 5)), (40, 1))), "all_duplicates": True}

    out, meta_cases = {}, {}
    for name, c in cases.items():
        if "recipe" in c:
            f32 = G.build(c["recipe"])
            te, tr = f32[0].astype(np.float64), f32[1].astype(np.float64)
        else:
            te, tr = c["stored"]
            out[name + "_te"], out[name + "_tr"] = te, tr
        k = max(c["ks"])
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            lists_all, a_te, a_tr = run_reference(CR, te, tr, k, True)
            lists_row, _, _ = run_reference(CR, te, tr, k, False)
            assert a_te.dtype == np.float64 and a_te.tobytes() == te.tobytes() and a_tr.tobytes() == tr.tobytes()
            d = distance.cdist(a_te, a_tr, "euclidean")                  # the call of :105 on the arrays the method arranged
            d_row = np.concatenate([distance.cdist(a_te[i:i + 1], a_tr, "euclidean") for i in range(len(te))])      # :113
            r_lists, r_dist = find_nn_restatement(te, tr, k)
        lists_all, lists_row = np.asarray(lists_all, np.int32), np.asarray(lists_row, np.int32)
        assert (np.argsort(d, axis=1)[:, :k] == lists_all).all()
        tied = sum(int(G.tie_positions(d[i], k).sum()) for i in range(len(te)))
        G.compare_lists(r_lists, lists_all, d, k)                        # the restatement's lists are the reference's under the tie rule
        out[name + "_lists"], out[name + "_cdist"] = lists_all, d
        m = {"shape": [len(te), len(tr), te.shape[1]], "ks": c["ks"], "num_NNimg": k,
             "branches_agree": bool((lists_all == lists_row).all()), "branch_distances_bit_equal": d.tobytes() == d_row.tobytes(),
             "restatement_distances_bit_equal_scipy": bool((G.keys(r_dist) == G.keys(d)).all() and (np.isnan(r_dist) == np.isnan(d)).all()),
             "tie_positions": tied, "list_positions": int(lists_all.size),
             "positions_differing_from_stable_order": int((r_lists != lists_all).sum()),
             "duplicates": bool(c.get("duplicates")), "all_duplicates": bool(c.get("all_duplicates")), "nonfinite": bool(c.get("nonfinite"))}
        if "recipe" in c:
            m["recipe"], m["sha256"] = c["recipe"], G.digest(*f32)
        meta_cases[name] = m
        print(name, {k_: v for k_, v in m.items() if k_ not in ("recipe", "sha256")})
    np.savez_compressed(os.path.join(HERE, "neighbours_case.npz"), **out)
    with open(os.path.join(HERE, "neighbours_meta.json"), "w") as f:
        json.dump({"cases": meta_cases,
                   "written_by": "the reference's Consensus_Reranking.find_NNimg" if CR is not None else
                                 "the two calls find_NNimg makes (cdist, np.argsort): the module did not import even with stand-ins",
                   "stand_ins": stood, "scipy": scipy.__version__, "numpy": np.__version__, "python": sys.version.split()[0],
                   "tie_rule": "*_lists hold the reference's np.argsort order; inside groups of exactly equal distances it is unspecified, "
                               "the device order is ascending index"}, f, indent=1)
    print("wrote neighbours_case.npz:", os.path.getsize(os.path.join(HERE, "neighbours_case.npz")), "bytes")


if __name__ == "__main__":
    main()
