"""Controllability scores without a GPU: the fourth header and its binding, the cooked tables of subgc.controllability, the cook's
refusals, `summarize` and `score_predictions`' re-ordering, and the numpy restatement of the stated arithmetic against the fixture the
reference's own NounIoU wrote (tests/golden/make_golden_controllability.py)."""
import ctypes

import numpy as np
import pytest

import accuracy_golden as A
import controllability_golden as G
from subgc import _lib, controllability as C
from subgc.controllability import SubgcError

N_ARGS = 26


@pytest.fixture(scope="module")
def case():
    return G.load()


@pytest.fixture(scope="module")
def cooked(case):
    meta, arr = case
    memo = {}

    def get(tag):
        if tag not in memo:
            memo[tag] = G.cook(meta, arr, tag)
        return memo[tag]
    return get


def test_controllability_header_parses_and_the_other_three_are_untouched():
    protos = _lib.parse_header(_lib.CONTROLLABILITY_HEADER)
    assert sorted(protos) == ["subgc_control_noun_iou"]
    args = protos["subgc_control_noun_iou"][1]
    assert [a for _, a in args] == [
        "tok", "tok64", "T", "bad", "bad_n", "rows", "tok_noun", "n_tok_noun", "vec", "norm", "n_noun", "d", "row_group", "n_groups", "pair_off",
        "n_pairs", "gcap_off", "n_caps", "gn_off", "gn", "n_gn", "iou", "pair_iou", "pair_mn", "assign", "stream"]
    assert len(args) == N_ARGS and args[2][0] is ctypes.c_int and args[9][0] is ctypes.c_void_p
    src = open(_lib.CONTROLLABILITY_HEADER).read()
    assert f"#define SUBGC_CTL_MAX_WORDS {C.MAX_WORDS} " in src and C.MAX_WORDS == 64
    assert "1e-8" in src and C.COS_EPS == 1e-8


def _args(**over):
    a = dict(tok=None, tok64=0, T=8, bad=None, bad_n=0, rows=0, tok_noun=None, n_tok_noun=0, vec=None, norm=None, n_noun=0, d=1, row_group=None,
             n_groups=0, pair_off=None, n_pairs=0, gcap_off=None, n_caps=0, gn_off=None, gn=None, n_gn=0, iou=None, pair_iou=None, pair_mn=None,
             assign=None, stream=None)
    a.update(over)
    return list(a.values())


def test_each_invoker_knows_only_its_own_header_and_arguments_are_validated_on_the_host():
    _lib.call_controllability("subgc_control_noun_iou", *_args())             # no rows: nothing to do, nothing launched
    with pytest.raises(SubgcError, match="1 <= T <= 64 .got 65."):
        _lib.call_controllability("subgc_control_noun_iou", *_args(T=65))
    with pytest.raises(SubgcError, match="1 <= T <= 64 .got 0."):
        _lib.call_controllability("subgc_control_noun_iou", *_args(T=0))
    with pytest.raises(SubgcError, match="d >= 1 .got 0."):
        _lib.call_controllability("subgc_control_noun_iou", *_args(d=0))
    with pytest.raises(SubgcError, match="rows, n_tok_noun"):
        _lib.call_controllability("subgc_control_noun_iou", *_args(rows=-1))
    with pytest.raises(SubgcError, match="3 ground-truth vector words without a vector table"):
        _lib.call_controllability("subgc_control_noun_iou", *_args(n_gn=3))
    with pytest.raises(SubgcError, match="null pointer"):
        _lib.call_controllability("subgc_control_noun_iou", *_args(rows=2))


@pytest.mark.parametrize("tag", G.SETS)
def test_cooked_tables_match_the_fixture(case, cooked, tag):
    meta, arr = case
    refs = cooked(tag)
    nv = refs.nouns
    nouns = arr[tag + "_nouns"].tolist()
    V = meta["V"]
    assert nv.vec.dtype == np.float32 and np.array_equal(nv.vec, arr[tag + "_vec"]) and nv.d == meta["sets"][tag]["d"]
    assert nv.words == [G.word(meta, i) for i in nouns]
    assert nv.norm.dtype == np.float64
    np.testing.assert_allclose(nv.norm, np.linalg.norm(arr[tag + "_vec"].astype(np.float64), axis=1), rtol=4 * nv.d * 2.0 ** -53)
    want = [-1] + [nouns.index(i) if i in nouns else -1 for i in range(1, V + 1)]
    assert nv.tok_noun.tolist() == want and refs.tok_noun[:V + 1].tolist() == want
    # the ids the accuracy cook gives to reference-only words reach the same vector rows
    for w, k in refs.accuracy.word_to_ix.items():
        assert refs.tok_noun[k] == nv.word_row.get(w, -1)
    np.testing.assert_array_equal(refs.gcap_off, arr[tag + "_gcap_off"])
    w, off = arr[tag + "_gwords"], arr[tag + "_gwoff"]
    per_cap = [[nouns.index(int(x)) for x in w[off[s]:off[s + 1]] if int(x) in nouns] for s in range(len(off) - 1)]
    assert refs.gn.tolist() == [x for c in per_cap for x in c] and refs.gn.dtype == np.int32
    np.testing.assert_array_equal(np.diff(refs.gn_off), [len(c) for c in per_cap])
    assert (refs.n_groups, refs.n_caps, refs.n_gn) == (len(refs.gcap_off) - 1, len(off) - 1, len(refs.gn))
    assert refs.accuracy.n_img == refs.n_groups and refs.accuracy.n_caps == refs.n_caps                  # the "images" are the groups
    # the plan's pairs and the m, n of the host word rule are the reference's
    sc = C.ControlScorer(refs)
    plan = sc.plan(arr[tag + "_row_group"].tolist())
    assert plan["P"] == meta["sets"][tag]["pairs"] == len(arr[tag + "_pair_iou"])
    np.testing.assert_array_equal([[len(g), len(p)] for _, g, p in G.pairs_of(refs, arr, tag, meta)], arr[tag + "_pair_mn"])


def test_the_planted_cases_are_in_the_fixture(case, cooked):
    meta, arr = case
    e = meta["edges"]
    for name in ("m_is_0", "n_is_0", "both_0", "m_64_n_64", "m_64_n_1", "m_1_n_64", "all_ties", "repeated_on_both_sides", "antiparallel",
                 "identical_vectors", "zero_vector", "bad_endings_with_a_vector", "only_bad_endings", "no_group", "six_captions"):
        assert name in e, name
    refs = cooked("edge")
    rg, pair_off = arr["edge_row_group"], C.ControlScorer(refs).plan(arr["edge_row_group"].tolist())["pair_off"]
    mn, ref = arr["edge_pair_mn"], arr["edge_pair_iou"]
    first = lambda name: int(pair_off[e[name]])
    assert mn[first("m_is_0")].tolist()[0] == 0 and ref[first("m_is_0")] == 1.0
    assert mn[first("n_is_0")].tolist() == [2, 0] and ref[first("n_is_0")] == 0.0
    assert mn[first("both_0")].tolist() == [0, 0] and ref[first("both_0")] == 1.0
    assert mn[first("m_64_n_64")].tolist() == [64, 64] and mn[first("m_64_n_1")].tolist() == [64, 1] and mn[first("m_1_n_64")].tolist() == [1, 64]
    assert rg[e["no_group"]] == -1 and np.isnan(arr["edge_row_iou"][e["no_group"]])
    # every similarity is 1; antiparallel: s = 0; identical vectors: both predicted words find a perfect partner -- up to the reference's
    # own fp32 cosine, which is not exactly +-1 for parallel vectors
    for name, want in (("all_ties", 3.0 / (4 + 3 - 3.0)), ("antiparallel", 0.0), ("identical_vectors", 2.0 / (2 + 2 - 2.0))):
        assert abs(ref[first(name)] - want) <= G.pair_bound(50, *mn[first(name)]), name
    S = G.matrix(refs.nouns.vec, refs.nouns.norm, [refs.nouns.word_row["w22"]], [refs.nouns.word_row["w1"], refs.nouns.word_row["w22"]])
    assert S.tolist() == [[0.5, 0.5]]                                                       # the zero vector: the clamped denominator
    # bad endings: removed in edge_rbe, kept in edge -- the same rows, different n
    p = first("bad_endings_with_a_vector")
    assert arr["edge_pair_mn"][p].tolist() == [3, 4] and arr["edge_rbe_pair_mn"][p].tolist() == [3, 2]
    p = first("only_bad_endings")
    assert arr["edge_pair_mn"][p].tolist() == arr["edge_rbe_pair_mn"][p].tolist() == [2, 2]
    assert meta["sets"]["edge_d1"]["d"] == 1 and meta["sets"]["rnd"]["d"] == 300 and meta["sets"]["exact"]["d"] == 50
    assert "STAND-IN" in meta["assignment_solver"] and set(meta["versions"]) == {"numpy", "torch", "scipy"}
    for tag in G.SETS:
        assert 0.0 <= meta["sets"][tag]["worst_difference_reference_vs_fp64"] < 1e-6


def test_cook_refusals(case):
    meta, arr = case
    voc = G.vocab(meta)
    vecs = {"w1": np.ones(3, np.float32), "w2": np.arange(3, dtype=np.float32), "w60": np.ones(3, np.float32)}
    nouns = C.NounVectors(vecs, voc, device=None)
    assert nouns.n_noun == 3 and nouns.d == 3 and nouns.tok_noun[1] == 0 and nouns.tok_noun[2] == 1 and (nouns.tok_noun[3:] == -1).all()
    with pytest.raises(ValueError, match="caption 1 of group 2 has 65 words with a vector; the limit is 64"):
        C.ControlReferences([["w1"], ["w3 w2"], ["w2", " ".join(["w1", "w60"] * 32 + ["w2"])]], nouns, voc, device=None)
    ok = C.ControlReferences([[" ".join(["w1", "w60"] * 32)], ["w3  w1"]], nouns, voc, device=None)      # the limit itself; a double space
    assert ok.n_gn == 65 and np.diff(ok.gn_off).tolist() == [64, 1]
    with pytest.raises(ValueError, match="group 1 has no ground-truth caption"):
        C.ControlReferences([["w1"], []], nouns, voc, device=None)
    with pytest.raises(ValueError, match="no ground-truth groups"):
        C.ControlReferences([], nouns, voc, device=None)
    with pytest.raises(ValueError, match=r"the vector of 'w2' has shape \(4,\)"):
        C.NounVectors({"w1": np.ones(3), "w2": np.ones(4)}, voc, device=None)
    with pytest.raises(ValueError, match="the vector of 'w2' has non-finite entries"):
        C.NounVectors({"w1": np.ones(3), "w2": np.array([1.0, np.inf, 0.0])}, voc, device=None)
    with pytest.raises(ValueError, match="the vector of 'w1' has non-finite entries"):
        C.NounVectors({"w1": np.array([np.nan, 1.0])}, voc, device=None)
    with pytest.raises(ValueError, match="no word vectors"):
        C.NounVectors({}, voc, device=None)
    sc = C.ControlScorer(ok)
    with pytest.raises(SubgcError, match="row 1 names group 2; the references hold 2 groups"):
        sc.plan([0, 2])
    assert sc.plan([1, -1, 0])["pair_off"].tolist() == [0, 1, 1, 2]


@pytest.mark.parametrize("tag", G.SETS)
def test_summarize_reproduces_the_reference_corpus_numbers(case, tag):
    meta, arr = case
    entries = G.reference_entries(arr, tag)
    s = C.summarize(entries)
    n = meta["sets"][tag]["live_rows"]
    assert s["rows"] == n and s["left_out"] == meta["sets"][tag]["rows"] - n
    assert isinstance(s["Noun_IoU"], np.float32) and s["Noun_IoU"] == arr[tag + "_corpus_iou_f32"]               # equal bits
    # the script's own np.mean: the same bits when every per-row score is an fp32 value; where a row of trivial pairs only made a Python
    # float the script's list is averaged in fp64, and the two means differ by the fp32 summation error of n values in [0, 1]
    if meta["sets"][tag]["every_row_score_is_float32"]:
        assert float(s["Noun_IoU"]) == float(arr[tag + "_corpus_iou"])
    assert abs(float(s["Noun_IoU"]) - float(arr[tag + "_corpus_iou"])) <= (n + 2) * G.U
    want = arr[tag + "_acc_corpus"]
    assert A.rel([s[f"Bleu_{k}"] for k in range(1, 5)], want[:4]) <= A.BLEU_TOL
    assert A.rel([s["CIDEr"]], [want[4]]) <= A.CIDER_TOL and A.rel([s["ROUGE_L"]], [want[5]]) <= A.ROUGE_TOL
    assert C.summarize([]) == {"rows": 0, "left_out": 0}


def test_order_captions_follows_order_list():
    preds = [{"image_id": 7, "caption": ["a", "b"]}, {"image_id": "3", "caption": ["c"]}, {"image_id": 9, "caption": ["d", "e", "f"]}]
    caps, ids = C.order_captions(preds, ["9", "7", "3"])
    assert caps == ["d", "e", "f", "a", "b", "c"] and ids == ["9", "9", "9", "7", "7", "3"]
    assert C.order_captions(preds, [3, 9])[0] == ["c", "d", "e", "f"]                        # ids compare as strings, like the script's
    with pytest.raises(ValueError, match="order_list names image '5'"):
        C.order_captions(preds, ["5"])


@pytest.mark.parametrize("tag", ["exact", "rnd", "edge", "edge_d1"])
def test_the_restatement_agrees_with_the_reference(case, cooked, tag):
    """Keeps the restatement honest without a GPU: the stated arithmetic with scipy's assignment against NounIoU's own values, within
    the derived bounds of DESIGN 4.K."""
    meta, arr = case
    refs = cooked(tag)
    pv, mn, rows = G.restate_set(refs, arr, tag, meta)
    np.testing.assert_array_equal(mn, arr[tag + "_pair_mn"])
    d = refs.nouns.d
    worst = 0.0
    for x, want, (m, n) in zip(pv, arr[tag + "_pair_iou"], mn):
        assert abs(float(x) - want) <= G.pair_bound(d, m, n), (m, n, x, want)
        worst = max(worst, abs(float(x) - want))
    print(tag, "worst pair difference restatement vs reference", worst)
    plan = C.ControlScorer(refs).plan(arr[tag + "_row_group"].tolist())
    for r, g in enumerate(arr[tag + "_row_group"]):
        a, b = plan["pair_off"][r], plan["pair_off"][r + 1]
        if g < 0:
            assert rows[r] == 0 and a == b
        else:
            assert abs(float(rows[r]) - arr[tag + "_row_iou"][r]) <= G.row_bound(d, mn[a:b])
