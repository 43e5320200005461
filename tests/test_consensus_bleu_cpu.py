"""Consensus re-ranking, method 'bleu', without a GPU: the Python restatement of the device contract (subgc.consensus.bleu_pair_restatement /
bleu_rerank_restatement) against the fixture the reference's own calculate_bleu_sentence wrote (tests/golden/make_golden_consensus_bleu.py)
within the derived bounds of DESIGN 4.O (tests/consensus_bleu_golden.py), every planted edge, the seventh header and its binding, and the
host-side refusals."""
import ctypes

import numpy as np
import pytest
import torch

import consensus_bleu_golden as G
from subgc import _lib, consensus, ops
from subgc._lib import SubgcError

NAMES = {
    "subgc_consensus_bleu_cook": ["tok", "tok64", "woff", "T", "row_len", "bad", "bad_n", "S", "max_words", "keys", "counts", "cnt", "wlen",
                                  "stream"],
    "subgc_consensus_bleu_score": ["ckeys", "ccounts", "ccnt", "cwlen", "T", "seg", "I", "max_cand", "top_k", "nn", "nn_ld", "k", "cap_off",
                                   "n_img", "n_caps", "nwoff", "nkeys", "ncounts", "ncnt", "nwlen", "n", "fpr", "m", "max_caps", "sim",
                                   "pair_out", "pair_ld", "stream"],
}


@pytest.fixture(scope="module")
def case():
    meta, arr = G.load()
    _, ids = G.corpus_sentences(arr)
    cands = G.rows_to_ids(arr["cand"])
    b = arr["bounds"]
    res = {}
    for name, p in meta["sets"].items():
        res[name] = [consensus.bleu_rerank_restatement(cands[b[i]:b[i + 1]], ids, arr["nn"][i], meta["k"], p["m"], p["n"], p["fpr"])
                     for i in range(len(b) - 1)]
    return meta, arr, ids, res


@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_matches_the_reference_fixture_within_the_derived_bounds(case, name):
    meta, arr, ids, res = case
    p, b = meta["sets"][name], arr["bounds"]
    worst_p = worst_s = 0.0
    for i in range(len(b) - 1):
        pairs, sums, order = res[name][i]
        nc = int(arr["n_caps"][i])
        ref_p = arr["pairs_" + name][b[i]:b[i + 1]]
        assert pairs.shape[1] == nc and np.all(ref_p[:, nc:] == -1.0)           # the fixture's padding: this image has exactly these captions
        ref_s, ref_o = arr["sums_" + name][b[i]:b[i + 1]], arr["orders_" + name][b[i]:b[i + 1]]
        worst_p, worst_s = max(worst_p, G.worst_rel(pairs, ref_p[:, :nc])), max(worst_s, G.worst_rel(sums, ref_s))
        assert G.within(pairs, ref_p[:, :nc], G.pair_bound(p["n"])), i
        assert G.within(sums, ref_s, G.sim_bound(p["n"], min(p["m"], nc))), i
        # the order: the stable one; the reference's np.argsort(-sim) may differ from it among identical candidate rows only
        np.testing.assert_array_equal(order, np.argsort(-ref_s, kind="stable"))
        for x, y in zip(order, ref_o):
            assert x == y or np.array_equal(arr["cand"][b[i] + x], arr["cand"][b[i] + y])
        # nothing left unjudged: adjacent sums are equal (identical rows) or apart by more than the fixture's gap rule, far above the bound
        s = ref_s[order]
        for x in range(len(s) - 1):
            assert (s[x] == s[x + 1] and np.array_equal(arr["cand"][b[i] + order[x]], arr["cand"][b[i] + order[x + 1]])) or \
                   s[x] - s[x + 1] > meta["gap_rule"] * s[x]
    print(f"set {name}: worst |restatement - reference| / reference: pairs {worst_p / G.U:.2f} u (bound {G.pair_bound(p['n']) / G.U:.2f} u), "
          f"sums {worst_s / G.U:.2f} u")
    assert meta["gap_rule"] > 1e6 * G.sim_bound(4, 2048)


@pytest.mark.parametrize("name", ["A", "B"])
def test_edge_cases_one_by_one(case, name):
    meta, arr, ids, res = case
    G.check_edges(meta, arr, ids, name, [r[0] for r in res[name]], [r[1] for r in res[name]], [r[2] for r in res[name]])


def test_pair_restatement_spot_values_and_the_bounds():
    f = consensus.bleu_pair_restatement
    assert f([1, 2, 3], [1, 2, 3, 4], 4, 1.0) == 0.0 and f([1, 2, 3, 4], [1, 2, 3], 4, 1.0) == 0.0      # n > len: 0, whatever matches
    assert f([1, 2, 3], [1, 2, 3, 4], 3, 1.0) > 0.0 and f([], [], 1, 1.0) == 0.0
    assert f([1, 2, 3, 4], [1, 2, 3, 4], 4, 1.0) == 1.0 == f([1, 2], [1, 2], 2, 0.5)
    assert f([4, 3, 2, 1], [1, 2, 3, 4], 4, 1.0) == 0.25                                                # unigrams only, still / n
    assert f([1, 1, 5, 6], [1, 2, 3, 4, 7, 8], 1, 0.0) == 0.25                                          # fpr = 0: f = pre = 1 / 4 (clipped)
    assert f([1, 1, 5, 6], [1, 2, 3, 4, 7, 8], 1, 1.0) == (2 * 0.25 * (1 / 6.0)) / (1 / 6.0 + 0.25)
    # the bounds: a few u for a pair score, dominated by the 2 (terms - 1) u of the two descending sums for a sum
    assert G.pair_bound(4) == 6 * G.U / (1 - 6 * G.U) and G.pair_bound(1) < G.pair_bound(4) < 7 * G.U
    assert 354 * G.U < G.sim_bound(4, 175) < 355 * G.U and G.sim_bound(2, 1) == G.pair_bound(2)


def test_consensus_header_parses_and_the_other_six_are_untouched():
    protos = _lib.parse_header(_lib.CONSENSUS_HEADER)
    assert sorted(protos) == sorted(NAMES)
    for name, want in NAMES.items():
        ret, args = protos[name]
        assert ret is ctypes.c_int and [a for _, a in args] == want, name
        assert dict((a, t) for t, a in args)["stream"] is ctypes.c_void_p
    types = dict((a, t) for t, a in protos["subgc_consensus_bleu_score"][1])
    assert types["fpr"] is ctypes.c_double and types["n"] is ctypes.c_int and types["pair_ld"] is ctypes.c_int64
    # the addressing arguments are subgc_consensus_score's, the sentence arguments subgc_consensus_cook's
    core = _lib.parse_header()
    addressing = ["seg", "I", "max_cand", "top_k", "nn", "nn_ld", "k", "cap_off", "n_img", "n_caps", "nwoff", "max_caps", "sim", "pair_out", "pair_ld"]
    assert [a for _, a in core["subgc_consensus_score"][1] if a in addressing] == [a for a in NAMES["subgc_consensus_bleu_score"] if a in addressing] == addressing
    assert [a for _, a in core["subgc_consensus_cook"][1]][:9] == NAMES["subgc_consensus_bleu_cook"][:9]
    src = open(_lib.CONSENSUS_HEADER).read()
    assert src.count("bleu_score_util.py") >= 4 and src.count("consensus_reranking.py") >= 4 and "conf_cr.py:45-48" in src


FAKE = 1 << 20                                                           # never dereferenced: the argument checks come first


def _score(L, **over):
    a = dict(T=20, I=2, max_cand=4, top_k=0, nn_ld=60, k=60, n_img=100, n_caps=500, n=4, fpr=1.0, m=175, max_caps=300)
    a.update(over)
    return L.subgc_consensus_bleu_score(FAKE, FAKE, FAKE, FAKE, a["T"], FAKE, a["I"], a["max_cand"], a["top_k"], FAKE, a["nn_ld"], a["k"], FAKE,
                                        a["n_img"], a["n_caps"], FAKE, FAKE, FAKE, FAKE, FAKE, a["n"], a["fpr"], a["m"], a["max_caps"], FAKE,
                                        None, 0, None)


@pytest.mark.parametrize("over,what", [(dict(n=0), b"1 <= n <= 4 n-gram orders (got 0)"), (dict(n=5), b"1 <= n <= 4 n-gram orders (got 5)"),
                                       (dict(fpr=-0.5), b"fpr finite and >= 0 (got -0.5)"), (dict(fpr=float("nan")), b"fpr finite and >= 0 (got nan)"),
                                       (dict(fpr=float("inf")), b"fpr finite and >= 0 (got inf)"), (dict(m=0), b"m >= 1 (got 0)"),
                                       (dict(k=61), b"k = 61 is larger than the neighbour lists"), (dict(k=257, nn_ld=300), b"k <= 256 neighbour images (got 257)"),
                                       (dict(k=0), b"1 <= k <= 256"), (dict(max_caps=2049), b"at most 2048 neighbour captions"),
                                       (dict(T=65), b"T <= 64 (got 65)")])
def test_score_entry_point_refuses_on_the_host(over, what):
    L = _lib.lib()
    assert _score(L, **over) == -1
    err = L.subgc_last_error()
    assert b"consensus_bleu_score" in err and what in err, err


def test_cook_entry_point_refuses_on_the_host_and_nothing_to_do_is_ok():
    L = _lib.lib()
    rc = L.subgc_consensus_bleu_cook(FAKE, 0, FAKE, 0, None, None, 0, 10, 257, FAKE, FAKE, FAKE, FAKE, None)
    assert rc == -1 and b"consensus_bleu_cook: a sentence holds at most 256 words (got max_words = 257)" in L.subgc_last_error()
    rc = L.subgc_consensus_bleu_cook(FAKE, 1, None, 65, None, None, 0, 10, 0, FAKE, FAKE, FAKE, FAKE, None)
    assert rc == -1 and b"T <= 64 (got 65)" in L.subgc_last_error()
    rc = L.subgc_consensus_bleu_cook(None, 1, None, 20, None, None, 0, 10, 0, FAKE, FAKE, FAKE, FAKE, None)
    assert rc == -1 and b"consensus_bleu_cook: null pointer" in L.subgc_last_error()
    assert L.subgc_consensus_bleu_cook(None, 0, None, 20, None, None, 0, 0, 0, None, None, None, None, None) == 0
    assert _score(L, I=0) == 0 and _score(L, max_cand=0) == 0


def test_reranker_refuses_bad_ngram_fpr_m_and_k():
    class Host:                                                          # the host tables `neighbours` reads
        n_img = 70
        cap_off = np.arange(71, dtype=np.int64) * 40                     # 40 captions per image
    B = consensus.BleuConsensusReranker
    for ngram in (0, 5, 2.5, True):
        with pytest.raises(SubgcError, match=f"ngram = {ngram}"):
            B(Host, ngram=ngram)
    for fpr in (-1.0, float("nan"), float("inf")):
        with pytest.raises(SubgcError, match=f"fpr = {fpr}"):
            B(Host, fpr=fpr)
    with pytest.raises(SubgcError, match="m = 0"):
        B(Host, m=0)
    with pytest.raises(SubgcError, match="k = 300"):
        B(Host, k=300)
    with pytest.raises(SubgcError, match="k = 0"):
        B(Host, k=0)
    rr = B(Host, fpr=0, ngram=1)                                         # fpr = 0 is legal: f = pre
    assert (rr.k, rr.m, rr.ngram, rr.fpr) == (60, 175, 1, 0.0) and isinstance(rr.fpr, float)
    with pytest.raises(SubgcError, match=r"k = 60 is larger than the neighbour list of image 1 \(59 entries\)"):
        rr.neighbours([list(range(60)), list(range(59))])
    with pytest.raises(SubgcError, match=r"2400 neighbour captions; the limit is 2048"):
        rr.neighbours([list(range(60))])


def test_factory_defaults_per_method_and_the_refusal():
    class Host:
        n_img = 70
        cap_off = np.arange(71, dtype=np.int64)
    c = consensus.make_reranker(Host)
    assert type(c) is consensus.ConsensusReranker and (c.k, c.m) == (60, 125)                 # conf_cr.py:43-44
    c = consensus.make_reranker(Host, method="cider", k=10, m=5)
    assert type(c) is consensus.ConsensusReranker and (c.k, c.m) == (10, 5)
    b = consensus.make_reranker(Host, "bleu")
    assert type(b) is consensus.BleuConsensusReranker and (b.k, b.m, b.ngram, b.fpr) == (60, 175, 4, 1.0)    # conf_cr.py:45-48
    b = consensus.make_reranker(Host, method="bleu", ngram=2, fpr=0.5, m=20, k=30)
    assert (b.k, b.m, b.ngram, b.fpr) == (30, 20, 2, 0.5)
    with pytest.raises(SubgcError, match="method = 'meteor'; only support cider and bleu currently"):
        consensus.make_reranker(Host, method="meteor")
    with pytest.raises(TypeError):
        consensus.make_reranker(Host, method="cider", ngram=2)          # the 'cider' method has no such parameter


def test_cpu_tensors_and_a_host_only_corpus_are_refused():
    tok = torch.zeros(4, 20, dtype=torch.int64)
    with pytest.raises(SubgcError, match="device tensors"):
        ops.consensus_bleu_cook(tok)
    rr = consensus.BleuConsensusReranker.__new__(consensus.BleuConsensusReranker)
    with pytest.raises(SubgcError, match="device tensors"):
        rr.rerank(tok, [0, 4], [[0]])
    meta, arr = G.load()
    sents, _ = G.corpus_sentences(arr)
    corpus = consensus.ConsensusCorpus(sents, G.vocab(meta["V"]), device=None)              # images without captions are fine
    assert corpus.n_img == meta["n_img"] and corpus.max_words == 200 and corpus.n_ids > meta["V"]
    with pytest.raises(SubgcError, match="not on a device"):
        corpus.bleu_cooked()
