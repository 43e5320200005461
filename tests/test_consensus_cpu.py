"""Consensus re-ranking without a GPU: the numpy restatement (tests/consensus_golden.py) against the fixture the reference's own
CiderScorer wrote, the host tables of subgc.consensus.ConsensusCorpus (id map, n-gram keys, document frequencies), the host-side
refusals of the three entry points and the consensus_rerank_ind writer."""
import numpy as np
import pytest
import torch

import consensus_golden as G
from subgc import _lib, consensus, ops


@pytest.fixture(scope="module")
def case():
    meta, arr = G.load()
    sents, ids = G.corpus_sentences(arr)
    return meta, arr, sents, ids, G.Scorer(ids)


def _vocab(V):
    return {str(i): G.word(i) for i in range(1, V + 1)}


def test_restatement_matches_the_reference_fixture(case):
    meta, arr, _, ids, sc = case
    b, cands = arr["bounds"], G.rows_to_ids(arr["cand"])
    ties = 0
    for i in range(len(b) - 1):
        pairs, sums, order = G.rerank(sc, cands[b[i]:b[i + 1]], ids, arr["nn"][i], meta["k"], meta["m"])
        ref_p = arr["pairs"][b[i]:b[i + 1]]
        assert np.all(ref_p[:, pairs.shape[1]:] == -1.0)                 # the fixture's padding: this image has exactly these captions
        assert G.close(pairs, ref_p[:, :pairs.shape[1]], 1e-12)
        ref_s, ref_o = arr["sums"][b[i]:b[i + 1]], arr["orders"][b[i]:b[i + 1]]
        assert G.close(sums, ref_s, 1e-12)
        assert sorted(order.tolist()) == list(range(len(sums)))
        # same sums position by position; the same candidate wherever the reference's sum at that rank is unique
        np.testing.assert_array_equal(ref_s[order], ref_s[ref_o])
        for r, (a, c) in enumerate(zip(order, ref_o)):
            if np.sum(ref_s == ref_s[c]) == 1:
                assert a == c, (i, r)
            else:
                ties += 1
        # stable rule: equal sums in ascending index
        for x, y in zip(order, order[1:]):
            assert sums[x] > sums[y] or (sums[x] == sums[y] and x < y)
    assert ties >= 5                                                     # the duplicates the fixture plants


def test_spot_values_of_the_reference(case):
    meta, _, _, _, sc = case
    assert sc.pair([], [1, 2, 3]) == 0.0 == meta["spot"]["empty_vs_123"]
    assert sc.pair([1, 2], []) == 0.0 == meta["spot"]["12_vs_empty"]
    assert meta["spot"]["w7_vs_w7"] == pytest.approx(2.5, rel=1e-12) and sc.pair([7], [7]) == pytest.approx(2.5, rel=1e-12)
    # delta is the difference in BIGRAM counts: a one-word and an empty sentence both have length 0
    assert sc.vec([7])[2] == 0 and sc.vec([])[2] == 0 and sc.vec([7, 8, 9])[2] == 2


def test_corpus_tables_match_the_scorer(case):
    meta, arr, sents, ids, sc = case
    c = consensus.ConsensusCorpus(sents, _vocab(meta["V"]), device=None)        # host tables only
    assert c.n_img == meta["n_img"] and c.n_caps == len(arr["corpus_woff"]) - 1 and c.max_words == 64
    assert len(c.ukeys) == len(sc.df) and np.all(c.ukeys[1:] > c.ukeys[:-1])
    assert c.ref_len == np.log(float(meta["n_img"])) and c.n_ids == 260 and c.word_to_ix["w150"] == 150
    for g, d in sc.df.items():
        key = 0
        for j, w in enumerate(g):
            key |= c.word_to_ix[G.word(w)] << (48 - 16 * j)       # corpus-only words got fresh ids
        p = int(np.searchsorted(c.ukeys, np.uint64(key)))
        assert c.ukeys[p] == np.uint64(key) and c.ulogdf[p] == np.log(max(1.0, d))
    np.testing.assert_array_equal(c.gauss[:40], [np.e ** (-(float(d) ** 2) / (2 * 6.0 ** 2)) for d in range(40)])
    # the unigram of word 1 occurs in every image: weight tf * (ref_len - log df) is (to rounding) zero
    p = int(np.searchsorted(c.ukeys, np.uint64(1 << 48)))
    assert abs(c.ref_len - c.ulogdf[p]) < 1e-15 * 8 and arr["df_check"][0] == meta["n_img"] and arr["df_check"][1] == 0


def test_id_map_oov_unk_and_the_16_bit_limit():
    vocab = {"1": "a", "2": "dog", "3": "UNK"}
    refs = [[["a", "dog", "runs"], ["UNK", "runs", "fast"]], [["a", "cat"]]]
    w2i, n = consensus.build_id_map(refs, vocab)
    assert (w2i["a"], w2i["dog"], w2i["UNK"]) == (1, 2, 3)               # a literal UNK in a caption IS the model's UNK
    assert (w2i["runs"], w2i["fast"], w2i["cat"]) == (4, 5, 6) and n == 6    # fresh ids above the vocabulary, first come first
    c = consensus.ConsensusCorpus.__new__(consensus.ConsensusCorpus)
    c.word_to_ix = w2i
    assert c.encode("UNK runs") == [3, 4]
    with pytest.raises(consensus.SubgcError, match="neither"):
        c.encode(["zebra"])
    big = {str(i): f"v{i}" for i in range(1, 65536)}                      # 65535 model ids: full
    assert consensus.build_id_map([[["v5"]]], big)[1] == 65535
    with pytest.raises(consensus.SubgcError, match=r"65536 word ids.*65535"):
        consensus.build_id_map([[["v5", "one_more"]]], big)
    with pytest.raises(consensus.SubgcError, match="one to one"):
        consensus.build_id_map([], {"1": "a", "2": "a"})


def test_ngram_keys_layout():
    keys, sent = consensus.ngram_keys([5, 6, 7, 9], [0, 3, 3, 4])
    want = {(0, 5 << 48), (0, 6 << 48), (0, 7 << 48), (0, (5 << 48) | (6 << 32)), (0, (6 << 48) | (7 << 32)),
            (0, (5 << 48) | (6 << 32) | (7 << 16)), (2, 9 << 48)}
    assert {(int(s), int(k)) for s, k in zip(sent, keys)} == want and len(keys) == len(want)
    k4, _ = consensus.ngram_keys([65535, 1, 2, 3], [0, 4])
    assert int(k4.max()) == (65535 << 48) | (1 << 32) | (2 << 16) | 3


FAKE = 1 << 20                                                           # never dereferenced: the argument checks come first


def _score(L, **over):
    a = dict(T=20, I=2, max_cand=4, top_k=0, nn_ld=60, k=60, n_img=100, n_caps=500, n_gauss=256, m=125, max_caps=300)
    a.update(over)
    return L.subgc_consensus_score(FAKE, FAKE, FAKE, FAKE, FAKE, a["T"], FAKE, a["I"], a["max_cand"], a["top_k"], FAKE, a["nn_ld"], a["k"], FAKE,
                                   a["n_img"], a["n_caps"], FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, a["n_gauss"], a["m"], a["max_caps"], FAKE,
                                   None, 0, None)


@pytest.mark.parametrize("over,what", [(dict(max_caps=2049), b"at most 2048 neighbour captions"), (dict(m=0), b"m >= 1"),
                                       (dict(k=61), b"larger than the neighbour lists"), (dict(k=257, nn_ld=300), b"k <= 256"),
                                       (dict(T=65), b"T <= 64")])
def test_score_entry_point_refuses_on_the_host(over, what):
    L = _lib.lib()
    assert _score(L, **over) == -1
    err = L.subgc_last_error()
    assert b"consensus_score" in err and what in err, err


def test_cook_and_rank_entry_points_refuse_on_the_host():
    L = _lib.lib()
    rc = L.subgc_consensus_cook(FAKE, 0, FAKE, 0, None, None, 0, 10, 257, FAKE, FAKE, 5, 1.0, FAKE, FAKE, FAKE, FAKE, FAKE, None)
    assert rc == -1 and b"at most 256 words" in L.subgc_last_error()
    rc = L.subgc_consensus_cook(FAKE, 1, None, 65, None, None, 0, 10, 0, FAKE, FAKE, 5, 1.0, FAKE, FAKE, FAKE, FAKE, FAKE, None)
    assert rc == -1 and b"T <= 64" in L.subgc_last_error()
    rc = L.subgc_consensus_rank(None, FAKE, 3, 0, FAKE, None, None)
    assert rc == -1 and b"consensus_rank: null pointer" in L.subgc_last_error()
    assert L.subgc_consensus_rank(None, None, 0, 0, None, None, None) == 0          # nothing to do


def test_cpu_tensors_are_refused():
    tok = torch.zeros(4, 20, dtype=torch.int64)
    with pytest.raises(ops.SubgcError, match="device tensors"):
        ops.consensus_cook(tok, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.float64), 1.0)
    with pytest.raises(ops.SubgcError, match="device tensors"):
        ops.consensus_rank(torch.zeros(4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 1, 0, torch.zeros(4, dtype=torch.int32))
    rr = consensus.ConsensusReranker.__new__(consensus.ConsensusReranker)
    with pytest.raises(ops.SubgcError, match="device tensors"):
        rr.rerank(tok, [0, 4], [[0]])


def test_reranker_refuses_bad_k_m_and_neighbourhoods():
    class Host:                                                          # the host tables `neighbours` reads
        n_img = 70
        cap_off = np.arange(71, dtype=np.int64) * 40                     # 40 captions per image
    with pytest.raises(consensus.SubgcError, match="m = 0"):
        consensus.ConsensusReranker(Host, k=60, m=0)
    with pytest.raises(consensus.SubgcError, match="k = 300"):
        consensus.ConsensusReranker(Host, k=300)
    rr = consensus.ConsensusReranker(Host, k=60, m=125)
    with pytest.raises(consensus.SubgcError, match=r"k = 60 is larger than the neighbour list of image 1 \(59 entries\)"):
        rr.neighbours([list(range(60)), list(range(59))])
    with pytest.raises(consensus.SubgcError, match=r"2400 neighbour captions; the limit is 2048"):
        rr.neighbours([list(range(60))])
    nn, mc = consensus.ConsensusReranker(Host, k=50).neighbours([list(range(70))])
    assert nn.shape == (1, 50) and nn.dtype == np.int32 and mc == 2000


def test_rerank_ind_writer_round_trips(tmp_path):
    d = {391895: np.array([2, 0, 1, 3]), "flickr_17": [0], 5: []}
    p = str(tmp_path / "consensus_rerank_ind.npy")
    consensus.save_rerank_ind(p, d)
    back = np.load(p, allow_pickle=True, encoding="latin1").tolist()      # exactly how misc/grd_utils.py:34 reads it
    assert back == {391895: [2, 0, 1, 3], "flickr_17": [0], 5: []}
    assert back[391895][0] == 2 and consensus.load_rerank_ind(p) == back


def test_caption_images_refuses_consensus_in_sct_mode():
    from subgc import eval_glue
    with pytest.raises(ValueError, match="sct"):
        eval_glue.caption_images(torch.nn.Linear(1, 1), [], [], {}, dict(sct=1), consensus={"reranker": None, "nn": {}})
