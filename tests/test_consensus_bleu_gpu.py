"""Consensus re-ranking, method 'bleu', on the device (subgc.consensus.BleuConsensusReranker, csrc/consensus_bleu.hip,
include/subgc_consensus_hip.h): BIT FOR BIT against the Python restatement of the contract (subgc.consensus.bleu_rerank_restatement),
and against the fixture the reference's own calculate_bleu_sentence wrote (tests/golden/make_golden_consensus_bleu.py) within the
derived bounds of DESIGN 4.O (tests/consensus_bleu_golden.py: a pair score (n + 2) u, a sum about (n + 2 + 2 (terms - 1)) u, u = 2^-53)."""
import os

import numpy as np
import pytest
import torch

import consensus_bleu_golden as G
from subgc import consensus, eval_glue, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def case():
    meta, arr = G.load()
    sents, ids = G.corpus_sentences(arr)
    corpus = consensus.ConsensusCorpus(sents, G.vocab(meta["V"]), device=DEV)
    seq = torch.from_numpy(arr["cand"]).to(DEV)
    bounds = [int(x) for x in arr["bounds"]]
    nn = [[int(x) for x in r] for r in arr["nn"]]
    cands = G.rows_to_ids(arr["cand"])
    c = dict(meta=meta, arr=arr, ids=ids, corpus=corpus, seq=seq, bounds=bounds, nn=nn, rr={}, dev={}, want={})
    for name, p in meta["sets"].items():
        rr = c["rr"][name] = consensus.BleuConsensusReranker(corpus, k=meta["k"], m=p["m"], ngram=p["n"], fpr=p["fpr"])
        c["dev"][name] = rr.rerank(seq, bounds, nn, return_pairs=True)
        c["want"][name] = [consensus.bleu_rerank_restatement(cands[a:z], ids, nn[i], meta["k"], p["m"], p["n"], p["fpr"])
                           for i, (a, z) in enumerate(zip(bounds, bounds[1:]))]
    return c


def _same_bits(x, y):
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    return x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", ["A", "B"])
def test_pair_scores_sums_and_orders_match_the_restatement_bit_for_bit(case, name):
    c = case
    order, sim, pairs = c["dev"][name]
    for i, (wp, ws, wo) in enumerate(c["want"][name]):
        nc = int(c["arr"]["n_caps"][i])
        assert wp.shape[1] == nc
        diff = np.argwhere(pairs[i][:, :nc] != wp)
        assert _same_bits(pairs[i][:, :nc], wp), (i, diff[:4].tolist(), [(float(pairs[i][a, b]).hex(), float(wp[a, b]).hex()) for a, b in diff[:4]])
        assert _same_bits(sim[i], ws), (i, [(float(x).hex(), float(y).hex()) for x, y in zip(sim[i], ws)])
        np.testing.assert_array_equal(order[i], wo)


@pytest.mark.parametrize("name", ["A", "B"])
def test_results_match_the_reference_fixture_within_the_derived_bounds(case, name):
    c = case
    p, b, arr = c["meta"]["sets"][name], c["bounds"], c["arr"]
    order, sim, pairs = c["dev"][name]
    worst_p = worst_s = 0.0
    for i in range(len(b) - 1):
        nc = int(arr["n_caps"][i])
        ref_p, ref_s = arr["pairs_" + name][b[i]:b[i + 1], :nc], arr["sums_" + name][b[i]:b[i + 1]]
        ref_o = arr["orders_" + name][b[i]:b[i + 1]]
        worst_p, worst_s = max(worst_p, G.worst_rel(pairs[i][:, :nc], ref_p)), max(worst_s, G.worst_rel(sim[i], ref_s))
        assert G.within(pairs[i][:, :nc], ref_p, G.pair_bound(p["n"])), i
        assert G.within(sim[i], ref_s, G.sim_bound(p["n"], min(p["m"], nc))), i
        # every position of every order: the reference's sums are apart by > 1e-6 relative or belong to identical rows (the generator
        # asserts it), so the device order is the stable order of the reference's sums, and the reference's own np.argsort(-sim)
        # differs from it among identical rows only
        np.testing.assert_array_equal(order[i], np.argsort(-ref_s, kind="stable"))
        for x, y in zip(order[i], ref_o):
            assert x == y or np.array_equal(arr["cand"][b[i] + x], arr["cand"][b[i] + y])
    print(f"set {name}: worst |device - reference| / reference: pairs {worst_p / G.U:.2f} u (bound {G.pair_bound(p['n']) / G.U:.2f} u), "
          f"sums {worst_s / G.U:.2f} u")


@pytest.mark.parametrize("name", ["A", "B"])
def test_edge_cases_one_by_one_on_the_device(case, name):
    c = case
    order, sim, pairs = c["dev"][name]
    G.check_edges(c["meta"], c["arr"], c["ids"], name, pairs, sim, order)


def test_cooked_lists_are_the_sentences_counters(case):
    """subgc_consensus_bleu_cook alone: ascending distinct keys with counts, the key count and the word count, rows and CSR (the corpus holds
    captions of 0, 1, 3, 57, 64 and 200 words: the long-sentence form of the kernel)."""
    c = case
    T = c["seq"].size(1)
    keys, counts, cnt, wlen = [t.cpu().numpy() for t in ops.consensus_bleu_cook(c["seq"])]
    rows = G.rows_to_ids(c["arr"]["cand"])

    def want(ids):
        d = {}
        for o in range(4):
            for p in range(len(ids) - o):
                key = 0
                for j, w in enumerate(ids[p:p + o + 1]):
                    key |= int(w) << (48 - 16 * j)
                d[key] = d.get(key, 0) + 1
        return sorted(d.items())

    for r, ids in enumerate(rows):
        w = want(ids)
        assert wlen[r] == len(ids) and cnt[r] == len(w), r
        assert list(zip(keys[4 * T * r:4 * T * r + cnt[r]].view(np.uint64).tolist(), counts[4 * T * r:4 * T * r + cnt[r]].tolist())) == w, r
    corpus = c["corpus"]
    assert corpus.max_words == 200
    keys, counts, cnt, wlen = [t.cpu().numpy() for t in corpus.bleu_cooked()]
    flat = [cap for caps in c["ids"] for cap in caps]
    assert len(flat) == corpus.n_caps and np.array_equal(wlen[:corpus.n_caps], [len(x) for x in flat])
    probe = sorted(set([0, 1, len(flat) - 1] + [int(corpus.cap_off[img]) + cap for img, cap in ((80, 1), (80, 2), (80, 3), (81, 1), (82, 2), (83, 3))]
                       + list(range(2, len(flat), 97))))
    for s in probe:
        w, base = want(corpus.encode([G.word(x) for x in flat[s]])), 4 * int(corpus.woff[s])
        assert cnt[s] == len(w), s
        assert list(zip(keys[base:base + cnt[s]].view(np.uint64).tolist(), counts[base:base + cnt[s]].tolist())) == w, s
    # a row cap (row_len) shortens the caption
    cap = torch.tensor([2] * c["seq"].size(0), dtype=torch.int32, device=DEV)
    _, _, cnt2, wlen2 = [t.cpu().numpy() for t in ops.consensus_bleu_cook(c["seq"], row_len=cap)]
    assert np.array_equal(wlen2, np.minimum([len(x) for x in rows], 2)) and np.array_equal(cnt2, [len(want(x[:2])) for x in rows])


def test_two_identical_calls_are_bit_identical(case):
    c = case
    for name in ("A", "B"):
        o2, s2, p2 = c["rr"][name].rerank(c["seq"], c["bounds"], c["nn"], return_pairs=True)
        order, sim, pairs = c["dev"][name]
        for i in range(len(c["bounds"]) - 1):
            nc = int(c["arr"]["n_caps"][i])
            assert np.array_equal(o2[i], order[i]) and _same_bits(s2[i], sim[i]) and _same_bits(p2[i][:, :nc], pairs[i][:, :nc])


def test_top_k_keeps_the_first_rows(case):
    c = case
    for name in ("A", "B"):
        o, s = c["rr"][name].rerank(c["seq"], c["bounds"], c["nn"], top_k=4)
        for i, (a, z) in enumerate(zip(c["bounds"], c["bounds"][1:])):
            n = min(4, z - a)
            assert len(o[i]) == n and _same_bits(s[i], c["dev"][name][1][i][:n])
            np.testing.assert_array_equal(o[i], np.argsort(-s[i], kind="stable"))


def test_remove_bad_endings_by_the_string_rule(case):
    """decode_sequence's rule on the device: trailing words of BAD_ENDINGS go, a caption made only of them stays whole."""
    c = case
    V = c["meta"]["V"]
    vocab = G.vocab(V)
    vocab["3"], vocab["4"], vocab["5"] = "the", "of", "a"
    name_of = lambda x: vocab[str(x)] if x <= V else G.word(x)
    corpus = consensus.ConsensusCorpus([[[name_of(x) for x in cap] for cap in caps] for caps in c["ids"]], vocab, device=DEV)
    rr = consensus.BleuConsensusReranker(corpus, k=c["meta"]["k"], m=20, ngram=2, fpr=0.5)
    rows = np.zeros((6, 20), np.int64)
    rows[:] = c["arr"]["cand"][c["bounds"][1]:c["bounds"][1] + 6]
    rows[0, :6] = [10, 11, 3, 12, 4, 5]; rows[0, 6:] = 0                   # two trailing bad words go, the inner one stays
    rows[1, :3] = [3, 4, 5]; rows[1, 3:] = 0                               # nothing but bad words: left whole
    rows[2, :2] = [12, 3]; rows[2, 2:] = 0                                 # one word left: shorter than n = 2, scores 0
    rows[3, :] = 0
    nn = [c["nn"][1]]
    sents = eval_glue.decode_sequence(vocab, rows, 1)
    assert sents[0].split() == ["w10", "w11", "the", "w12"] and sents[1] == "the of a" and sents[2] == "w12" and sents[3] == ""
    assert eval_glue.decode_sequence(vocab, rows, 0) != sents
    ref_ids = [[corpus.encode([name_of(x) for x in cap]) for cap in caps] for caps in c["ids"]]
    sums = []
    for flag in (0, 1):
        o, s = rr.rerank(torch.from_numpy(rows).to(DEV), [0, 6], nn, remove_bad_endings=flag)
        cands = [corpus.encode(t) for t in eval_glue.decode_sequence(vocab, rows, flag)]
        _, want_s, want_o = consensus.bleu_rerank_restatement(cands, ref_ids, nn[0], rr.k, rr.m, rr.ngram, rr.fpr)
        assert _same_bits(s[0], want_s), flag
        np.testing.assert_array_equal(o[0], want_o)
        sums.append(s[0])
    assert sums[0][2] > 0.0 and sums[1][2] == 0.0 and not _same_bits(sums[0][0], sums[1][0])


def test_more_candidates_and_captions_than_a_workgroup_covers():
    """The kernel gives a candidate one workgroup whose 256 threads take a neighbour caption each per pass: an image with 300 candidates
    (drawn from 60 distinct rows, so the restatement stays quick) against 300 neighbour captions (two passes) at the m-RNN defaults
    k = 60, m = 175, n = 4, next to a small image; vocabulary 9488 with corpus-only words above it and captions of 65 - 200 words."""
    rng = np.random.default_rng(7)
    V, n_img = 9488, 400
    vocab = G.vocab(V)

    def zipf(n, hi):
        return [int(x) for x in np.minimum(rng.zipf(1.25, size=n), hi)]

    ids = [[zipf(int(rng.integers(4, 21)), V + 40) for _ in range(5)] for _ in range(n_img)]
    for j, L in ((3, 65), (17, 120), (200, 200)):
        ids[j][2] = zipf(L, V + 40)
    sents = [[[G.word(x) for x in cap] for cap in caps] for caps in ids]
    corpus = consensus.ConsensusCorpus(sents, vocab, device=DEV)
    ref_ids = [[corpus.encode(cap) for cap in caps] for caps in sents]
    rr = consensus.BleuConsensusReranker(corpus)
    assert (rr.k, rr.m, rr.ngram, rr.fpr) == (60, 175, 4, 1.0)
    nn = [[3, 17, 200] + [int(x) for x in rng.choice(np.arange(20, 199), 57, replace=False)],
          [int(x) for x in rng.choice(n_img, 60, replace=False)]]
    distinct = np.zeros((60, 20), np.int64)
    for r in range(60):
        src = ids[nn[0][int(rng.integers(60))]][int(rng.integers(5))]
        s = [x for x in src if x <= V][:int(rng.integers(2, 14))] + zipf(int(rng.integers(0, 8)), V)
        distinct[r, :min(len(s), 20)] = s[:20]
    rows = np.concatenate([distinct[rng.integers(0, 60, size=300)], distinct[:7]])
    bounds = [0, 300, 307]
    o, s, p = rr.rerank(torch.from_numpy(rows).to(DEV), bounds, nn, return_pairs=True)
    cands = G.rows_to_ids(rows)
    for i in range(2):
        want_p, want_s, want_o = consensus.bleu_rerank_restatement(cands[bounds[i]:bounds[i + 1]], ref_ids, nn[i], 60, 175, 4, 1.0)
        assert want_p.shape == (bounds[i + 1] - bounds[i], 300) and np.count_nonzero(want_s) > 0
        assert _same_bits(p[i][:, :300], want_p) and _same_bits(s[i], want_s)
        np.testing.assert_array_equal(o[i], want_o)


def _glue_model(golden):
    import subgc.models as models
    g = golden("subgc_greedy")
    w = golden("subgc_beam").group("weights")
    w["logit.bias"][0] += 2.0
    opt = g.opt(caption_model="topdown", gpn_drop_prob=0.0)
    m = models.setup(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = m.to(DEV).eval()
    D = g.meta["opt"]["att_feat_size"]
    cpu = [synthetic.make_test_batch(M, D=D, seed=400 + i, fc_size=D, node_pool=pool) for i, (M, pool) in enumerate([(24, 14), (5, None), (30, 10)])]
    return m, [{k: v.to(DEV) for k, v in b.items()} for b in cpu], [{"id": 1000 + i} for i in range(len(cpu))]


@pytest.mark.parametrize("return_att,top_k", [(1, 4), (0, None)])
def test_caption_images_with_the_bleu_reranker_end_to_end(golden, return_att, top_k):
    m, images, infos = _glue_model(golden)
    kw = dict(sample_max=1, beam_size=1, return_att=return_att, remove_bad_endings=0)
    vocab = {str(i): f"w{i}" for i in range(1, 60)}
    rng = np.random.default_rng(11)
    words = [vocab[str(i)] for i in range(1, 60)] + ["zz1", "zz2", "UNK"]
    sents = [[[words[min(int(x), len(words)) - 1] for x in rng.zipf(1.4, size=int(rng.integers(0, 16)))] for _ in range(int(rng.integers(2, 6)))]
             for _ in range(80)]
    corpus = consensus.ConsensusCorpus(sents, vocab, device=DEV)
    rr = consensus.make_reranker(corpus, "bleu", k=10, m=20, ngram=2, fpr=0.5)
    nn = {info["id"]: [int(x) for x in rng.choice(80, 12, replace=False)] for info in infos}
    before = eval_glue.caption_images(m, images, infos, vocab, kw)
    after = eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr, "nn": nn, "top_k": top_k})
    ref_ids = [[corpus.encode(cap) for cap in caps] for caps in sents]
    picks, seqs, bounds = [], [], [0]
    for p0, p1 in zip(before, after):
        for key, v in p0.items():                                        # nothing that was there changes, key for key
            if key == "grounding":
                assert p1[key]["subg_index"] == p1["consensus_rerank_ind"][0]        # the grounded sentence is the re-ranker's first choice
                np.testing.assert_array_equal(p1[key]["sort_ind"], v["sort_ind"])
            elif isinstance(v, np.ndarray):
                np.testing.assert_array_equal(p1[key], v)
            else:
                assert p1[key] == v
        assert ("grounding" in p1) == bool(return_att)
        assert set(p1) - set(p0) == {"consensus_rerank_ind", "consensus_sim"}
        caps = p1["caption"] if top_k is None else p1["caption"][:top_k]
        _, want_s, want_o = consensus.bleu_rerank_restatement([corpus.encode(s) for s in caps], ref_ids, nn[p1["image_id"]], 10, 20, 2, 0.5)
        assert _same_bits(p1["consensus_sim"], want_s)
        np.testing.assert_array_equal(p1["consensus_rerank_ind"], want_o)
        assert p1["consensus_rerank_ind"].dtype == np.int64 and p1["consensus_sim"].dtype == np.float64
        picks.append(int(want_o[0]))
        rows = np.zeros((len(caps), 32), np.int64)
        for r, s in enumerate(caps):
            e = corpus.encode(s)
            rows[r, :len(e)] = e
        seqs.append(rows)
        bounds.append(bounds[-1] + len(caps))
    print("re-ranker's first choices:", picks)
    # consensus_rerank_ind equals the stand-alone rerank of the same captions
    o, s = rr.rerank(torch.from_numpy(np.concatenate(seqs)).to(DEV), bounds, [nn[info["id"]] for info in infos])
    for i, p1 in enumerate(after):
        np.testing.assert_array_equal(p1["consensus_rerank_ind"], o[i])
        assert _same_bits(p1["consensus_sim"], s[i])
    if return_att:                                                       # one pass = a second run that is handed the re-ranker's pick
        second = eval_glue.caption_images(m, images, infos, vocab, kw, grd_pick=picks)
        for p1, p2 in zip(after, second):
            assert p1["grounding"]["subg_index"] == p2["grounding"]["subg_index"]
            for key in ("att2_ind", "node_ind", "sort_ind"):
                np.testing.assert_array_equal(p1["grounding"][key], p2["grounding"][key])


@pytest.mark.skipif(os.getenv("SUBGC_POISON_EMPTY") == "1", reason="the poisoned run fills every torch.empty buffer with an ATen fill_ by design")
def test_bleu_rerank_of_a_decode_batch_issues_no_aten_device_kernel(case):
    """The method of tests/test_no_aten_gpu.py: after the one-time corpus build and its lazy cook, a re-rank -- alone or inside
    eval_collect -- is C-ABI launches plus host <-> device copies."""
    from test_no_aten_gpu import Watch
    c = case
    rr = c["rr"]["A"]
    rows, T = c["seq"].shape
    score = torch.linspace(0, 1, rows, device=DEV)
    keep = torch.arange(rows, device=DEV)
    AL = torch.rand(T + 1, rows, 9, device=DEV)
    idx = torch.arange(9, device=DEV).repeat(rows, 1)
    cons = {"reranker": rr, "nn": c["nn"], "top_k": 4, "remove_bad_endings": 1}

    def run():
        return rr.rerank(c["seq"], c["bounds"], c["nn"], top_k=4), ops.eval_collect(score, keep, c["seq"], c["bounds"], AL=AL, idx=idx, consensus=cons)

    run()
    torch.cuda.synchronize()
    with Watch() as w:
        (o, s), h = run()
    torch.cuda.synchronize()
    assert not w.seen, dict(w.seen)
    assert len(o) == len(c["bounds"]) - 1 and h["c_first"].shape == (len(o),)


def test_debug_bounds_reports_a_bad_neighbour_index(case):
    c = case
    rr = c["rr"]["A"]
    bad = [list(r) for r in c["nn"]]
    bad[3][5] = c["meta"]["n_img"]
    neg = [list(r) for r in c["nn"]]
    neg[0][0] = -2
    with ops.debug_bounds():
        rr.rerank(c["seq"], c["bounds"], c["nn"])                         # valid: passes
        with pytest.raises(ops.SubgcError, match=r"consensus_bleu_score: nn \(neighbour image indices\).*outside \[0, 299\].*row 3, column 5: 300"):
            rr.rerank(c["seq"], c["bounds"], bad)
        with pytest.raises(ops.SubgcError, match="neighbour image indices"):
            rr.rerank(c["seq"], c["bounds"], neg)
    o, s = rr.rerank(c["seq"], c["bounds"], bad)                          # mode off: the documented clamp, no error
    torch.cuda.synchronize()
    assert _same_bits(s[0], c["dev"]["A"][1][0])                          # images with valid lists are untouched
    clamped = [list(r) for r in c["nn"]]
    clamped[3][5] = c["meta"]["n_img"] - 1                                # ... and the bad index reads as the last image
    o2, s2 = rr.rerank(c["seq"], c["bounds"], clamped)
    assert _same_bits(s[3], s2[3]) and np.array_equal(o[3], o2[3])


def test_cider_rerank_is_untouched_by_a_bleu_rerank_on_the_same_corpus(case):
    """The lazy cook adds tables to the corpus and changes none: a CIDEr rerank before the first BLEU use of a fresh corpus and after it
    returns identical bits."""
    c = case
    sents, _ = G.corpus_sentences(c["arr"])
    corpus = consensus.ConsensusCorpus(sents, G.vocab(c["meta"]["V"]), device=DEV)
    assert corpus._bleu_cooked is None
    cider = consensus.make_reranker(corpus, "cider", k=c["meta"]["k"], m=125)
    o1, s1, p1 = cider.rerank(c["seq"], c["bounds"], c["nn"], return_pairs=True)
    assert corpus._bleu_cooked is None                                    # the 'cider' method never cooks the BLEU lists
    bleu = consensus.make_reranker(corpus, "bleu", k=c["meta"]["k"])
    ob, sb = bleu.rerank(c["seq"], c["bounds"], c["nn"])
    assert corpus._bleu_cooked is not None and bleu.m == 175
    held = corpus._bleu_cooked
    o2, s2, p2 = cider.rerank(c["seq"], c["bounds"], c["nn"], return_pairs=True)
    bleu.rerank(c["seq"], c["bounds"], c["nn"])
    assert corpus._bleu_cooked is held                                    # cooked once
    for i in range(len(c["bounds"]) - 1):
        nc = int(c["arr"]["n_caps"][i])
        assert np.array_equal(o1[i], o2[i]) and _same_bits(s1[i], s2[i]) and _same_bits(p1[i][:, :nc], p2[i][:, :nc])
        assert _same_bits(sb[i], c["dev"]["A"][1][i]) and np.array_equal(ob[i], c["dev"]["A"][0][i])
