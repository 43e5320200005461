"""Consensus re-ranking on the device (subgc.consensus, csrc/consensus.hip) against the fixture the reference's own CiderScorer wrote
(tests/golden/make_golden_consensus.py) and, for sizes the fixture does not cover, against the numpy restatement of
tests/consensus_golden.py.

The bound on sums and pair scores is 1e-11 relative (1e-300 absolute floor for zeros).  It is derived, not measured: every term is
non-negative (no cancellation), a sum has at most ~250 terms (n * eps ~ 3e-14), a few divisions and square roots are done in fp64, and
log / the Gaussian table come from the host bit for bit -- 1e-11 leaves two to three orders of margin."""
import os

import numpy as np
import pytest
import torch

import consensus_golden as G
from subgc import consensus, eval_glue, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-11


def _vocab(V):
    return {str(i): G.word(i) for i in range(1, V + 1)}


@pytest.fixture(scope="module")
def case():
    meta, arr = G.load()
    sents, ids = G.corpus_sentences(arr)
    corpus = consensus.ConsensusCorpus(sents, _vocab(meta["V"]), device=DEV)
    rr = consensus.ConsensusReranker(corpus, k=meta["k"], m=meta["m"])
    seq = torch.from_numpy(arr["cand"]).to(DEV)
    bounds = [int(x) for x in arr["bounds"]]
    nn = [[int(x) for x in r] for r in arr["nn"]]
    order, sim, pairs = rr.rerank(seq, bounds, nn, return_pairs=True)
    return dict(meta=meta, arr=arr, ids=ids, corpus=corpus, rr=rr, seq=seq, bounds=bounds, nn=nn, order=order, sim=sim, pairs=pairs)


def _ncaps(c, i):
    return int((c["arr"]["pairs"][c["bounds"][i]] != -1.0).sum())


def test_sums_and_pair_scores_match_the_reference(case):
    c = case
    b = c["bounds"]
    worst_s = worst_p = 0.0
    for i in range(len(b) - 1):
        ref_s = c["arr"]["sums"][b[i]:b[i + 1]]
        n = _ncaps(c, i)
        ref_p = c["arr"]["pairs"][b[i]:b[i + 1], :n]
        got_p = c["pairs"][i][:, :n]
        worst_s = max(worst_s, float(np.max(np.abs(c["sim"][i] - ref_s) / np.maximum(np.abs(ref_s), 1e-300))))
        worst_p = max(worst_p, float(np.max(np.abs(got_p - ref_p) / np.maximum(np.abs(ref_p), 1e-300))))
        print(f"image {i}: {len(ref_s)} candidates x {n} captions, worst rel err so far: sums {worst_s:.3e} pairs {worst_p:.3e}")
        assert G.close(c["sim"][i], ref_s, REL), i
        assert G.close(got_p, ref_p, REL), i


def test_orders_complete_check(case):
    c = case
    b = c["bounds"]
    for i in range(len(b) - 1):
        o = c["order"][i]
        ref_s = c["arr"]["sums"][b[i]:b[i + 1]]
        assert sorted(o.tolist()) == list(range(len(ref_s)))
        assert G.close(ref_s[o], np.sort(ref_s)[::-1], REL), i
        rows = c["arr"]["cand"][b[i]:b[i + 1]]
        pos = {int(x): r for r, x in enumerate(o)}
        for x in range(len(rows)):
            for y in range(x + 1, len(rows)):
                if np.array_equal(rows[x], rows[y]):
                    assert pos[x] < pos[y], (i, x, y)             # identical captions: ascending index


def test_two_identical_calls_are_bit_identical(case):
    c = case
    o2, s2, p2 = c["rr"].rerank(c["seq"], c["bounds"], c["nn"], return_pairs=True)
    for i in range(len(c["bounds"]) - 1):
        n = _ncaps(c, i)
        assert np.array_equal(o2[i], c["order"][i])
        assert s2[i].tobytes() == c["sim"][i].tobytes()
        assert p2[i][:, :n].tobytes() == c["pairs"][i][:, :n].tobytes()


def test_edge_cases_one_by_one(case):
    c = case
    e, b, arr = c["meta"]["edges"], c["bounds"], c["arr"]
    m = c["meta"]["m"]

    def ref_pairs(i, cand):
        return arr["pairs"][b[i] + cand, :_ncaps(c, i)]

    i, a = e["empty_candidate"]
    assert not arr["cand"][b[i] + a].any() and c["sim"][i][a] == 0.0 and not c["pairs"][i][a, :_ncaps(c, i)].any()
    # the empty and the one-word neighbour caption sit in the first neighbour image of image 0: columns 1 and 2
    i, img, cap = e["empty_neighbour_caption"]
    assert c["nn"][i][0] == img and len(c["ids"][img][cap]) == 0
    assert not c["pairs"][i][:, cap].any() and not ref_pairs(i, 1)[cap].any()
    i, a = e["one_word_candidate"]
    _, img, cap = e["one_word_neighbour_caption"]
    assert c["ids"][img][cap] == [7] and list(arr["cand"][b[i] + a][:2]) == [7, 0]
    assert abs(c["pairs"][i][a, cap] - 2.5) <= REL * 2.5                # ('w7', 'w7'): one order of four matches exactly
    assert G.close(c["pairs"][i][a, :_ncaps(c, i)], ref_pairs(i, a), REL) and c["sim"][i][a] > 0
    i, x, y = e["duplicate_candidates"]
    assert np.array_equal(arr["cand"][b[i] + x], arr["cand"][b[i] + y])
    assert c["sim"][i][x].tobytes() == c["sim"][i][y].tobytes()
    o = c["order"][i].tolist()
    assert o.index(x) + 1 == o.index(y)                                   # adjacent, lower index first
    i, a = e["unseen_ngrams_candidate"]
    assert G.close(c["pairs"][i][a, :_ncaps(c, i)], ref_pairs(i, a), REL) and G.close(c["sim"][i][a], arr["sums"][b[i] + a], REL)
    # an n-gram the corpus never saw has df 0 -> weight tf * ref_len; the unigram every image holds has weight (to rounding) zero
    keys, wts, cnt, blen, norm = [t.cpu().numpy() for t in ops.consensus_cook(c["seq"], c["corpus"].d_ukeys, c["corpus"].d_ulogdf, c["corpus"].ref_len)]
    T = c["seq"].size(1)
    row = b[i] + a
    kk, ww = keys[4 * T * row:4 * T * row + cnt[row]].view(np.uint64), wts[4 * T * row:4 * T * row + cnt[row]]
    assert np.all(kk[1:] > kk[:-1])                                       # ascending, every key once
    assert ww[list(kk).index(np.uint64(150 << 48))] == 1.0 * c["corpus"].ref_len
    i, a = e["weight_zero_unigram_candidate"]
    row = b[i] + a
    kk, ww = keys[4 * T * row:4 * T * row + cnt[row]].view(np.uint64), wts[4 * T * row:4 * T * row + cnt[row]]
    assert abs(ww[list(kk).index(np.uint64(1 << 48))]) < 1e-14 and blen[row] == int((arr["cand"][row] > 0).sum()) - 1
    assert G.close(c["sim"][i][a], arr["sums"][row], REL)
    assert blen[b[0]] == 0 and blen[b[0] + 1] == 0 and cnt[b[0]] == 0 and cnt[b[0] + 1] == 1     # empty and one-word: length 0 both
    i = e["fewer_than_m_image"]
    n = _ncaps(c, i)
    assert n < m and G.close(c["sim"][i], arr["sums"][b[i]:b[i + 1]], REL)
    assert G.close(c["sim"][i][0], float(np.sum(np.sort(c["pairs"][i][0, :n])[::-1])), 1e-13)   # ALL pair scores are summed
    assert _ncaps(c, 0) > m                                               # and elsewhere only the m largest
    # corpus captions of 50+ words are neighbours of image 0
    col = 0
    seen = 0
    for img in c["nn"][0][:c["meta"]["k"]]:
        for cap in range(len(c["ids"][img])):
            if [img, cap] in e["long_captions"]:
                assert len(c["ids"][img][cap]) >= 50
                assert G.close(c["pairs"][0][:, col], arr["pairs"][b[0]:b[1], col], REL) and c["pairs"][0][:, col].any()
                seen += 1
            col += 1
    assert seen == 2


def test_top_k_keeps_the_first_rows(case):
    c = case
    o, s = c["rr"].rerank(c["seq"], c["bounds"], c["nn"], top_k=4)
    for i, (a, z) in enumerate(zip(c["bounds"], c["bounds"][1:])):
        n = min(4, z - a)
        assert len(o[i]) == n and s[i].tobytes() == c["sim"][i][:n].tobytes()
        np.testing.assert_array_equal(o[i], np.argsort(-s[i], kind="stable"))


def test_remove_bad_endings_by_the_string_rule(case):
    """decode_sequence's rule on the device: trailing words of BAD_ENDINGS go, a caption made only of them stays whole."""
    c = case
    vocab = _vocab(c["meta"]["V"])
    vocab["3"], vocab["4"], vocab["5"] = "the", "of", "a"
    corpus = consensus.ConsensusCorpus([[[vocab[str(x)] if x <= c["meta"]["V"] else G.word(x) for x in cap] for cap in caps] for caps in c["ids"]],
                                       vocab, device=DEV)
    rr = consensus.ConsensusReranker(corpus, k=c["meta"]["k"], m=c["meta"]["m"])
    rows = np.zeros((6, 20), np.int64)
    src = c["arr"]["cand"][c["bounds"][1]:c["bounds"][1] + 6]
    rows[:] = src
    rows[0, :6] = [10, 11, 3, 12, 4, 5]; rows[0, 6:] = 0                   # two trailing bad words go, the inner one stays
    rows[1, :3] = [3, 4, 5]; rows[1, 3:] = 0                               # nothing but bad words: left whole
    rows[2, :2] = [12, 3]; rows[2, 2:] = 0
    rows[3, :] = 0
    nn = [c["nn"][1]]
    sents = eval_glue.decode_sequence(vocab, rows, 1)
    assert sents[0].split() == ["w10", "w11", "the", "w12"] and sents[1] == "the of a" and sents[2] == "w12" and sents[3] == ""
    assert eval_glue.decode_sequence(vocab, rows, 0) != sents
    ref_ids = [[corpus.encode([vocab[str(x)] if x <= c["meta"]["V"] else G.word(x) for x in cap]) for cap in caps] for caps in c["ids"]]
    sc = G.Scorer(ref_ids)
    for flag in (0, 1):
        o, s = rr.rerank(torch.from_numpy(rows).to(DEV), [0, 6], nn, remove_bad_endings=flag)
        cands = [corpus.encode(t) for t in eval_glue.decode_sequence(vocab, rows, flag)]
        _, want_s, want_o = G.rerank(sc, cands, ref_ids, nn[0], rr.k, rr.m)
        assert G.close(s[0], want_s, REL), flag
        np.testing.assert_array_equal(o[0], want_o)


def test_mrnn_like_shape_against_the_restatement():
    """Vocabulary 9488, k = 60, m = 125, ~300 neighbour captions, 100 candidates, 2 images; some corpus captions of 65 - 200 words
    (the long-caption form of the cook kernel)."""
    rng = np.random.default_rng(7)
    V, n_img = 9488, 400
    vocab = _vocab(V)

    def zipf(n, hi):
        return [int(x) for x in np.minimum(rng.zipf(1.25, size=n), hi)]

    ids = [[zipf(int(rng.integers(4, 21)), V + 40) for _ in range(5)] for _ in range(n_img)]
    for j, L in ((3, 65), (17, 120), (200, 200)):
        ids[j][2] = zipf(L, V + 40)
    sents = [[[G.word(x) for x in cap] for cap in caps] for caps in ids]
    corpus = consensus.ConsensusCorpus(sents, vocab, device=DEV)
    assert corpus.max_words == 200
    ref_ids = [[corpus.encode(cap) for cap in caps] for caps in sents]
    rr = consensus.ConsensusReranker(corpus, k=60, m=125)
    nn = [[3, 17, 200] + [int(x) for x in rng.choice(np.arange(20, 199), 57, replace=False)],
          [int(x) for x in rng.choice(n_img, 60, replace=False)]]
    rows = np.zeros((200, 20), np.int64)
    for r in range(200):
        i = r // 100
        src = ids[nn[i][int(rng.integers(60))]][int(rng.integers(5))]
        s = [x for x in src if x <= V][:int(rng.integers(2, 14))] + zipf(int(rng.integers(0, 8)), V)
        rows[r, :min(len(s), 20)] = s[:20]
    rows[150] = rows[120]
    o, s, p = rr.rerank(torch.from_numpy(rows).to(DEV), [0, 100, 200], nn, return_pairs=True)
    sc = G.Scorer(ref_ids)
    cands = G.rows_to_ids(rows)
    for i in range(2):
        want_p, want_s, want_o = G.rerank(sc, cands[100 * i:100 * i + 100], ref_ids, nn[i], 60, 125)
        assert want_p.shape == (100, 300)
        print(f"image {i}: worst rel err sums {np.max(np.abs(s[i] - want_s) / np.maximum(want_s, 1e-300)):.3e}")
        assert G.close(p[i][:, :300], want_p, REL) and G.close(s[i], want_s, REL)
        assert G.close(want_s[o[i]], np.sort(want_s)[::-1], REL)
        if i == 1:
            assert list(o[i]).index(20) < list(o[i]).index(50)


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


@pytest.mark.parametrize("rbe,top_k", [(0, 4), (1, None)])
def test_caption_images_with_consensus_end_to_end(golden, rbe, top_k):
    m, images, infos = _glue_model(golden)
    kw = dict(sample_max=1, beam_size=1, return_att=1, remove_bad_endings=0)
    vocab = {str(i): f"w{i}" for i in range(1, 60)}
    # give the words the captions end with most often the names of dangling function words, so that remove_bad_endings bites
    plain = eval_glue.caption_images(m, images, infos, vocab, kw)
    last = [s.split()[-1] for p in plain for s in p["caption"] if s]
    common = [w for w, _ in sorted({w: last.count(w) for w in set(last)}.items(), key=lambda t: (-t[1], t[0]))][:3]
    for w, name in zip(common, ("the", "of", "a")):
        vocab[w[1:]] = name
    kw["remove_bad_endings"] = rbe
    rng = np.random.default_rng(11)
    words = [vocab[str(i)] for i in range(1, 60)] + ["zz1", "zz2", "UNK"]
    sents = [[[words[min(int(x), len(words)) - 1] for x in rng.zipf(1.4, size=int(rng.integers(0, 16)))] for _ in range(int(rng.integers(2, 6)))]
             for _ in range(80)]
    corpus = consensus.ConsensusCorpus(sents, vocab, device=DEV)
    rr = consensus.ConsensusReranker(corpus, k=10, m=20)
    nn = {info["id"]: [int(x) for x in rng.choice(80, 12, replace=False)] for info in infos}
    before = eval_glue.caption_images(m, images, infos, vocab, kw)
    after = eval_glue.caption_images(m, images, infos, vocab, kw, consensus={"reranker": rr, "nn": nn, "top_k": top_k})
    if rbe:                                                              # some caption did lose its dangling words
        assert any(len(a.split()) < len(b.split()) for p0, p in zip(before, plain) for a, b in zip(p0["caption"], p["caption"]))
    ref_ids = [[corpus.encode(cap) for cap in caps] for caps in sents]
    sc = G.Scorer(ref_ids)
    picks = []
    for p0, p1 in zip(before, after):
        for key, v in p0.items():                                        # nothing that was there changes, key for key
            if key == "grounding":
                assert p1[key]["subg_index"] == p1["consensus_rerank_ind"][0]
                np.testing.assert_array_equal(p1[key]["sort_ind"], v["sort_ind"])
            elif isinstance(v, np.ndarray):
                np.testing.assert_array_equal(p1[key], v)
            else:
                assert p1[key] == v
        assert set(p1) - set(p0) == {"consensus_rerank_ind", "consensus_sim"}
        caps = p1["caption"] if top_k is None else p1["caption"][:top_k]
        _, want_s, want_o = G.rerank(sc, [corpus.encode(s) for s in caps], ref_ids, nn[p1["image_id"]], 10, 20)
        assert G.close(p1["consensus_sim"], want_s, REL)
        np.testing.assert_array_equal(p1["consensus_rerank_ind"], want_o)
        assert p1["consensus_rerank_ind"].dtype == np.int64 and p1["consensus_sim"].dtype == np.float64
        picks.append(int(want_o[0]))
    print("re-ranker's first choices:", picks)
    # one pass = the reference's two passes: the same grounding as a second run that is handed the re-ranker's pick
    second = eval_glue.caption_images(m, images, infos, vocab, kw, grd_pick=picks)
    for p1, p2 in zip(after, second):
        assert p1["grounding"]["subg_index"] == p2["grounding"]["subg_index"]
        for key in ("att2_ind", "node_ind", "sort_ind"):
            np.testing.assert_array_equal(p1["grounding"][key], p2["grounding"][key])
    # an explicit grd_pick still wins
    forced = eval_glue.caption_images(m, images, infos, vocab, kw, grd_pick=[0] * len(images), consensus={"reranker": rr, "nn": nn, "top_k": top_k})
    for p0, pf, p1 in zip(before, forced, after):
        assert pf["grounding"]["subg_index"] == 0
        np.testing.assert_array_equal(pf["grounding"]["node_ind"], p0["grounding"]["node_ind"])
        np.testing.assert_array_equal(pf["consensus_rerank_ind"], p1["consensus_rerank_ind"])
    with pytest.raises(ValueError, match="sct"):
        eval_glue.caption_images(m, images, infos, vocab, dict(kw, sct=1), consensus={"reranker": rr, "nn": nn})


@pytest.mark.skipif(os.getenv("SUBGC_POISON_EMPTY") == "1", reason="the poisoned run fills every torch.empty buffer with an ATen fill_ by design")
def test_rerank_of_a_decode_batch_issues_no_aten_device_kernel(case):
    """The method of tests/test_no_aten_gpu.py: after the one-time corpus build, a re-rank -- alone or inside eval_collect -- is C-ABI
    launches plus host <-> device copies."""
    from test_no_aten_gpu import Watch
    c = case
    rows, T = c["seq"].shape
    score = torch.linspace(0, 1, rows, device=DEV)
    keep = torch.arange(rows, device=DEV)
    AL = torch.rand(T + 1, rows, 9, device=DEV)
    idx = torch.arange(9, device=DEV).repeat(rows, 1)
    cons = {"reranker": c["rr"], "nn": c["nn"], "top_k": 4, "remove_bad_endings": 1}

    def run():
        return c["rr"].rerank(c["seq"], c["bounds"], c["nn"], top_k=4), ops.eval_collect(score, keep, c["seq"], c["bounds"], AL=AL, idx=idx, consensus=cons)

    run()
    torch.cuda.synchronize()
    with Watch() as w:
        (o, s), h = run()
    torch.cuda.synchronize()
    assert not w.seen, dict(w.seen)
    assert len(o) == len(c["bounds"]) - 1 and h["c_first"].shape == (len(o),)


def test_debug_bounds_reports_a_bad_neighbour_index(case):
    c = case
    bad = [list(r) for r in c["nn"]]
    bad[3][5] = c["meta"]["n_img"]
    neg = [list(r) for r in c["nn"]]
    neg[0][0] = -2
    with ops.debug_bounds():
        c["rr"].rerank(c["seq"], c["bounds"], c["nn"])                    # valid: passes
        with pytest.raises(ops.SubgcError, match=r"consensus_score: nn \(neighbour image indices\).*outside \[0, 299\].*row 3, column 5: 300"):
            c["rr"].rerank(c["seq"], c["bounds"], bad)
        with pytest.raises(ops.SubgcError, match="neighbour image indices"):
            c["rr"].rerank(c["seq"], c["bounds"], neg)
    o, s = c["rr"].rerank(c["seq"], c["bounds"], bad)                     # mode off: the documented clamp, no error, no fault
    torch.cuda.synchronize()
    assert s[0].tobytes() == c["sim"][0].tobytes()                        # images with valid lists are untouched
