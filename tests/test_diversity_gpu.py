"""Diversity scores on the device (subgc.diversity, csrc/diversity.hip) against the fixture the reference's own diversity_score.py
wrote (tests/golden/make_golden_diversity.py) and, for sizes the fixture does not cover, against the set-and-dict restatement of
tests/diversity_golden.py.

Counts and the ratios formed from them are compared with ==: they are integers, divided on the host by the script's own expressions.
mBLEU-4 and the sentence BLEU-4 values get 1e-12 relative.  Derived, not measured: a value is 4 divisions, 3 products, one pow and one
exp in fp64; the brevity exponent 1 - 1/ratio has a condition number of at most the length ratio (<= 64); together on the order of
100 ulp ~ 2e-14, and the bound leaves roughly 50x that.  The first test prints the worst relative error it meets on the fixture."""
import os

import numpy as np
import pytest
import torch

import diversity_golden as G
from subgc import diversity, eval_glue, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 1e-12
INT_KEYS = ("drawn", "distinct", "words", "unigrams", "bigrams", "novel", "novel_of")


@pytest.fixture(scope="module")
def case():
    meta, arr = G.load()
    voc = G.vocab(meta["V"])
    ix = diversity.NoveltyIndex(meta["train"], voc, device=DEV)
    scorer = diversity.DiversityScorer(ix, meta["n_best"])
    seq = torch.from_numpy(arr["seq"].astype(np.int64)).to(DEV)
    score = torch.from_numpy(arr["score"]).to(DEV)
    bounds = [int(x) for x in arr["bounds"]]
    draws = {run: G.fixture_draws(meta, arr, run) for run in ("mb4", "plain")}
    got = {run: scorer.score(seq, bounds, score, draws[run]) for run in ("mb4", "plain")}
    return dict(meta=meta, arr=arr, voc=voc, ix=ix, scorer=scorer, seq=seq, score=score, bounds=bounds, draws=draws, got=got)


def _check_printed(got, want, with_mb4):
    if with_mb4:
        print("printed mBLEU-4:", got[:2], "reference:", want[:2], "worst rel err", G.worst_rel(got[:2], want[:2]))
        assert G.close(got[:2], want[:2], REL)
    assert got[-8:] == want[-8:]                                          # integer counts divided on the host: equal bits


def test_fixture_counts_bleu_and_printed_numbers_match_the_reference(case):
    c = case
    meta, arr = c["meta"], c["arr"]
    for run in ("mb4", "plain"):
        want = G.fixture_per_image(meta, arr, run)
        for i, (g, w) in enumerate(zip(c["got"][run], want)):
            for key in INT_KEYS:
                np.testing.assert_array_equal(g[key], w[key], err_msg=f"{run} image {i} {key}")
                assert g[key].dtype == np.int64
            assert ("mbleu4" in g) == (run == "mb4")
        _check_printed(diversity.summarize(c["got"][run])["printed"], meta["runs"][run]["printed"], run == "mb4")
    worst = 0.0
    for i, g in enumerate(c["got"]["mb4"]):
        ref = arr["bleu4"][i]
        np.testing.assert_array_equal(g["selected"], arr["selected"][i])
        np.testing.assert_array_equal(np.isnan(g["bleu4"]), np.isnan(ref))
        ok = ~np.isnan(ref)
        worst = max(worst, G.worst_rel(g["bleu4"][ok], ref[ok]))
        assert G.close(g["bleu4"][ok], ref[ok], REL), i
        assert g["mbleu4_valid"].all()
        assert G.close(g["mbleu4"], [np.mean(np.array(row[~np.isnan(row)])) for row in ref], REL)
    print(f"sentence BLEU-4: worst relative error against the reference {worst:.3e}")
    s = diversity.summarize(c["got"]["mb4"])
    assert s["mbleu4_left_out"] == [0, 0] and s["novel"] == [int(x) for x in meta["runs"]["mb4"]["printed"][6:8]]


def test_fixture_planted_cases_one_by_one(case):
    c = case
    e, got, arr = c["meta"]["edges"], c["got"]["mb4"], c["arr"]
    i, cap = e["empty_caption_selected"]
    q = got[i]["selected"][0].tolist().index(cap)
    assert got[i]["bleu4"][0, q] == 0.0 == arr["bleu4"][i, 0, q]           # no words: exp(1 - 1/ratio) underflows to 0 on both sides
    assert got[i]["words"][0] == 1 + 1 + c["meta"]["T"] + 3 + 5           # the empty caption counts as ONE word
    assert got[i]["novel"][0] == 2                                        # '' ('.'), 'w3 w1 w2' and its 5-word form are training captions
    i, cap = e["shorter_than_every_reference"]
    q = got[i]["selected"][0].tolist().index(cap)
    assert 0 < got[i]["bleu4"][0, q] < 1 and G.close(got[i]["bleu4"][0, q], arr["bleu4"][i, 0, q], REL)
    i, x, y = e["duplicates_in_a_draw"]
    assert got[i]["drawn"][0] == 7 and got[i]["distinct"][0] == 6
    i, cap = e["equals_double_space_train_caption_if_split_wrongly"]
    assert got[i]["novel"].tolist() == [2, 2] and got[i]["novel_of"].tolist() == [2, 2]     # 'w4 w5 w6' is only a validation caption


@pytest.mark.parametrize("run", ["mb4", "plain"])
def test_score_predictions_is_the_drop_in_for_the_script(case, run):
    c = case
    meta, arr, b = c["meta"], c["arr"], c["bounds"]
    sents = eval_glue.decode_sequence(c["voc"], arr["seq"].astype(np.int64), 0)
    preds = [{"image_id": 5000 + i, "caption": sents[b[i]:b[i + 1]], "subgraph_score": arr["score"][b[i]:b[i + 1]]} for i in range(len(b) - 1)]
    s, per = diversity.score_predictions(preds, c["voc"], novelty=c["ix"], evaluate_mB4=run == "mb4")
    _check_printed(s["printed"], meta["runs"][run]["printed"], run == "mb4")
    for g, w in zip(per, c["got"][run]):
        assert sorted(g) == sorted(w)
        for key in g:
            assert np.asarray(g[key]).tobytes() == np.asarray(w[key]).tobytes(), key
    with pytest.raises(diversity.SubgcError, match="not in the vocabulary"):
        diversity.score_predictions([{"image_id": 1, "caption": ["w1 zebra"], "subgraph_score": np.zeros(1, np.float32)}], c["voc"])


def _compare(g, t, r, metric, n_best):
    if metric == 1:
        assert (g["drawn"][t], g["distinct"][t]) == (r["drawn"], r["distinct"])
    elif metric == 3:
        assert (g["words"][t], g["unigrams"][t], g["bigrams"][t]) == (r["words"], r["unigrams"], r["bigrams"])
    elif metric == 2:
        assert (g["novel"][t], g["novel_of"][t]) == (r["novel"], len(r["selected"]))
    else:
        n = len(r["selected"])
        assert g["selected"][t, :n].tolist() == r["selected"] and (g["selected"][t, n:] == -1).all()
        assert bool(g["mbleu4_valid"][t]) == (n >= 2)
        if n >= 2:
            assert G.close(g["bleu4"][t, :n], r["bleu4"], REL) and np.isnan(g["bleu4"][t, n:]).all()
            assert G.close(g["mbleu4"][t], r["mbleu4"], REL)
        else:
            assert np.isnan(g["bleu4"][t]).all() and np.isnan(g["mbleu4"][t])


def _random_batch(rng, sizes, T, n_ids, levels):
    rows = np.zeros((sum(sizes), T), np.int32)
    for r in range(len(rows)):
        L = int(rng.integers(0, T + 1))
        rows[r, :L] = rng.integers(1, n_ids + 1, size=L)
    score = (rng.integers(0, levels, size=len(rows)) / np.float32(levels)).astype(np.float32)     # few levels: equal scores are routine
    return rows, score, [0] + [int(x) for x in np.cumsum(sizes)]


def test_random_sets_against_the_restatement():
    """360 sets: 30 images of 1 .. 130 rows, T = 6, five word ids (captions repeat, n-grams overlap, scores tie), three draws of any
    size per image and metric; int32 token rows, as eval_collect hands them over."""
    rng = np.random.default_rng(5)
    sizes = [1, 2, 4, 5, 6, 63, 64, 65, 127, 128, 129, 130] + [int(x) for x in rng.integers(1, 131, size=18)]
    rows, score, bounds = _random_batch(rng, sizes, 6, 5, 40)
    voc = G.vocab(5)
    train = [" ".join(G.word(x) for x in rng.integers(1, 6, size=int(rng.integers(0, 5)))) for _ in range(150)]
    ix = diversity.NoveltyIndex(train, voc, device=DEV)
    scorer = diversity.DiversityScorer(ix, 5)
    draws = {m: [[rng.choice(n, int(rng.integers(1, n + 1)), replace=False) for _ in range(3)] for n in sizes] for m in (1, 2, 3, 4)}
    got = scorer.score(torch.from_numpy(rows).to(DEV), bounds, torch.from_numpy(score).to(DEV), draws)
    caps = G.rows_to_ids(rows)
    checked = novel = tied = 0
    for i, n in enumerate(sizes):
        mine, sc = caps[bounds[i]:bounds[i + 1]], score[bounds[i]:bounds[i + 1]]
        for m in (1, 2, 3, 4):
            for t in range(3):
                r = G.restate(mine, sc, draws[m][i][t], 5, ix.captions)
                _compare(got[i], t, r, m, 5)
                checked += 1
                novel += (r["novel"] or 0) if m == 2 else 0
                tied += m == 4 and len(set(sc[r["selected"]].tolist())) < len(r["selected"])
    assert checked == 360 and novel > 0 and tied > 10
    assert sum(int(g["novel_of"].sum() - g["novel"].sum()) for g in got) > 0          # and some selected captions are training captions


def test_tie_rule_later_in_the_draw_first():
    score = np.asarray([0.5, 0.5, 0.5, 0.5, 0.2, 0.5, 0.9, 0.5, -0.0, 0.0], np.float32)
    rows = np.zeros((10, 4), np.int64)
    rows[:, 0] = np.arange(1, 11)
    draws = {4: [[np.asarray([3, 0, 7, 1, 6, 5, 2]), np.asarray([4, 1]), np.asarray([8, 9]), np.asarray([9, 8])]]}
    g = diversity.DiversityScorer(None, 5).score(torch.from_numpy(rows).to(DEV), [0, 10], torch.from_numpy(score).to(DEV), draws)[0]
    assert g["selected"][0].tolist() == [6, 2, 5, 1, 7]                   # 0.9, then the 0.5 rows from the END of the draw backwards
    assert g["selected"][1].tolist() == [1, 4, -1, -1, -1]
    assert g["selected"][2].tolist() == [9, 8, -1, -1, -1] and g["selected"][3].tolist() == [8, 9, -1, -1, -1]     # -0 == +0: a tie
    for t, d in enumerate(draws[4][0]):
        assert g["selected"][t, :min(5, len(d))].tolist() == G.restate(G.rows_to_ids(rows), score, d, 5)["selected"]


def test_short_selections_return_flags_and_do_not_fault():
    rows = np.asarray([[1, 2, 0], [3, 0, 0], [1, 2, 0], [3, 0, 0]], np.int64)
    score = torch.tensor([0.3, 0.1, 0.2, 0.4], device=DEV)
    bounds = [0, 1, 1, 4]                                                 # a one-row image, an image without rows, a three-row image
    sizes = [1, 0, 3]
    draws = diversity.per_image_draws(sizes, [7, 8, 9], (20, 100), 2019)
    scorer = diversity.DiversityScorer(None, 5)
    got = scorer.score(torch.from_numpy(rows).to(DEV), bounds, score, draws)
    torch.cuda.synchronize()
    one, none, three = got
    assert one["drawn"].tolist() == [1, 1] and one["distinct"].tolist() == [1, 1] and one["words"].tolist() == [2, 2]
    assert not one["mbleu4_valid"].any() and np.isnan(one["mbleu4"]).all() and one["selected"][0].tolist() == [0, -1, -1, -1, -1]
    assert none["drawn"].tolist() == [0, 0] and none["words"].tolist() == [0, 0] and not none["mbleu4_valid"].any()
    assert three["mbleu4_valid"].all() and three["drawn"].tolist() == [3, 3] and three["distinct"].tolist() == [2, 2]
    assert "novel" not in one                                             # no index: no Novel Caption count
    s = diversity.summarize(got)
    assert s["mbleu4_left_out"] == [2, 2] and s["mbleu4"][0] == three["mbleu4"][0]
    # an empty batch, and a batch whose only image has no rows
    empty = torch.zeros(0, 3, dtype=torch.int64, device=DEV)
    assert scorer.score(empty, [0], score[:0], {m: [] for m in (1, 2, 3, 4)}) == []
    lone = scorer.score(empty, [0, 0], score[:0], diversity.per_image_draws([0], [1], (20, 100), 2019))
    torch.cuda.synchronize()
    assert len(lone) == 1 and lone[0]["drawn"].tolist() == [0, 0] and not lone[0]["mbleu4_valid"].any()
    with pytest.raises(diversity.SubgcError, match="limit is 1024"):
        scorer.score(torch.from_numpy(rows).to(DEV), [0, 4], score, {1: [[np.zeros(1025, np.int64)]]})
    with pytest.raises(diversity.SubgcError, match="limit is 64"):
        scorer.score(torch.zeros(2, 65, dtype=torch.int64, device=DEV), [0, 2], score[:2], {1: [[np.zeros(1, np.int64)]]})
    with pytest.raises(diversity.SubgcError, match="2 <= n_best <= 16"):
        diversity.DiversityScorer(None, 17)


@pytest.mark.parametrize("n_best", [5, 16])
def test_whole_1000_row_image_against_the_restatement(n_best):
    """The MRNN case at its largest: one image of 1000 rows drawn whole (the counting rank, the hash table and the distinct scan at full
    length), T = 20; n_best = 16 also fills the selection buffers and takes np.mean's eight-lane order."""
    rng = np.random.default_rng(11)
    T, n = 20, 1000
    pool = [rng.integers(1, 31, size=int(rng.integers(8, T + 1))) for _ in range(12)]
    rows = np.zeros((n, T), np.int64)
    for r in range(n):
        t = pool[int(rng.integers(len(pool)))]
        a = int(rng.integers(0, 3))
        c = t[a:a + int(rng.integers(1, len(t) + 1))].copy()
        if rng.random() < 0.4:
            c[int(rng.integers(len(c)))] = int(rng.integers(1, 31))
        rows[r, :len(c)] = c
    rows[17] = rows[3]
    rows[999] = pool[0].tolist() + [0] * (T - len(pool[0]))
    score = rng.random(n).astype(np.float32)
    score[[5, 900, 17]] = score.max()                                     # a three-way tie at the top
    caps = G.rows_to_ids(rows)
    voc = G.vocab(30)
    ix = diversity.NoveltyIndex([" ".join(G.word(x) for x in c) for c in caps[::7]], voc, device=DEV)
    draws = {m: [[rng.permutation(n), rng.choice(n, 100, replace=False)]] for m in (1, 2, 3, 4)}
    got = diversity.DiversityScorer(ix, n_best).score(torch.from_numpy(rows).to(DEV), [0, n], torch.from_numpy(score).to(DEV), draws)[0]
    for m in (1, 2, 3, 4):
        for t in range(2):
            _compare(got, t, G.restate(caps, score, draws[m][0][t], n_best, ix.captions), m, n_best)
    assert got["distinct"][0] < 1000 and got["drawn"][0] == 1000
    print(f"n_best {n_best}: mBLEU-4 {got['mbleu4']}, worst rel err vs np.mean of the device's own sentence values "
          f"{G.worst_rel(got['mbleu4'], [np.mean(got['bleu4'][t]) for t in range(2)]):.3e}")
    assert G.close(got["mbleu4"], [float(np.mean(got["bleu4"][t])) for t in range(2)], REL)


def test_remove_bad_endings_follows_the_string_rule():
    voc = G.vocab(12)
    voc["3"], voc["4"], voc["5"] = "the", "of", "a"
    rows = np.asarray([[10, 11, 3, 12, 4, 5], [3, 4, 5, 0, 0, 0], [12, 3, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [10, 11, 3, 12, 0, 0], [12, 0, 0, 0, 0, 0],
                       [10, 11, 3, 12, 4, 0]], np.int64)
    score = torch.linspace(1, 0, 7, device=DEV)
    sents = eval_glue.decode_sequence(voc, rows, 1)
    assert sents[0] == "w10 w11 the w12" and sents[1] == "the of a" and sents[2] == "w12" and sents[3] == ""
    ix = diversity.NoveltyIndex(["w12", "w10 w11 the w12 of a"], voc, device=DEV)
    scorer = diversity.DiversityScorer(ix, 5)
    draws = {m: [[np.arange(7), np.asarray([6, 0, 4])]] for m in (1, 2, 3, 4)}
    bad = {3, 4, 5}
    w2i = ix.word_to_ix
    for flag in (0, 1):
        got = scorer.score(torch.from_numpy(rows).to(DEV), [0, 7], score, draws, remove_bad_endings=flag)[0]
        caps = G.rows_to_ids(rows, bad if flag else None)
        assert caps == [[w2i[w] for w in s.split(" ")] if s else [] for s in eval_glue.decode_sequence(voc, rows, flag)]
        for m in (1, 2, 3, 4):
            for t in range(2):
                _compare(got, t, G.restate(caps, score.cpu().numpy(), draws[m][0][t], 5, ix.captions), m, 5)
        assert got["distinct"].tolist() == ([7, 3] if not flag else [4, 1])      # rows 0, 4, 6 and rows 2, 5 become one caption each
    with pytest.raises(diversity.SubgcError, match="needs the vocabulary"):
        diversity.DiversityScorer(None, 5).score(torch.from_numpy(rows).to(DEV), [0, 7], score, draws, remove_bad_endings=1)


def test_two_identical_calls_are_bit_identical(case):
    c = case
    again = c["scorer"].score(c["seq"], c["bounds"], c["score"], c["draws"]["mb4"])
    for g, w in zip(again, c["got"]["mb4"]):
        assert sorted(g) == sorted(w)
        for key in g:
            assert g[key].tobytes() == w[key].tobytes(), key


@pytest.mark.skipif(os.getenv("SUBGC_POISON_EMPTY") == "1", reason="the poisoned run fills every torch.empty buffer with an ATen fill_ by design")
def test_scoring_a_decode_batch_issues_no_aten_device_kernel(case):
    """The method of tests/test_no_aten_gpu.py: after the one-time index build, scoring -- alone or inside eval_collect -- is C-ABI
    launches plus host <-> device copies."""
    from test_no_aten_gpu import Watch
    c = case
    rows = c["seq"].size(0)
    keep = torch.arange(rows, device=DEV)
    sizes = c["meta"]["sub_nums"]
    plan = c["scorer"].plan(c["draws"]["mb4"], sizes)

    def run():
        return (c["scorer"].score(c["seq"], c["bounds"], c["score"], c["draws"]["mb4"]),
                ops.eval_collect(c["score"], keep, c["seq"], c["bounds"], identity=True, diversity={"scorer": c["scorer"], "plan": plan}))

    run()
    torch.cuda.synchronize()
    with Watch() as w:
        per, h = run()
    torch.cuda.synchronize()
    assert not w.seen, dict(w.seen)
    inside = c["scorer"].unpack(plan, h["d_int"], h["d_f64"])
    for g, x in zip(per, inside):                                         # and the eval_collect path computed the same thing
        for key in g:
            assert g[key].tobytes() == x[key].tobytes(), key


def test_debug_bounds_reports_a_bad_draw_index_and_a_bad_seg(case):
    c = case
    sizes = c["meta"]["sub_nums"]
    bad = {m: [[d.copy() for d in per] for per in v] for m, v in c["draws"]["mb4"].items()}
    bad[3][3][1][2] = sizes[3]                                            # image 3 has rows 0 .. sizes[3] - 1
    neg = {m: [[d.copy() for d in per] for per in v] for m, v in c["draws"]["mb4"].items()}
    neg[1][0][0][0] = -1
    nt, n_img = 2, len(sizes)
    with ops.debug_bounds():
        c["scorer"].score(c["seq"], c["bounds"], c["score"], c["draws"]["mb4"])                  # valid: passes
        with pytest.raises(ops.SubgcError, match=rf"diversity_select: draw \(image-local row indices\): 1 entries outside their image's rows "
                                                 rf"\(first at set {n_img * nt + 3 * nt + 1}, position 2: {sizes[3]}; image 3 has {sizes[3]} rows\)"):
            c["scorer"].score(c["seq"], c["bounds"], c["score"], bad)
        with pytest.raises(ops.SubgcError, match="image-local row indices"):
            c["scorer"].score(c["seq"], c["bounds"], c["score"], neg)
        crooked = list(c["bounds"])
        crooked[2] = crooked[1] - 1
        with pytest.raises(ops.SubgcError, match=r"seg \(row boundaries of the images\) is not monotone.*first at image 1"):
            c["scorer"].score(c["seq"], crooked, c["score"], c["draws"]["mb4"])
    got = c["scorer"].score(c["seq"], c["bounds"], c["score"], bad)       # mode off: the documented clamp, no error, no fault
    torch.cuda.synchronize()
    for i in (0, 1, 2, 4, 5):                                             # the other images are untouched
        for key in got[i]:
            assert got[i][key].tobytes() == c["got"]["mb4"][i][key].tobytes()


def test_caption_images_with_diversity_end_to_end(golden):
    from subgc import consensus
    from test_consensus_gpu import _glue_model
    m, images, infos = _glue_model(golden)
    kw = dict(sample_max=1, beam_size=1, remove_bad_endings=0)
    voc = {str(i): f"w{i}" for i in range(1, 60)}
    before = eval_glue.caption_images(m, images, infos, voc, kw)
    train = [s for p in before for s in p["caption"][::3]] + ["w1 w2 zebra", "W1 w2."]
    ix = diversity.NoveltyIndex(train, voc, device=DEV)
    scorer = diversity.DiversityScorer(ix, 5)
    div = {"scorer": scorer, "top_n": (3, 100), "seed": 2019}
    after = eval_glue.caption_images(m, images, infos, voc, kw, diversity=div)
    import inspect
    assert inspect.signature(eval_glue.caption_images).parameters["diversity"].default is None       # off by default
    w2i = ix.word_to_ix
    for p0, p1 in zip(before, after):
        assert set(p1) - set(p0) == {"diversity"}
        for key, v in p0.items():                                         # nothing that was there changes, key for key
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(p1[key], v)
            else:
                assert p1[key] == v
        d = p1["diversity"]
        assert d["top_n"] == [3, 100]
        caps = [[w2i[w] for w in s.split(" ")] if s else [] for s in p1["caption"]]
        draws = diversity.per_image_draws([len(caps)], [p1["image_id"]], (3, 100), 2019)
        for metric in (1, 2, 3, 4):
            for t in range(2):
                _compare(d, t, G.restate(caps, p1["subgraph_score"], draws[metric][0][t], 5, ix.captions), metric, 5)
    assert sum(int(p["diversity"]["novel_of"][1] - p["diversity"]["novel"][1]) for p in after) > 0
    s = diversity.summarize([p["diversity"] for p in after])
    assert len(s["printed"]) == 10 and s["mbleu4_left_out"] == [sum(len(p["caption"]) < 2 for p in after)] * 2

    def same(a, b):
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key

    for group in (2, 256):                                                # the batch an image falls into cannot change its result
        for p1, p2 in zip(after, eval_glue.caption_images(m, images, infos, voc, kw, group=group, diversity=div)):
            same(p1["diversity"], p2["diversity"])
    back = eval_glue.caption_images(m, images[::-1], infos[::-1], voc, kw, diversity=div)[::-1]
    for p1, p2 in zip(after, back):
        same(p1["diversity"], p2["diversity"])
    # together with consensus= (and the grounding pass): both sets of keys, the same values
    rng = np.random.default_rng(11)
    words = [voc[str(i)] for i in range(1, 60)]
    sents = [[[words[min(int(x), len(words)) - 1] for x in rng.zipf(1.4, size=int(rng.integers(1, 12)))] for _ in range(3)] for _ in range(40)]
    rr = consensus.ConsensusReranker(consensus.ConsensusCorpus(sents, voc, device=DEV), k=8, m=10)
    nn = {info["id"]: [int(x) for x in rng.choice(40, 8, replace=False)] for info in infos}
    cons = {"reranker": rr, "nn": nn, "top_k": 4}
    kw_att = dict(kw, return_att=1)
    only = eval_glue.caption_images(m, images, infos, voc, kw_att, consensus=cons)
    both = eval_glue.caption_images(m, images, infos, voc, kw_att, consensus=cons, diversity=div)
    for p0, p1, p2 in zip(only, both, after):
        assert set(p1) - set(p0) == {"diversity"}
        same(p1["diversity"], p2["diversity"])
        np.testing.assert_array_equal(p1["consensus_rerank_ind"], p0["consensus_rerank_ind"])
        assert p1["consensus_sim"].tobytes() == p0["consensus_sim"].tobytes()
        np.testing.assert_array_equal(p1["grounding"]["node_ind"], p0["grounding"]["node_ind"])
    with pytest.raises(ValueError, match="sct"):
        eval_glue.caption_images(m, images, infos, voc, dict(kw, sct=1), diversity=div)
