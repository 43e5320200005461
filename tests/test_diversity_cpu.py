"""Diversity scores without a GPU: the host half of subgc.diversity -- the script's draw stream, the per-image draws, the
training-caption index and the summary -- against the fixture the reference's own diversity_score.py wrote
(tests/golden/make_golden_diversity.py), the set-and-dict restatement of tests/diversity_golden.py against the same fixture, and the
three new prototypes of the header."""
import numpy as np
import pytest

import diversity_golden as G
from subgc import _lib, diversity


@pytest.fixture(scope="module")
def case():
    return G.load()


@pytest.mark.parametrize("run", ["mb4", "plain"])
def test_reference_draws_reproduce_the_recorded_stream(case, run):
    meta, arr = case
    want = G.fixture_draws(meta, arr, run)
    got = diversity.reference_draws(meta["sub_nums"], tuple(meta["top_n"]), evaluate_mB4=run == "mb4", seed=meta["seed"])
    assert sorted(got) == sorted(want) == ([1, 2, 3, 4] if run == "mb4" else [1, 2, 3])
    for metric in want:
        for i, per in enumerate(want[metric]):
            for t, d in enumerate(per):
                np.testing.assert_array_equal(got[metric][i][t], d)
                assert len(d) == min(meta["top_n"][t], meta["sub_nums"][i]) and len(set(d.tolist())) == len(d)
    # the property that makes the draws an input: without --evaluate_mB4 metric 3 gets the draws metric 4 had with it
    if run == "plain":
        with_mb4 = G.fixture_draws(meta, arr, "mb4")
        np.testing.assert_array_equal(want[3][8][1], with_mb4[4][8][1])
        assert not np.array_equal(want[3][8][1], with_mb4[3][8][1])


def test_per_image_draws_do_not_depend_on_order_or_batching():
    subs, keys = [5, 400, 1, 20, 0, 120], [17, "COCO_val_42", 3, 99, 8, 12345678901]
    whole = diversity.per_image_draws(subs, keys, (20, 100), 2019)
    assert sorted(whole) == [1, 2, 3, 4]
    perm = [4, 2, 0, 5, 1, 3]
    shuffled = diversity.per_image_draws([subs[p] for p in perm], [keys[p] for p in perm], (20, 100), 2019)
    for metric in whole:
        for j, p in enumerate(perm):
            for t in range(2):
                np.testing.assert_array_equal(shuffled[metric][j][t], whole[metric][p][t])
        for i in range(len(subs)):                                        # one image at a time = any batching
            alone = diversity.per_image_draws([subs[i]], [keys[i]], (20, 100), 2019)
            for t, k in enumerate((20, 100)):
                np.testing.assert_array_equal(alone[metric][0][t], whole[metric][i][t])
                d = whole[metric][i][t]
                assert len(d) == min(k, subs[i]) and len(set(d.tolist())) == len(d) and all(0 <= x < subs[i] for x in d)
    # metric, top_n, key and seed all enter
    assert not np.array_equal(whole[1][1][1], whole[2][1][1])
    assert not np.array_equal(whole[1][1][0], whole[1][1][1][:20])
    assert not np.array_equal(whole[1][1][1], diversity.per_image_draws([400], ["COCO_val_43"], (20, 100), 2019)[1][0][1])
    assert not np.array_equal(whole[1][1][1], diversity.per_image_draws([400], ["COCO_val_42"], (20, 100), 7)[1][0][1])
    with pytest.raises(diversity.SubgcError, match="one image key per image"):
        diversity.per_image_draws([1, 2], [1], (20,), 0)


def test_novelty_index_keeps_and_drops_the_planted_strings(case):
    meta, _ = case
    e = meta["edges"]
    ix = diversity.NoveltyIndex(meta["train"], G.vocab(meta["V"]), device=None)
    w = ix.word_to_ix
    assert tuple(w[x] for x in e["train_equal"].split(" ")) in ix.captions and e["train_equal"] in ix
    raw, lowered = e["train_equal_after_lower_and_dot"]
    assert raw in meta["train"] and lowered not in meta["train"] and lowered in ix
    assert e["train_empty_after_dot"] in meta["train"] and () in ix.captions and "" in ix       # '.' -> '' -> the zero-word caption
    for key in ("train_double_space_dropped", "train_out_of_vocabulary_dropped", "train_trailing_space_dropped"):
        assert e[key] in meta["train"]
    assert ix.dropped == 3
    assert "w1 w2" not in ix and "w4 w5" not in ix and "w4 w5 w6" not in ix                 # what a careless split() would have let in
    assert e["only_in_a_validation_image"] not in ix
    # the device tables: distinct captions in lexicographic order of their id lists, a prefix first
    caps = [tuple(int(x) for x in ix.tok[ix.off[c]:ix.off[c + 1]]) for c in range(ix.n)]
    assert caps == sorted(ix.captions) and len(set(caps)) == len(caps) and caps[0] == ()
    with pytest.raises(diversity.SubgcError, match="one to one"):
        diversity.NoveltyIndex([], {"1": "a", "2": "a"}, device=None)
    with pytest.raises(diversity.SubgcError, match="word ids are 1"):
        diversity.NoveltyIndex([], {"0": "a"}, device=None)


@pytest.mark.parametrize("run", ["mb4", "plain"])
def test_summarize_turns_the_per_image_expectations_into_the_printed_numbers(case, run):
    meta, arr = case
    s = diversity.summarize(G.fixture_per_image(meta, arr, run))
    want = meta["runs"][run]["printed"]
    assert len(s["printed"]) == len(want) == (10 if run == "mb4" else 8)
    assert s["printed"] == want                                           # the script's own expressions on the same numbers: equal bits
    if run == "mb4":
        assert s["mbleu4"] == want[:2] and s["mbleu4_left_out"] == [0, 0]
    assert [s["unigram"][0], s["bigram"][0], s["unigram"][1], s["bigram"][1]] == want[-8:-4]
    assert s["novel"] == want[-4:-2] and s["distinct"] == want[-2:]
    # an image without a valid mBLEU is left out and counted
    if run == "mb4":
        per = G.fixture_per_image(meta, arr, run)
        per[0] = dict(per[0], mbleu4_valid=np.array([False, True]), mbleu4=np.array([np.nan, per[0]["mbleu4"][1]]))
        s2 = diversity.summarize(per)
        assert s2["mbleu4_left_out"] == [1, 0] and s2["mbleu4"][1] == s["mbleu4"][1] and s2["mbleu4"][0] != s["mbleu4"][0]
        assert s2["mbleu4"][0] == float(np.mean(np.array([e["mbleu4"][0] for e in per[1:]])))


def test_restatement_matches_the_reference_fixture(case):
    """The set-and-dict restatement the GPU tests lean on for other sizes gives the fixture's counts exactly and its BLEU values to 1e-14."""
    meta, arr = case
    b, caps, score = arr["bounds"], G.rows_to_ids(arr["seq"]), arr["score"]
    ix = diversity.NoveltyIndex(meta["train"], G.vocab(meta["V"]), device=None)
    draws, exp = G.fixture_draws(meta, arr, "mb4"), arr["exp_mb4"]
    for i in range(len(b) - 1):
        mine, sc = caps[b[i]:b[i + 1]], score[b[i]:b[i + 1]]
        for t in range(len(meta["top_n"])):
            r = {m: G.restate(mine, sc, draws[m][i][t], meta["n_best"], ix.captions) for m in (1, 2, 3, 4)}
            assert [r[1]["drawn"], r[1]["distinct"], r[3]["words"], r[3]["unigrams"], r[3]["bigrams"], r[2]["novel"]] == exp[i, t, :6].tolist()
            n = len(r[4]["selected"])
            assert r[4]["selected"] == arr["selected"][i, t, :n].tolist()
            assert G.close(r[4]["bleu4"], arr["bleu4"][i, t, :n], 1e-14)


def test_the_planted_cases_are_in_the_fixture(case):
    meta, arr = case
    e, b, caps = meta["edges"], arr["bounds"], G.rows_to_ids(arr["seq"])
    assert sorted(set(meta["sub_nums"])) == [2, 3, 5, 7, 20, 21, 100, 120, 400] and min(meta["sub_nums"]) >= 2
    for i in range(len(b) - 1):
        sc = arr["score"][b[i]:b[i + 1]]
        assert len(np.unique(sc)) == len(sc)                              # ties are the device's to define: none in the fixture
    i, c = e["empty_caption_selected"]
    assert caps[b[i] + c] == [] and c in arr["selected"][i, 0]
    i, c = e["one_word_caption"]
    assert len(caps[b[i] + c]) == 1 and c in arr["selected"][i, 0]
    i, c = e["full_length_caption"]
    assert len(caps[b[i] + c]) == meta["T"] == arr["seq"].shape[1]
    for key, lens in (("closest_length_tie", (1, 5)), ("closest_length_tie_2", (6, 8))):
        i, c = e[key]
        sel = [x for x in arr["selected"][i, 0] if x >= 0]
        others = [len(caps[b[i] + x]) for x in sel if x != c]
        L = len(caps[b[i] + c])
        assert c in sel and lens[0] in others and lens[1] in others and L - lens[0] == lens[1] - L == min(abs(o - L) for o in others)
    i, c = e["shorter_than_every_reference"]
    sel = [x for x in arr["selected"][i, 0] if x >= 0]
    assert all(len(caps[b[i] + x]) > len(caps[b[i] + c]) for x in sel if x != c)
    q = sel.index(c)
    assert 0 < arr["bleu4"][i, 0, q] < 1                                  # a real value under the brevity factor, not the 1e-15 floor
    i, x, y = e["duplicates_in_a_draw"]
    assert caps[b[i] + x] == caps[b[i] + y] and arr["exp_mb4"][i, 0, 1] < arr["exp_mb4"][i, 0, 0]
    p = meta["runs"]["mb4"]["printed"]
    assert p[0] > 0.05 and p[1] > 0.05 and p[8] < 1 and p[9] < 1


def test_plan_and_unpack_lay_the_sets_out_and_the_entries_are_plain_data(case):
    import pickle
    from subgc import ops, parallel
    meta, arr = case
    scorer = diversity.DiversityScorer(None, meta["n_best"])
    draws = G.fixture_draws(meta, arr, "mb4")
    plan = scorer.plan(draws, meta["sub_nums"])
    n_img, nt = len(meta["sub_nums"]), 2
    S = plan["n_sets"]
    assert S == 3 * n_img * nt and plan["max_draw"] == 100          # no novelty index: metric 2 has no sets
    assert [m for m, _, _ in plan["index"][::n_img * nt]] == [4, 3, 1] and plan["index"][nt + 1] == (4, 1, 1)
    tab = plan["table"]
    assert tab.dtype == np.int32 and len(tab) == 3 * S + 1 + plan["n_draw"]
    img, flags, off, flat = tab[:S], tab[S:2 * S], tab[2 * S:3 * S + 1], tab[3 * S + 1:]
    assert flags.tolist() == [4] * (n_img * nt) + [2] * (n_img * nt) + [1] * (n_img * nt) and off[0] == 0 and off[-1] == plan["n_draw"]
    for s, (m, i, t) in enumerate(plan["index"]):
        assert img[s] == i
        np.testing.assert_array_equal(flat[off[s]:off[s + 1]], draws[m][i][t])
    h_int = np.zeros((S, ops.DIV_COLS + 5), np.int32)
    h_int[:, 0], h_int[:, 1], h_int[:, 2], h_int[:, 3], h_int[:, 7] = 20, 10, 5, 40, 1
    per = scorer.unpack(plan, h_int, np.full((S, 6), 0.25), (20, 100))
    assert len(per) == n_img and "novel" not in per[0] and per[3]["distinct"].tolist() == [10, 10] and per[3]["mbleu4"].tolist() == [0.25, 0.25]
    back = parallel.gather_by_index(pickle.loads(pickle.dumps(per[::-1])), list(range(n_img))[::-1], n_img)
    for a, b in zip(per, back):
        assert sorted(a) == sorted(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    with pytest.raises(diversity.SubgcError, match="limit is 1024"):
        scorer.plan({1: [[np.zeros(1025, np.int64)]]}, [2000])
    with pytest.raises(diversity.SubgcError, match="draws for 1 images, the batch holds 2"):
        scorer.plan({1: [[np.zeros(1, np.int64)]]}, [3, 3])


def test_new_prototypes_parse_from_the_header():
    protos = _lib.parse_header()
    names = [n for n in protos if n.startswith("subgc_diversity_")]
    assert sorted(names) == ["subgc_diversity_best", "subgc_diversity_distinct", "subgc_diversity_select"]
    assert [a for _, a in protos["subgc_diversity_select"][1]] == ["score", "seg", "I", "rows", "set_img", "set_off", "draw", "n_sets", "n_draw",
                                                                  "max_draw", "n_best", "out_i", "ld_i", "stream"]
    assert len(protos["subgc_diversity_distinct"][1]) == 18 and len(protos["subgc_diversity_best"][1]) == 20
    src = open(_lib.HEADER).read()
    for name, value in (("SUBGC_DIV_SEL", 8), ("SUBGC_DIV_WANT_DRAW", 1), ("SUBGC_DIV_WANT_WORDS", 2), ("SUBGC_DIV_WANT_BLEU", 4)):
        assert f"#define {name} {value}\n" in src
    from subgc import ops
    assert ops.DIV_COLS == 8 and ops.DIV_WANT == {1: 1, 2: 2, 3: 2, 4: 4}
    assert len(protos) == 133
