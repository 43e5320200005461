"""Helpers of the tests of consensus re-ranking, method 'bleu': the fixture tests/golden/make_golden_consensus_bleu.py wrote by running
the reference's own calculate_bleu_sentence, and the derived bounds of DESIGN 4.O between the reference (math.fsum of the n F-scores)
and the device contract (their left-to-right sum), which subgc.consensus.bleu_pair_restatement / bleu_rerank_restatement restate."""
import json
import os

import numpy as np

from consensus_golden import corpus_sentences, rows_to_ids, word  # noqa: F401  (the fixture uses the CIDEr fixture's corpus layout)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53                       # the unit roundoff of fp64


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the bound on |prod of k factors (1 + d_i)^(+-1) - 1|, |d_i| <= u."""
    return k * U / (1.0 - k * U)


def pair_bound(n):
    """|contract - reference| <= pair_bound(n) * reference for one pair score.  Both divide a sum S of n non-negative F-scores, computed
    identically, by n.  Left to right: S (1 + t), |t| <= gamma(n - 1) (each term passes at most n - 1 roundings); fsum: one rounding; one
    more rounding each for the two divisions: n + 2 factors (1 + d) between the two results."""
    return gamma(n + 2)


def sim_bound(n, terms):
    """|contract - reference| <= sim_bound * reference for the sum of the `terms` = min(m, captions) largest pair scores.  With e =
    pair_bound(n) every pair score moves by at most e of itself, so the EXACT sum of the `terms` largest moves by at most e of itself
    whichever scores are the largest afterwards (it is the maximum over all subsets of that size, and each subset's sum moves by at
    most e of itself): two nearly equal scores swapping places are covered.  Each side then adds its sorted terms left to right: at
    most g = gamma(terms - 1) of its exact sum, whatever the order.  Together (e + g (1 + e) + g) of the reference's exact sum, which is
    at most its computed sum / (1 - g)."""
    e, g = pair_bound(n), gamma(max(terms - 1, 0))
    return (e + g * (1.0 + e) + g) / (1.0 - g)


def load():
    """-> (meta dict, arrays dict) of the committed fixture."""
    with open(os.path.join(GOLDEN, "consensus_bleu_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "consensus_bleu_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def vocab(V):
    return {str(i): word(i) for i in range(1, V + 1)}


def column(arr, meta, i, img, cap):
    """The column of image i's pair scores that belongs to caption `cap` of corpus image `img` (which must be among its first k neighbours)."""
    cap_off, col = arr["corpus_cap_off"], 0
    for j in arr["nn"][i][:meta["k"]]:
        if int(j) == img:
            return col + cap
        col += int(cap_off[j + 1] - cap_off[j])
    raise KeyError((i, img))


def within(got, want, rel):
    """|got - want| <= rel * |want|, elementwise; zeros must be zeros."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= rel * np.abs(want)))


def worst_rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nz = want != 0
    return float(np.max(np.abs(got - want)[nz] / np.abs(want)[nz], initial=0.0))


def check_edges(meta, arr, ids, name, pairs, sims, orders):
    """Every planted edge of the fixture, one by one, on one parameter set's results: pairs[i] [candidates, >= captions], sims[i],
    orders[i] per image (from the restatement or from the device)."""
    e, p, b = meta["edges"], meta["sets"][name], arr["bounds"]
    n, fpr, m = p["n"], p["fpr"], p["m"]
    cand = rows_to_ids(arr["cand"])
    ncap = [int(x) for x in arr["n_caps"]]
    col = lambda key: column(arr, meta, e[key][0], e[key][1], e[key][2])
    i, a = e["empty_candidate"]
    assert cand[b[i] + a] == [] and sims[i][a] == 0.0 and not pairs[i][a, :ncap[i]].any()
    # a candidate of n - 1 words scores 0 against everything (the guard tests n, not the order at hand); with the other n it does not
    i, a = e["three_word_candidate"]
    assert len(cand[b[i] + a]) == 3 and (sims[i][a] == 0.0) == (n == 4) and bool(pairs[i][a, :ncap[i]].any()) == (n != 4)
    i, a = e["one_word_candidate"]
    assert cand[b[i] + a] == [7] and sims[i][a] == 0.0 and not pairs[i][a, :ncap[i]].any()
    # a candidate of exactly n words scores
    i, a = e["four_word_candidate" if n == 4 else "two_word_candidate"]
    assert len(cand[b[i] + a]) == n and sims[i][a] > 0.0
    # neighbour captions: empty, n - 1 words (0 for every candidate), and the one-word caption with n = 2 (also shorter than n)
    i = e["empty_neighbour_caption"][0]
    assert ids[e["empty_neighbour_caption"][1]][e["empty_neighbour_caption"][2]] == [] and not pairs[i][:, col("empty_neighbour_caption")].any()
    assert ids[80][2] == [7, 8, 9] and ids[80][3] == [7]
    assert not pairs[i][:, col("one_word_neighbour_caption")].any()
    if n == 4:
        assert not pairs[i][:, col("three_word_neighbour_caption")].any()
    # clipping: word 20 three times in the candidate, once in the caption
    i, a = e["repeated_word_candidate"]
    assert cand[b[i] + a] == [20, 20, 21, 22, 23, 20] and ids[80][4] == [20, 21, 22, 23, 24, 25]
    acc = [4, 3, 2, 1]                                                      # unigrams 20 (clipped to 1), 21, 22, 23; 20-21 21-22 22-23; ...
    f = []
    for o in range(n):
        pre, rec = acc[o] / float(6 - o), acc[o] / float(6 - o)
        f.append(((fpr + 1) * pre * rec) / (rec + fpr * pre))
    want = f[0]
    for x in f[1:]:
        want = want + x
    assert pairs[i][a, col("clip_caption")] == want / float(n)
    # no common word: 0 everywhere
    i, a = e["no_common_word_candidate"]
    assert cand[b[i] + a] == [150, 151, 152, 153, 154] and sims[i][a] == 0.0 and not pairs[i][a, :ncap[i]].any()
    # unigrams only: f_1 = 1, the other orders 0, still divided by n
    i, a = e["unigrams_only_candidate"]
    assert pairs[i][a, col("distinct_words_caption")] == 1.0 / n
    i, a = e["identical_candidate"]
    assert cand[b[i] + a] == ids[80][5] and pairs[i][a, col("distinct_words_caption")] == 1.0
    # duplicates: equal bits, adjacent in the order, lower index first
    for key in ("duplicate_candidates", "triplicate_candidates"):
        i, *dup = e[key]
        assert all(cand[b[i] + x] == cand[b[i] + dup[0]] for x in dup)
        assert all(sims[i][x].tobytes() == sims[i][dup[0]].tobytes() for x in dup)
        o = [int(x) for x in orders[i]]
        at = o.index(dup[0])
        assert o[at:at + len(dup)] == dup
    # more / fewer neighbour captions than m
    big, small = e["more_captions_than_m_image"][name], e["fewer_captions_than_m_image"][name]
    assert ncap[big] > m > ncap[small] >= 1
    assert sims[small][0] == sum(sorted(pairs[small][0, :ncap[small]].tolist(), reverse=True))           # ALL pair scores are summed
    row = int(np.argmax((pairs[big][:, :ncap[big]] != 0).sum(1)))                                        # the candidate with the most scores
    top = sorted(pairs[big][row, :ncap[big]].tolist(), reverse=True)
    assert sims[big][row] == sum(top[:m])                                                                 # only the m largest
    if name == "B":
        assert top[m] > 0.0 and sims[big][row] < sum(top)                                                 # ... and that leaves scores out
    # long captions (57, 64, 200 words) are neighbours of image 0 and score; corpus-only words exist; the neighbour lists are longer than k
    for img, cap, L in e["long_captions"]:
        assert len(ids[img][cap]) == L and pairs[0][:, column(arr, meta, 0, img, cap)].any()
    assert max(max(c, default=0) for caps in ids for c in caps) > meta["V"]
    assert arr["nn"].shape[1] == e["neighbour_list_entries"] > meta["k"]
