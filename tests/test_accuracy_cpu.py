"""Accuracy scores without a GPU: the metrics header and its binding, the host tables of subgc.accuracy and `summarize` against the
fixture the reference's own scorers wrote (tests/golden/make_golden_accuracy.py), the plain restatement of tests/accuracy_golden.py
against the same fixture, the string -> id mapping of `score_predictions`, and every refusal."""
import pickle

import numpy as np
import pytest

import accuracy_golden as G
from subgc import _lib, accuracy
from subgc.accuracy import SubgcError


@pytest.fixture(scope="module")
def case():
    return G.load()


@pytest.fixture(scope="module")
def refs(case):
    meta, arr = case
    return accuracy.AccuracyReferences(G.fixture_refs(arr), G.vocab(meta["V"]), device=None)


def test_metrics_header_parses_and_the_core_header_is_untouched():
    protos = _lib.parse_header(_lib.METRICS_HEADER)
    assert sorted(protos) == ["subgc_accuracy_oracle", "subgc_accuracy_rows"]
    assert [a for _, a in protos["subgc_accuracy_oracle"][1]] == ["row_i", "ld_i", "row_d", "ld_d", "rows", "seg", "I", "oracle_num", "first",
                                                                 "img_i", "ld_ii", "img_d", "ld_id", "stream"]
    rows = [a for _, a in protos["subgc_accuracy_rows"][1]]
    assert len(rows) == 37 and rows[:6] == ["tok", "tok64", "T", "bad", "bad_n", "rows"] and rows[-6:] == ["beta2", "out_i", "ld_i", "out_d", "ld_d", "stream"]
    src = open(_lib.METRICS_HEADER).read()
    for name, value in (("SUBGC_ACC_ROW_INT", 10), ("SUBGC_ACC_ROW_F64", 6), ("SUBGC_ACC_IMG_INT", 56), ("SUBGC_ACC_IMG_F64", 12),
                        ("SUBGC_ACC_MAX_REFS", 32), ("SUBGC_ACC_MAX_REF_WORDS", 256)):
        assert f"#define {name} {value} " in src or f"#define {name} {value}\n" in src
    assert (accuracy.ROW_INT, accuracy.ROW_F64, accuracy.IMG_INT, accuracy.IMG_F64, accuracy.MAX_REFS, accuracy.MAX_REF_WORDS) == (10, 6, 56, 12, 32, 256)


def test_the_second_invoker_raises_with_the_last_error_and_knows_only_its_header():
    with pytest.raises(SubgcError, match="oracle_num >= 1 .got 0."):
        _lib.call_metrics("subgc_accuracy_oracle", None, 10, None, 6, 0, None, 0, 0, None, None, 56, None, 12, None)
    with pytest.raises(SubgcError, match="1 <= T <= 64 .got 65."):
        _lib.call_metrics("subgc_accuracy_rows", *([None, 0, 65, None, 0, 0, None, 0, None, 0] + [None] * 5 + [None, 0, None, None, 0] + [None] * 5 +
                                                   [None, None, None, 0, None, 0, 1.44, None, 10, None, 6, None]))


def test_host_tables_match_the_reference(case, refs):
    meta, arr = case
    np.testing.assert_array_equal(refs.bkeys, arr["bkeys"])
    np.testing.assert_array_equal(refs.bmax, arr["bmax"])
    np.testing.assert_array_equal(refs.boff, arr["boff"])
    np.testing.assert_array_equal(refs.ukeys, arr["df_keys"])
    np.testing.assert_array_equal(refs.ulogdf, np.log(np.maximum(1.0, arr["df"])))
    assert refs.ref_len == float(arr["ref_len"]) == float(np.log(float(len(meta["sizes"]))))
    one = int(np.searchsorted(refs.ukeys, np.uint64(meta["edges"]["word_in_every_image"]) << np.uint64(48)))
    assert refs.ulogdf[one] == refs.ref_len                               # the unigram in every image: weight 0
    assert refs.n_img == len(meta["sizes"]) and refs.n_ids > meta["V"]     # reference-only words got ids above the vocabulary


def test_the_planted_cases_are_in_the_fixture(case):
    meta, arr = case
    e, b, caps, R = meta["edges"], arr["bounds"], G.rows_to_ids(arr["seq"]), G.fixture_refs(arr)
    row = lambda ic: int(b[ic[0]] + ic[1])
    assert caps[row(e["empty_candidate"])] == [] and (arr["row_d"][row(e["empty_candidate"]), :5] == 0.0).all()
    assert arr["row_d"][row(e["empty_candidate"]), 5] == 1.0 and R[e["empty_reference"][0]][e["empty_reference"][1]] == []
    assert len(caps[row(e["one_word_candidate"])]) == 1 and len(caps[row(e["full_length_candidate"])]) == 64 == meta["T"]
    assert len(R[e["one_reference"]]) == 1 and len(R[e["seven_references"]]) == 7
    i, c = e["shorter_than_every_reference"]
    assert all(len(r) > len(caps[row((i, c))]) for r in R[i]) and 0 < arr["row_d"][row((i, c)), 0] < 1
    i, c = e["closest_length_tie"]
    L = len(caps[row((i, c))])
    assert {L - 1, L + 1} <= {len(r) for r in R[i]} and L not in {len(r) for r in R[i]} and arr["row_i"][row((i, c)), 1] == L - 1
    assert len(R[e["reference_over_64_words"][0]][e["reference_over_64_words"][1]]) > 64
    assert len(R[e["reference_256_words"][0]][e["reference_256_words"][1]]) == 256
    sizes = meta["sizes"]
    assert sizes[e["one_candidate"]] == 1 and sizes[e["fewer_than_oracle_num"]] == 3 and sizes[e["many_candidates"]] == 130
    i, x, y = e["duplicate_candidates"]
    assert caps[b[i] + x] == caps[b[i] + y] and (arr["row_d"][b[i] + x] == arr["row_d"][b[i] + y]).all()
    assert (arr["row_i"][row(e["unseen_ngrams"]), 6:] == 0).all()
    i, c = e["clipped_repeats"]
    assert arr["row_i"][row((i, c)), 6] < arr["row_i"][row((i, c)), 2]
    assert meta["smallest_relative_gap"] > 1e-9 and meta["oracle_nums"] == [1, 5, 20, 1000] and len(sizes) == 40


def test_summarize_reproduces_the_reference_corpus_numbers(case):
    meta, arr = case
    for q, N in enumerate(meta["oracle_nums"]):
        s = accuracy.summarize(G.fixture_per_image(meta, arr, q))
        assert [s[n] for n in accuracy.NAMES[:4]] == arr["top1"][:4].tolist()               # BLEU from the integers: equal bits
        assert [s["oracle"][n] for n in accuracy.NAMES[:4]] == arr["oracle"][q, :4].tolist()
        assert s["CIDEr"] == arr["top1"][4] and s["ROUGE_L"] == arr["top1"][5]              # np.mean of the same values
        assert s["oracle"]["CIDEr"] == arr["oracle"][q, 4] and s["oracle"]["ROUGE_L"] == arr["oracle"][q, 5]
        assert s["images"] == len(meta["sizes"]) and s["left_out"] == 0
    empty = {"n": 0}
    s2 = accuracy.summarize(G.fixture_per_image(meta, arr, 0) + [empty])
    assert s2["left_out"] == 1 and s2["Bleu_4"] == s["Bleu_4"]


def test_restatement_matches_the_reference_fixture(case, refs):
    """The restatement the GPU tests lean on for other shapes: integers and picks exactly, values within the device's own bounds."""
    meta, arr = case
    ref_ids = [[refs.encode(c) for c in caps] for caps in G.fixture_refs(arr)]
    cands, b = G.rows_to_ids(arr["seq"]), arr["bounds"].tolist()
    rows = G.restate_rows(cands, b, list(range(len(b) - 1)), ref_ids)
    for q, N in enumerate(meta["oracle_nums"]):
        got = G.restate(cands, b, list(range(len(b) - 1)), ref_ids, N, rows=rows)
        worst = G.compare(got, G.fixture_per_image(meta, arr, q))
        assert worst[0] <= G.BLEU_TOL and worst[1] <= G.CIDER_TOL and worst[2] <= G.ROUGE_TOL, worst


def test_predictions_are_mapped_from_strings_to_ids(case, refs):
    meta, arr = case
    cands, b = G.rows_to_ids(arr["seq"]), arr["bounds"]
    preds = [{"image_id": 1000 + i, "caption": [" ".join(f"w{x}" for x in c) for c in cands[b[i]:b[i + 1]]]} for i in range(3)]
    seq, bounds = accuracy.encode_predictions(preds, refs)
    assert bounds == b[:4].tolist() and seq.dtype == np.int64 and seq.shape == (b[3], 64)
    np.testing.assert_array_equal(seq, arr["seq"][:b[3]].astype(np.int64))
    with pytest.raises(SubgcError, match="'zebra' is neither in the model's vocabulary nor in the references .a caption of image 7."):
        accuracy.encode_predictions([{"image_id": 7, "caption": ["w1 zebra"]}], refs)
    with pytest.raises(SubgcError, match="a caption of 65 words; the limit is 64"):
        accuracy.encode_predictions([{"image_id": 7, "caption": [" ".join(["w1"] * 65)]}], refs)


def test_refusals_name_their_numbers(refs):
    v = {"1": "a", "2": "b"}
    with pytest.raises(SubgcError, match="image 1 has 0 reference captions"):
        accuracy.AccuracyReferences([[["a"]], []], v, device=None)
    with pytest.raises(SubgcError, match="image 0 has 33 reference captions; the limit is 32"):
        accuracy.AccuracyReferences([[["a"]] * 33], v, device=None)
    with pytest.raises(SubgcError, match="a reference caption of 257 words .image 0.; the limit is 256"):
        accuracy.AccuracyReferences([[["a"] * 257]], v, device=None)
    with pytest.raises(SubgcError, match="accuracy: the references need 65536 word ids, the 16-bit n-gram lanes hold 65535"):
        accuracy.AccuracyReferences([[["zebra"]]], {str(i): f"m{i}" for i in range(1, 65536)}, device=None)
    with pytest.raises(SubgcError, match="lists of words"):
        accuracy.AccuracyReferences([["a b"]], v, device=None)
    with pytest.raises(SubgcError, match="no reference images"):
        accuracy.AccuracyReferences([], v, device=None)
    with pytest.raises(SubgcError, match="oracle_num = 0"):
        accuracy.AccuracyScorer(refs, 0)
    sc = accuracy.AccuracyScorer(refs, 5)
    with pytest.raises(SubgcError, match="batch image 1 names reference image 40; the references hold 40 images"):
        sc.check_index([0, 40])
    import torch
    with pytest.raises(SubgcError, match="no CPU fallback"):
        sc.score(torch.zeros(2, 4, dtype=torch.int64), [0, 2], [0])


def test_entries_are_plain_data_and_survive_the_gather(case):
    from subgc import parallel
    meta, arr = case
    b = arr["bounds"].tolist()[:6]
    rows, I = b[-1], 5
    host = np.arange(accuracy.AccuracyScorer.arena_words(rows, I), dtype=np.int32)
    sc = accuracy.AccuracyScorer.__new__(accuracy.AccuracyScorer)
    sc.oracle_num = 20
    per = sc.unpack(host, b)
    assert len(per) == I and per[2]["material"].shape == (b[3] - b[2], 10) and per[2]["oracle_material"].shape == (4, 10)
    row_d, row_i, img_d, img_i = sc.views(host, rows, I)
    assert row_i[0, 0] == 2 * (6 * rows + 12 * I) and img_i[0, 0] == row_i[0, 0] + 10 * rows and per[1]["top1_row"] == img_i[1, 1]
    back = parallel.gather_by_index(pickle.loads(pickle.dumps(per[::-1])), list(range(I))[::-1], I)
    for a, c in zip(per, back):
        assert sorted(a) == sorted(c) and all(np.array_equal(np.asarray(a[k]), np.asarray(c[k])) for k in a)
