"""Grounding scores without a GPU: the third header and its binding, the cooked tables of subgc.grounding and `summarize` against the
fixture the reference's own evaluator wrote (tests/golden/make_golden_grounding.py), and the cook's refusals."""
import math

import numpy as np
import pytest

import grounding_golden as G
from subgc import _lib, grounding
from subgc.grounding import SubgcError

SETS = ["rnd", "edge", "nan", "grd_subgc_0", "grd_subgc_1", "grd_fullgc_0", "grd_fullgc_1"]


@pytest.fixture(scope="module")
def case():
    return G.load()


def test_grounding_header_parses_and_the_other_two_are_untouched():
    protos = _lib.parse_header(_lib.GROUNDING_HEADER)
    assert sorted(protos) == ["subgc_grounding_material", "subgc_grounding_score"]
    assert [a for _, a in protos["subgc_grounding_material"][1]] == [
        "tok", "tok64", "T", "bad", "bad_n", "rows", "seg", "pick", "I", "node", "T1", "n_words", "tok_class", "n_tok_class", "box_off", "boxes",
        "n_boxes", "mat_n", "mat_cls", "mat_idx", "mat_box", "ld_m", "stream"]
    assert [a for _, a in protos["subgc_grounding_score"][1]] == [
        "mat_n", "mat_cls", "mat_box", "ld_m", "I", "img_ref", "n_ref", "pair_off", "n_pairs", "cap_off", "n_caps", "obj_off", "obj_cls", "obj_idx",
        "obj_box", "n_obj", "ex_off", "ex_lemma", "n_ex", "class_lemma", "n_class", "iou_thresh", "prec_off", "prec", "n_prec", "rec_off", "rec",
        "n_rec", "stream"]
    import ctypes
    assert protos["subgc_grounding_score"][1][21][0] is ctypes.c_float
    src = open(_lib.GROUNDING_HEADER).read()
    for name, value in (("SUBGC_GRD_MISS", grounding.MISS), ("SUBGC_GRD_HIT", grounding.HIT), ("SUBGC_GRD_SKIP", grounding.SKIP),
                        ("SUBGC_GRD_HALLUCINATED", grounding.HALLUCINATED), ("SUBGC_GRD_ABSENT", grounding.ABSENT), ("SUBGC_GRD_NONE", grounding.NONE),
                        ("SUBGC_GRD_MAX_WORDS", grounding.MAX_WORDS), ("SUBGC_GRD_MAX_OBJ", grounding.MAX_OBJ)):
        assert f"#define {name} {value} " in src or f"#define {name} {value}\n" in src, name
    assert (grounding.MISS, grounding.HIT, grounding.SKIP, grounding.HALLUCINATED, grounding.ABSENT, grounding.MAX_WORDS, grounding.MAX_OBJ) == (
        0, 1, 2, 3, 4, 64, 64)


def test_each_invoker_knows_only_its_own_header():
    with pytest.raises(SubgcError, match="1 <= T <= 64 .got 65."):
        _lib.call_grounding("subgc_grounding_material", None, 0, 65, None, 0, 0, None, None, 0, None, 1, None, None, 0, None, None, 0, None, None, None,
                            None, 64, None)
    with pytest.raises(SubgcError, match="ld_m >= 1 .got 0."):
        _lib.call_grounding("subgc_grounding_score", *([None, None, None, 0, 0, None, 0, None, 0, None, 0] + [None] * 4 + [0, None, None, 0, None, 0, 0.5,
                                                                                                                  None, None, 0, None, None, 0, None]))


@pytest.mark.parametrize("tag", ["rnd", "edge", "grd_subgc_0"])
def test_cooked_tables_match_the_fixture(case, tag):
    meta, arr = case
    refs = G.references(meta, arr, tag)
    anns, split = G.annotations(meta, arr, tag)
    t, W = meta["sets"][tag]["annotations"], meta["words"]
    keep = [j for j, a in enumerate(anns) if a["image_id"] in split]
    assert refs.image_ids == [str(anns[j]["image_id"]) for j in keep] and refs.n_img == len(keep)
    cap, obj = arr[t + "_cap_off"], arr[t + "_obj_off"]
    caps = [s for j in keep for s in range(cap[j], cap[j + 1])]
    np.testing.assert_array_equal(np.diff(refs.cap_off), [cap[j + 1] - cap[j] for j in keep])
    np.testing.assert_array_equal(np.diff(refs.obj_off), [obj[s + 1] - obj[s] for s in caps])
    sel = np.concatenate([np.arange(obj[s], obj[s + 1]) for s in caps] + [np.zeros(0, np.int64)]).astype(np.int64)
    assert [refs.class_names[c] for c in refs.obj_cls] == [W[x] for x in arr[t + "_obj_cls"][sel]]
    np.testing.assert_array_equal(refs.obj_idx, arr[t + "_obj_idx"][sel])
    np.testing.assert_array_equal(refs.obj_box, arr[t + "_obj_box"][sel].astype(np.float32))
    assert refs.obj_box.dtype == np.float32 and refs.obj_box.shape == (len(sel), 4)
    # the excluded lemmas of every caption: ascending ids on the device side, the fixture's strings as a set
    np.testing.assert_array_equal(np.diff(refs.ex_off), np.diff(arr[t + "_ex_off"]))
    name = {v: k for k, v in refs.lemma_id.items()}
    for s in range(len(caps)):
        mine = refs.ex_lemma[refs.ex_off[s]:refs.ex_off[s + 1]]
        assert (np.diff(mine) > 0).all()
        assert sorted(name[x] for x in mine) == [W[x] for x in arr[t + "_ex_lemma"][arr[t + "_ex_off"][s]:arr[t + "_ex_off"][s + 1]]]
    if not tag.startswith("grd_"):
        # the class list: the detection words by id, then the process_clss words outside them; a class word's lemma through the lemmatizer
        assert refs.class_names[:12] == [meta["det_id_to_det_wd"][str(k)] for k in range(1, 13)]
        assert set(refs.class_names[12:]) == set(meta["extra_classes"]) and refs.n_class == 14 == len(set(refs.class_names))
        assert name[refs.class_lemma[refs.class_id["c3s"]]] == "c3" and name[refs.class_lemma[refs.class_id["c1"]]] == "c1"
        # vocabulary id -> class: w<i> -> l<i> -> detection id i ("with" -> l12 too); other bad endings, non-class lemmas, unknown words: none
        assert refs.tok_class.tolist() == [-1] + list(range(12)) + [-1, -1, 11, -1, -1, -1]
        assert refs.bad.tolist() == [0] * 13 + [1, 1, 1, 0, 0, 0]
    for j, k in enumerate(keep):
        assert {refs.class_names[c] for c in refs.img_classes[j]} == {w for c in anns[k]["captions"] for w in c["process_clss"]}


@pytest.mark.parametrize("tag", SETS)
def test_summarize_reproduces_the_reference_numbers(case, tag):
    meta, arr = case
    refs = G.references(meta, arr, tag)
    want = arr[tag + "_numbers"].tolist()
    entries = G.expected_entries(meta, arr, tag, refs)
    s = grounding.summarize(entries, refs)
    got = G.numbers(s)
    assert s["num_vocab"] == meta["sets"][tag]["num_vocab"]
    assert all((g == w) or (math.isnan(g) and math.isnan(w)) for g, w in zip(got, want)), (got, want)      # reference order: equal bits
    G.close(got, want, s["num_vocab"])
    # the per-class lists are the evaluator's own, in its order of first appearance
    for mode in ("all", "loc"):
        for side, key in (("precision", "prec"), ("recall", "recall")):
            assert s["per_class_" + mode][side] == meta["sets"][tag]["per_class"][mode][key], (mode, side)
    # any order of the entries gives the same bits: the images are walked in reference order
    G.close(G.numbers(grounding.summarize(entries[::-1], refs)), want, s["num_vocab"])
    assert G.numbers(grounding.summarize(entries[::-1], refs))[:2] == got[:2]


def test_nan_and_missing_image_rules(case):
    meta, arr = case
    want = arr["nan_numbers"]
    assert want[0] == 0.0 and want[1] == 0.0 and np.isnan(want[2]) and np.isnan(want[5])
    refs = G.references(meta, arr, "edge")
    e = meta["edges"]["missing_image"]
    entries = G.expected_entries(meta, arr, "edge", refs)
    j = refs.index[str(e["image"])]
    assert j not in [x["ref"] for x in entries] and 0 < j < refs.n_img - 1               # in the split, in the middle, not submitted
    s = grounding.summarize(entries, refs)
    assert s["missing"] == 1 and s["images"] == refs.n_img - 1
    for mode in ("all", "loc"):                                                          # zeros in BOTH modes, nothing in precision
        assert s["per_class_" + mode]["recall"][e["class"]] == [0, 0] and e["class"] not in s["per_class_" + mode]["precision"]
    assert refs.class_id[e["class"]] in refs.img_classes[j] and s["num_vocab"] == meta["sets"]["edge"]["num_vocab"] == 10
    # once the image has an entry its class counts: num_vocab grows by one and every number shrinks by that factor
    sc = grounding.GroundingScorer(refs)
    s2 = grounding.summarize(entries + [sc.empty_entry(j)], refs)
    assert s2["num_vocab"] == 11 and s2["missing"] == 0
    assert s2["per_class_all"]["recall"][e["class"]] == [0, 0] and e["class"] not in s2["per_class_loc"]["recall"]
    assert s2["prec_all"] == pytest.approx(s["prec_all"] * 10 / 11, rel=1e-15)
    # a class that only ever appears hallucinated: 0 to the sum, nothing to num_vocab
    lone = [x for x in entries if x["ref"] == refs.index["9003"]]
    s3 = grounding.summarize(lone, refs)
    assert s3["num_vocab"] == 0 and s3["per_class_all"]["precision"] == {"c5": [0]} and s3["per_class_loc"]["precision"] == {}
    # image ids outside the split are not cooked
    assert str(meta["edges"]["outside_the_split"]) not in refs.index


def test_the_planted_cases_are_in_the_fixture(case):
    meta, arr = case
    e = meta["edges"]
    for name in ("iou_exactly_half", "nearest_hit", "disjoint", "fraction_of_a_pixel", "fp32_hit_fp64_miss", "fp32_miss_fp64_hit", "zero_area_gt",
                 "zero_area_pred", "zero_area_both", "identical", "predicted_twice_annotated_twice", "lemma", "caption_without_objects",
                 "five_captions", "one_caption", "empty_predicted_list", "sixty_four_words", "missing_image"):
        assert name in e, name
    assert e["iou_exactly_half"]["code"] == grounding.MISS and e["nearest_hit"]["code"] == grounding.HIT and e["nearest_hit"]["ulps_above"] >= 1
    assert e["fp32_hit_fp64_miss"]["code"] == grounding.HIT and e["fp32_miss_fp64_hit"]["code"] == grounding.MISS
    for tag in ("rnd",):
        s = meta["sets"][tag]
        assert min(s["precision_code_counts"][:4]) >= 5 and min(s["recall_code_counts"][:2] + s["recall_code_counts"][4:]) >= 5
    res = G.results(meta, arr, "edge")
    assert len(res["9006"][0]["clss"]) == 64 and res["9005"][0]["clss"] == []
    anns, _ = G.annotations(meta, arr, "edge")
    by = {a["image_id"]: a for a in anns}
    assert len(by[9004]["captions"]) == 5 and len(by[9000]["captions"]) == 1 and by[9003]["captions"][0]["process_clss"] == []
    assert "" in by[9002]["captions"][0]["tokens"] and by[9001]["captions"][0]["process_idx"] == [5, 2]


def test_refusals_name_their_numbers(case):
    meta, arr = case
    cap = lambda idx, box, n=None: {"tokens": ["t1"] * 70, "process_clss": ["c1"] * (len(idx) if n is None else n), "process_idx": idx, "process_bnd_box": box}
    mk = lambda c: grounding.GroundingReferences([{"image_id": 1, "captions": [c]}], [1], meta["det_id_to_det_wd"], G.WD_TO_LEMMA, G.LEMMA_DET, G.VOCAB,
                                                 meta["lemma"], device=None)
    with pytest.raises(SubgcError, match="a duplicate process_idx .image 1, caption 0"):
        mk(cap([2, 2], [[0, 0, 1, 1]] * 2))
    with pytest.raises(SubgcError, match="65 objects .image 1, caption 0.; the limit is 64"):
        mk(cap(list(range(65)), [[0, 0, 1, 1]] * 65))
    with pytest.raises(SubgcError, match=r"process_bnd_box is \[n_obj, 4\]"):
        mk(cap([0, 1], [[0, 0, 1, 1, 1]] * 2))
    with pytest.raises(SubgcError, match=r"process_bnd_box is \[n_obj, 4\]"):
        mk(cap([0, 1], [[0, 0, 1, 1]]))
    refs = mk(cap(list(range(64)), [[0, 0, 1, 1]] * 64))                  # the limit itself is fine
    assert refs.n_obj == 64 and refs.n_caps == 1
    sc = grounding.GroundingScorer(refs)
    with pytest.raises(SubgcError, match="batch image 1 names reference image 1; the references hold 1 images"):
        sc.check_index([0, 1])
    with pytest.raises(SubgcError, match=r"boxes are \[n, 4\]"):
        grounding.prepare_boxes(np.zeros((3, 5)))
    b = grounding.prepare_boxes(np.array([[1.0, 2.0, 3.0, 4.0]]), (900, 400))
    assert b.dtype == np.float32 and b[0, 0] == np.float32(1.0 * 900 / 592)
    plan = sc.plan([0, 0])
    assert plan["P"] == 2 and plan["n_prec"] == 128 and plan["n_rec"] == 128 and sc.arena_words(plan) == 2 + 6 * 2 * 64 + 32 + 32
