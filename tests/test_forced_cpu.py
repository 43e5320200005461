"""Forced decode and GT-sentence grounding without a GPU: the eighth header and its binding, the host-side refusals, the numpy restatement
of the score contract (subgc.grounding_gt.restatement) against the fixture the reference's own `gt_grd_eval` wrote
(tests/golden/make_golden_grounding_gt.py) byte for byte and `grd_accu` with it, `GtCaptionRows`, and `score_submission`'s exception."""
import ctypes

import numpy as np
import pytest

import grounding_gt_golden as GG
from subgc import _lib, forced
from subgc import grounding_gt as GT
from subgc._lib import SubgcError

NAMES = {
    "subgc_forced_pick": ["logits", "ld", "n", "V", "forced", "ld_f", "Tf", "t", "seq", "seqlp", "T", "next_tok", "unfinished", "n_unfinished",
                          "prev_count", "raw_logits", "stream"],
    "subgc_forced_finish": ["seq", "seqlp", "T", "n", "Tf", "ll", "n_tok", "stream"],
    "subgc_gt_grounding_material": ["node", "T1", "n_words", "rows", "row_img", "box_off", "n_img", "boxes", "n_boxes", "mat_n", "mat_idx", "mat_box",
                                    "ld_m", "stream"],
    "subgc_gt_grounding_score": ["mat_n", "mat_idx", "mat_box", "ld_m", "rows", "pair_cap", "pair_row", "n_pairs", "obj_off", "n_caps", "obj_idx",
                                 "obj_box", "n_obj", "iou_thresh", "out_off", "out", "n_out", "stream"],
}
SETS = ["rnd", "edge", "model"]


@pytest.fixture(scope="module")
def case():
    return GG.load()


def test_forced_header_parses_and_the_other_seven_are_untouched():
    protos = _lib.parse_header(_lib.FORCED_HEADER)
    assert sorted(protos) == sorted(NAMES)
    for name, want in NAMES.items():
        ret, args = protos[name]
        assert ret is ctypes.c_int and [a for _, a in args] == want, name
        assert dict((a, t) for t, a in args)["stream"] is ctypes.c_void_p
    t = dict((a, ty) for ty, a in protos["subgc_forced_pick"][1])
    assert t["ld"] is ctypes.c_int64 and t["ld_f"] is ctypes.c_int64 and t["logits"] is ctypes.c_void_p
    assert all(t[a] is ctypes.c_int for a in ("n", "V", "Tf", "t", "T", "raw_logits"))
    t = dict((a, ty) for ty, a in protos["subgc_forced_finish"][1])
    assert all(t[a] is ctypes.c_int for a in ("T", "n", "Tf")) and t["ll"] is ctypes.c_void_p
    t = dict((a, ty) for ty, a in protos["subgc_gt_grounding_score"][1])
    assert t["iou_thresh"] is ctypes.c_float and all(t[a] is ctypes.c_int for a in ("ld_m", "rows", "n_pairs", "n_caps", "n_obj", "n_out"))
    # the pick's bookkeeping arguments are subgc_decode_pick's, in its order
    core = _lib.parse_header()
    book = ["seq", "seqlp", "T", "next_tok", "unfinished", "n_unfinished", "prev_count", "raw_logits", "stream"]
    assert [a for _, a in core["subgc_decode_pick"][1] if a in book] == [a for a in NAMES["subgc_forced_pick"] if a in book] == book
    src = open(_lib.FORCED_HEADER).read()
    assert "eval_grd_flickr30k_entities.py:63-109" in src and "AttModel.py:295-316" in src and "grd_utils.py:49-60" in src
    assert "bbox_transform.py:194-220" in src and "chunk-then-scan" in src


FAKE = 1 << 20                                                           # never dereferenced: the argument checks come first


def _pick(L, **over):
    a = dict(ld=9488, n=3, V=9488, ld_f=17, Tf=17, t=0, T=17)
    a.update(over)
    return L.subgc_forced_pick(FAKE, a["ld"], a["n"], a["V"], FAKE, a["ld_f"], a["Tf"], a["t"], FAKE, FAKE, a["T"], FAKE, FAKE, None, None, 1, None)


@pytest.mark.parametrize("over,what", [(dict(V=16385, ld=16385), b"at most 16384 columns"), (dict(ld=9000), b"ld >= V"),
                                       (dict(Tf=65, ld_f=65, T=65), b"1 <= Tf <= 64 forced steps (got 65)"),
                                       (dict(t=17), b"step t = 17 is outside the forced rows' 0 .. Tf - 1 = 16"), (dict(t=-1), b"step t = -1"),
                                       (dict(T=16), b"must cover Tf = 17"), (dict(ld_f=16), b"must cover Tf = 17"), (dict(V=0), b"V > 0")])
def test_pick_entry_point_refuses_on_the_host(over, what):
    L = _lib.lib()
    assert _pick(L, **over) == -1
    err = L.subgc_last_error()
    assert b"forced_pick" in err and what in err, err


def test_the_other_entry_points_refuse_on_the_host_and_nothing_to_do_is_ok():
    L = _lib.lib()
    assert _pick(L, n=0) == 0
    assert L.subgc_forced_finish(FAKE, FAKE, 65, 3, 65, FAKE, FAKE, None) == -1 and b"1 <= Tf <= 64" in L.subgc_last_error()
    assert L.subgc_forced_finish(FAKE, FAKE, 10, 3, 11, FAKE, FAKE, None) == -1 and b"1 <= Tf <= T" in L.subgc_last_error()
    assert L.subgc_forced_finish(None, FAKE, 10, 3, 10, FAKE, FAKE, None) == -1 and b"forced_finish: null pointer" in L.subgc_last_error()
    assert L.subgc_forced_finish(None, None, 10, 0, 10, None, None, None) == 0
    rc = L.subgc_gt_grounding_material(FAKE, 17, FAKE, 4, FAKE, FAKE, 2, FAKE, 74, FAKE, FAKE, FAKE, 16, None)
    assert rc == -1 and b"gt_grounding_material: ld_m = 16 is shorter than min(T1, 64) = 17" in L.subgc_last_error()
    rc = L.subgc_gt_grounding_material(FAKE, 17, FAKE, 4, FAKE, FAKE, 0, FAKE, 74, FAKE, FAKE, FAKE, 64, None)
    assert rc == -1 and b"rows without an image" in L.subgc_last_error()
    assert L.subgc_gt_grounding_material(None, 17, None, 0, None, None, 0, None, 0, None, None, None, 64, None) == 0
    rc = L.subgc_gt_grounding_score(FAKE, FAKE, FAKE, 0, 4, FAKE, FAKE, 4, FAKE, 9, FAKE, FAKE, 20, 0.5, FAKE, FAKE, 20, None)
    assert rc == -1 and b"gt_grounding_score: ld_m >= 1 (got 0)" in L.subgc_last_error()
    rc = L.subgc_gt_grounding_score(FAKE, FAKE, FAKE, 64, 4, FAKE, FAKE, 4, FAKE, 0, FAKE, FAKE, 20, 0.5, FAKE, FAKE, 20, None)
    assert rc == -1 and b"pairs without a reference caption" in L.subgc_last_error()
    assert L.subgc_gt_grounding_score(None, None, None, 64, 0, None, None, 0, None, 0, None, None, 0, 0.5, None, None, 0, None) == 0


def test_python_side_refusals(case):
    meta, arr = case
    with pytest.raises(SubgcError, match="token rows of 65 steps; the limit is 64"):
        forced._token_rows([np.ones((2, 65), np.int64)], 1)
    with pytest.raises(SubgcError, match="2 token arrays for 1 images"):
        forced._token_rows([np.ones((2, 5), np.int64)] * 2, 1)
    with pytest.raises(SubgcError, match="integer token rows"):
        forced._token_rows([np.ones((2, 5), np.float32)], 1)
    tok, counts = forced._token_rows([np.ones((2, 5), np.int64), np.full((1, 7), 3, np.int32)], 2)
    assert tok.shape == (3, 7) and counts == [2, 1] and tok[0].tolist() == [1] * 5 + [0, 0] and tok[2].tolist() == [3] * 7
    refs = GG.references(meta, arr, "edge")
    sc = GT.GtGroundingScorer(refs)
    j = refs.index["8002"]
    with pytest.raises(SubgcError, match="not on a device"):
        sc.enqueue_score(None, None, sc.plan([j], [5]))
    long = {"idx_in_sent": list(range(65)), "bbox": [[0, 0, 1, 1]] * 65}
    with pytest.raises(SubgcError, match="a list of 65 entries; the limit is 64"):
        sc.score_lists([(j, [long] * 5)], device="cpu")
    with pytest.raises(SubgcError, match="brings 4 rows and has 5 reference captions"):
        sc.plan([j], [4])
    with pytest.raises(SubgcError, match="names reference image 99"):
        sc.plan([99], [5])
    assert abs(forced.perplexity([-2.0], [2])[0] - np.e) < 1e-15


@pytest.mark.parametrize("tag", SETS)
def test_restatement_reproduces_every_byte_of_the_fixture_and_grd_accu(case, tag):
    meta, arr = case
    refs = GG.references(meta, arr, tag)
    got = GG.restate_submission(refs, GG.results(arr, tag))
    want = GG.expected_entries(meta, arr, tag, refs)
    GG.same_events(got, want)
    s = GT.summarize(got, refs)
    ref_accu = float(arr[tag + "_accu"][0])
    print(tag, "grd_accu", s["grd_accu"], "reference", ref_accu)
    assert s["n_classes"] == meta["sets"][tag]["n_classes"]
    GG.accu_close(s["grd_accu"], ref_accu, s["n_classes"])
    assert {k: [int(sum(v)), len(v)] for k, v in meta["sets"][tag]["per_class"]} == {k: list(v) for k, v in s["per_class"].items()}
    assert [k for k, _ in meta["sets"][tag]["per_class"]] == list(s["per_class"])          # first appearance, the evaluator's order
    counts = [int((np.concatenate([e["events"][:, 1] for e in got]) == c).sum()) for c in range(4)]
    assert counts == meta["sets"][tag]["code_counts"]
    # an image of the split without an entry is "not grounded": dropping the NOROW entries changes nothing
    kept = [e for e in got if not (len(e["events"]) and (e["events"][:, 1] == GT.NOROW).all())]
    assert GT.summarize(kept, refs)["grd_accu"] == s["grd_accu"]


def test_edge_cases_one_by_one(case):
    meta, arr = case
    refs = GG.references(meta, arr, "edge")
    got = {refs.image_ids[e["ref"]]: e["events"][:, 1].tolist() for e in GG.restate_submission(refs, GG.results(arr, "edge"))}
    for name, e in meta["edges"].items():
        if isinstance(e, dict) and "event" in e:
            assert got[str(e["image"])][e["event"]] == e["code"], name
        if isinstance(e, dict) and "codes" in e:
            assert got[str(e["image"])] == e["codes"], name
    assert meta["edges"]["iou_exactly_at_the_threshold"]["code"] == GT.MISS and meta["edges"]["gt_box_w_h_1"]["code"] == GT.MISS
    assert got["8003"] == [] and "8004" not in got and "8999" not in got
    assert GT.iou_f32([0, 0, 9, 4], [0, 0, 9, 9]) == np.float32(0.5) and GT.iou_f32([5, 5, 5, 5], [0, 0, 9, 9]) == -1.0


def test_the_five_predictions_exception_is_the_reference_s(case):
    meta, arr = case
    refs = GG.references(meta, arr, "bad5")
    assert meta["bad5"]["message"] == "Each image must have five caption predictions!"
    with pytest.raises(Exception) as ei:
        GG.restate_submission(refs, GG.results(arr, "bad5"))
    assert type(ei.value) is Exception and str(ei.value) == meta["bad5"]["message"]
    with pytest.raises(Exception) as ei:                                   # raised on the host, before any device work
        GT.GtGroundingScorer(refs).score_submission(GG.results(arr, "bad5"), device="cpu")
    assert type(ei.value) is Exception and str(ei.value) == meta["bad5"]["message"]


def test_gt_caption_rows_alignment_and_truncation():
    ix = {"1": "a", "2": "dog", "3": "runs", "4": "UNK"}
    anns = [{"image_id": 7, "captions": [{"tokens": ["a", "dog", "", "zebra", "runs"]}, {"tokens": ["dog"] * 9}, {"tokens": []}]},
            {"image_id": 8, "captions": [{"tokens": ["a"]}]}, {"image_id": 9, "captions": [{"tokens": ["runs", "a"]}]}]
    rows = GT.GtCaptionRows(anns, [7, "9"], ix, seq_length=6, unk="UNK")
    assert rows.image_ids == ["7", "9"] and rows.index == {"7": 0, "9": 1}
    r = rows[7]
    assert r.shape == (3, 7) and r.dtype == np.int64
    assert r[0].tolist() == [1, 2, 4, 4, 3, 0, 0]                           # position j = annotation word j; empty and unknown -> unk
    assert r[1].tolist() == [2] * 6 + [0]                                   # cut at seq_length; the end token's column stays
    assert r[2].tolist() == [0] * 7
    assert rows.rows_of("9").tolist() == [[3, 1, 0, 0, 0, 0, 0]]
    assert GT.GtCaptionRows(anns, [7], ix, 6, 4)[7].tolist() == r.tolist()  # unk as an id
    with pytest.raises(SubgcError, match="not in the split"):
        rows[8]
    with pytest.raises(SubgcError, match="not in the vocabulary"):
        GT.GtCaptionRows(anns, [7], ix, 6, "nope")
    with pytest.raises(SubgcError, match="seq_length <= 63"):
        GT.GtCaptionRows(anns, [7], ix, 64, 4)


def test_to_submission_round_trips_through_the_restatement(case):
    meta, arr = case
    refs = GG.references(meta, arr, "model")
    res = GG.results(arr, "model")
    entries = []
    for j, img in enumerate(refs.image_ids):
        entries.append({"ref": j, "rows": [{"idx_in_sent": np.asarray(e["idx_in_sent"]), "bbox": np.asarray(e["bbox"], np.float32).reshape(-1, 4)}
                                           for e in res[img]]})
    sub = GT.to_submission(entries, refs)["results"]
    assert sorted(sub) == sorted(res) and all(len(v) == 5 for v in sub.values())
    GG.same_events(GG.restate_submission(refs, sub), GG.expected_entries(meta, arr, "model", refs))
