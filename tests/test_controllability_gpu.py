"""Controllability scores on the device against the fixture the reference's own NounIoU and COCO scorers wrote
(tests/golden/make_golden_controllability.py).  The assignment is checked for what it is -- a valid partial matching whose value is
scipy's optimum on the same fp32 matrix up to fp64 summation rounding -- and the arithmetic around it bit for bit against the numpy
restatement of the header's contract, evaluated on the device's own assignment.  Against the reference the values lie within the bounds
derived in DESIGN 4.K (controllability_golden.pair_bound / row_bound); every test prints the worst difference it saw before it asserts.
"""
import numpy as np
import pytest
import torch

import accuracy_golden as A
import controllability_golden as G
from subgc import controllability as C
from subgc.controllability import SubgcError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7f7f7f7f                                    # int8 127 (no word), a float no score can be, an m / n no caption has


@pytest.fixture(scope="module")
def case():
    return G.load()


@pytest.fixture(scope="module")
def scored(case):
    """tag -> (references on the device, scorer, the per-row entries of one `score` call, the host pairs), computed once."""
    meta, arr = case
    memo = {}

    def get(tag, tok64=False):
        if (tag, tok64) not in memo:
            refs = memo[(tag, not tok64)][0] if (tag, not tok64) in memo else G.cook(meta, arr, tag, device=DEV)
            sc = C.ControlScorer(refs)
            seq = torch.from_numpy(arr[tag + "_seq"].astype(np.int64 if tok64 else np.int32)).to(DEV)
            entries = sc.score(seq, arr[tag + "_row_group"].tolist(), remove_bad_endings=meta["sets"][tag]["remove_bad_endings"])
            memo[(tag, tok64)] = (refs, sc, entries, G.pairs_of(refs, arr, tag, meta))
        return memo[(tag, tok64)]
    return get


def _flat(entries, key):
    return np.concatenate([np.asarray(e[key]).reshape((-1,) + np.asarray(e[key]).shape[1:]) for e in entries])


@pytest.mark.parametrize("tag", G.SETS)
def test_structure_is_exact(case, scored, tag):
    meta, arr = case
    refs, sc, entries, pairs = scored(tag)
    mn, assign = _flat(entries, "pair_mn"), _flat(entries, "assign")
    np.testing.assert_array_equal(mn, arr[tag + "_pair_mn"])
    assert assign.shape == (len(pairs), 64) and assign.dtype == np.int8
    for p, (m, n) in enumerate(mn):
        a = assign[p]
        used = a[a >= 0]
        assert len(used) == min(m, n) and len(set(used.tolist())) == len(used), p      # exactly min(m, n) matched, no column twice
        assert (used < n).all() and (a[m:] == -1).all(), p                              # inside the predicted words; -1 beyond m
    for e, g in zip(entries, arr[tag + "_row_group"]):
        assert e["group"] == g and len(e["pair_iou"]) == (0 if g < 0 else refs.gcap_off[g + 1] - refs.gcap_off[g])
        if g < 0:
            assert e["noun_iou"] == 0 and e["accuracy"] is None


@pytest.mark.parametrize("tag,tok64", [("exact", False), ("edge", False), ("edge", True), ("edge_rbe", False), ("edge_rbe", True), ("edge_d1", False)])
def test_assignment_is_optimal_and_the_arithmetic_is_bit_exact(case, scored, tag, tok64):
    meta, arr = case
    refs, sc, entries, pairs = scored(tag, tok64)
    nv = refs.nouns
    assign, pair_iou = _flat(entries, "assign"), _flat(entries, "pair_iou")
    assert meta["excused_from_bit_exactness"] == []                                     # no entry needed the platform excuse
    checked = 0
    for p, (r, gt, pw) in enumerate(pairs):                                             # no pair is skipped
        S = G.matrix(nv.vec, nv.norm, gt, pw)
        m, n = S.shape
        a = assign[p, :m].astype(np.int64)
        if m and n:
            got = float(S.astype(np.float64)[np.flatnonzero(a >= 0), a[a >= 0]].sum())
            best = G.scipy_assign(S)[1]
            assert got >= best - min(m, n) ** 2 * 2.0 ** -53, (p, m, n, got, best)
        want = G.pair_value(S, a)
        assert pair_iou[p].tobytes() == want.tobytes(), (p, m, n, pair_iou[p], want)
        checked += 1
    assert checked == meta["sets"][tag]["pairs"]
    for e in entries:
        assert np.float32(e["noun_iou"]).tobytes() == G.row_value(e["pair_iou"]).tobytes()
    if tok64:                                                                           # the token width changes nothing
        other = scored(tag, False)[2]
        for e, o in zip(entries, other):
            assert e["assign"].tobytes() == o["assign"].tobytes() and e["pair_iou"].tobytes() == o["pair_iou"].tobytes()


@pytest.mark.parametrize("tag", G.SETS)
def test_values_lie_within_the_derived_bounds_of_the_reference(case, scored, tag):
    meta, arr = case
    refs, sc, entries, pairs = scored(tag)
    d = refs.nouns.d
    pair_iou, mn = _flat(entries, "pair_iou"), _flat(entries, "pair_mn")
    diff = np.abs(pair_iou.astype(np.float64) - arr[tag + "_pair_iou"])
    bound = np.array([G.pair_bound(d, m, n) for m, n in mn])
    rows = [(abs(float(e["noun_iou"]) - arr[tag + "_row_iou"][r]), G.row_bound(d, e["pair_mn"])) for r, e in enumerate(entries) if e["group"] >= 0]
    print(tag, "worst pair difference", diff.max(), "bound", bound.max(), "worst row difference", max(x for x, _ in rows), "bound", max(b for _, b in rows))
    assert (diff <= bound).all(), (diff.max(), np.argmax(diff - bound))
    assert all(x <= b for x, b in rows)
    s = C.summarize(entries)
    assert abs(float(s["Noun_IoU"]) - float(arr[tag + "_corpus_iou"])) <= max(b for _, b in rows) + (len(rows) + 2) * G.U


@pytest.mark.parametrize("tag", G.SETS)
def test_bleu_rouge_cider_of_the_groups(case, scored, tag):
    meta, arr = case
    refs, sc, entries, _ = scored(tag)
    got = [e["accuracy"] for e in entries if e["group"] >= 0]
    worst = A.compare(got, G.accuracy_entries(arr, tag))                                # material and picks ==
    print(tag, "worst relative differences (BLEU, CIDEr, ROUGE-L)", worst)
    assert worst[0] <= A.BLEU_TOL and worst[1] <= A.CIDER_TOL and worst[2] <= A.ROUGE_TOL
    s, want = C.summarize(entries), arr[tag + "_acc_corpus"]
    assert A.rel([s[f"Bleu_{k}"] for k in range(1, 5)], want[:4]) <= A.BLEU_TOL
    assert A.rel([s["CIDEr"]], [want[4]]) <= A.CIDER_TOL and A.rel([s["ROUGE_L"]], [want[5]]) <= A.ROUGE_TOL


@pytest.mark.parametrize("tag", ["rnd", "edge"])
def test_two_runs_give_equal_bits(case, scored, tag):
    meta, arr = case
    refs, sc, entries, _ = scored(tag)
    seq = torch.from_numpy(arr[tag + "_seq"].astype(np.int32)).to(DEV)
    again = sc.score(seq, arr[tag + "_row_group"].tolist(), remove_bad_endings=meta["sets"][tag]["remove_bad_endings"])
    for a, b in zip(entries, again):
        for key in ("pair_iou", "pair_mn", "assign"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert np.float32(a["noun_iou"]).tobytes() == np.float32(b["noun_iou"]).tobytes()
        if a["accuracy"] is not None:
            assert a["accuracy"]["values"].tobytes() == b["accuracy"]["values"].tobytes()


def _launch(sc, arr, tag, meta, arena=None, table=None, slack=0):
    from subgc import ops
    plan = sc.plan(arr[tag + "_row_group"].tolist())
    rows = plan["rows"]
    seq = torch.from_numpy(arr[tag + "_seq"].astype(np.int32)).to(DEV)
    if table is None:
        table = np.concatenate([plan["idx"], plan["pair_off"]]).astype(np.int32)
    if arena is None:
        arena = torch.full((sc.arena_words(plan) + slack,), SENTINEL, dtype=torch.int32, device=DEV)
    sc.enqueue_noun_iou(seq, torch.from_numpy(table).to(DEV), meta["sets"][tag]["remove_bad_endings"], arena, plan)
    return plan, arena


@pytest.mark.parametrize("tag", ["edge", "rnd"])
def test_poisoned_buffers_every_owned_slot_is_written_and_nothing_else(case, scored, tag):
    meta, arr = case
    refs, sc, entries, _ = scored(tag)
    slack = 64
    plan, arena = _launch(sc, arr, tag, meta, slack=slack)
    host = arena.cpu().numpy()
    words = sc.arena_words(plan)
    acc, iou, pair, mn, ass = sc.views(host[:words], plan)
    assert (acc == SENTINEL).all()                                                      # the accuracy records belong to other launches
    assert (host[words:] == SENTINEL).all() and len(host) == words + slack              # nothing past the last pair
    sent_f = np.array([SENTINEL], np.int32).view(np.float32)[0]
    assert not (iou == sent_f).any() and not (pair == sent_f).any() and not (mn == SENTINEL).any() and not (ass == 127).any()
    np.testing.assert_array_equal(pair, _flat(entries, "pair_iou"))
    np.testing.assert_array_equal(ass, _flat(entries, "assign"))
    np.testing.assert_array_equal(iou, np.array([e["noun_iou"] for e in entries], np.float32))
    # fewer rows than the buffers hold: the rows and pairs behind them stay untouched
    k = plan["rows"] // 2
    sub = sc.plan(arr[tag + "_row_group"][:k].tolist())
    arena2 = torch.full((sc.arena_words(sub) + slack,), SENTINEL, dtype=torch.int32, device=DEV)
    seq = torch.from_numpy(arr[tag + "_seq"][:k].astype(np.int32)).to(DEV)
    sc.enqueue_noun_iou(seq, torch.from_numpy(np.concatenate([sub["idx"], sub["pair_off"]]).astype(np.int32)).to(DEV),
                        meta["sets"][tag]["remove_bad_endings"], arena2, sub)
    host2 = arena2.cpu().numpy()
    assert (host2[sc.arena_words(sub):] == SENTINEL).all()
    np.testing.assert_array_equal(sc.views(host2[:sc.arena_words(sub)], sub)[2], pair[:sub["P"]])


def test_debug_bounds_reports_instead_of_reading(case, scored):
    from subgc import ops
    meta, arr = case
    refs, sc, _, _ = scored("edge")
    plan = sc.plan(arr["edge_row_group"].tolist())
    rows = plan["rows"]
    good = np.concatenate([plan["idx"], plan["pair_off"]]).astype(np.int32)
    with ops.debug_bounds():
        _launch(sc, arr, "edge", meta)                                                  # the clean tables pass (the -1 row included)
        bad = good.copy()
        bad[2] = refs.n_groups + 5
        with pytest.raises(SubgcError, match="row_group"):
            _launch(sc, arr, "edge", meta, table=bad)
        bad = good.copy()
        bad[rows + 3] = bad[rows + 4] + 1                                               # pair_off goes down
        with pytest.raises(SubgcError, match=r"pair_off .pairs of the rows. is not monotone inside .0, %d." % plan["P"]):
            _launch(sc, arr, "edge", meta, table=bad)
        keep = refs.d_gn
        try:
            gn = refs.gn.copy()
            gn[5] = refs.nouns.n_noun
            refs.d_gn = torch.from_numpy(gn).to(DEV)
            with pytest.raises(SubgcError, match="gn .vector rows of the ground-truth words."):
                _launch(sc, arr, "edge", meta)
        finally:
            refs.d_gn = keep
        _launch(sc, arr, "edge", meta)
    torch.cuda.synchronize()


def test_score_predictions_is_the_drop_in_and_prints_the_script_lines(case, scored, capsys):
    meta, arr = case
    tag = "sct_subgc"
    refs, sc, entries, _ = scored(tag)
    voc = G.vocab(meta)
    from subgc import eval_glue
    caps = eval_glue.decode_sequence(voc, arr[tag + "_seq"].astype(np.int64).tolist(), 0)
    # three images holding 1, 3 and 2 region sets, listed out of order: order_list puts them back
    preds = [{"image_id": 12, "caption": caps[1:4]}, {"image_id": 11, "caption": caps[0:1]}, {"image_id": 13, "caption": caps[4:6]}]
    s, got = C.score_predictions(preds, ["11", "12", "13"], refs, voc)
    out = capsys.readouterr().out
    for a, b in zip(got, entries):
        assert a["pair_iou"].tobytes() == b["pair_iou"].tobytes() and a["assign"].tobytes() == b["assign"].tobytes()
        assert a["accuracy"]["values"].tobytes() == b["accuracy"]["values"].tobytes()
    assert s["Noun_IoU"] == C.summarize(entries)["Noun_IoU"]
    assert "totally 3 images in the test set" in out and "Blue_1 " in out and "Bleu_2 " in out and "ROUGE_L " in out and "CIDEr " in out
    assert "Noun IoU %s" % s["Noun_IoU"] in out and "METEOR" not in out and "SPICE" not in out
    with pytest.raises(ValueError, match="4 generated captions, the references hold 6 groups"):
        C.score_predictions(preds[:2], ["11", "12"], refs, voc, verbose=False)


def test_caption_images_scores_the_sct_decode(golden, case):
    import inspect
    from subgc import eval_glue, synthetic
    from test_parity_gpu import build
    meta, arr = case
    g = golden("subgc_sct")
    m = build(g, golden("subgc_beam").group("weights"), False)
    assert m.sct
    o = g.meta["opt"]
    images = [{k: v.to(DEV) for k, v in g.tensors("inputs").items()}]
    for i, M in enumerate((4, 9)):
        b = synthetic.make_test_batch(M, D=o["att_feat_size"], seed=70 + i, fc_size=o["fc_feat_size"])
        images.append({k: v.to(DEV) for k, v in b.items()})
    infos = [{"id": 500 + i} for i in range(len(images))]
    voc = G.vocab(meta)
    kw = dict(sample_max=1, beam_size=1, sct=1, remove_bad_endings=1)
    assert inspect.signature(eval_glue.caption_images).parameters["controllability"].default is None     # off by default
    plain = eval_glue.caption_images(m, images, infos, voc, kw)
    counts = [len(p["caption"]) for p in plain]
    assert counts[0] == 6 and min(counts) >= 1
    # fabricated groups for every kept row (the fixture's, cycled) over the fixture's vectors
    pool = G.groups(meta, arr, "sct_subgc") + G.groups(meta, arr, "rnd")
    gt = [pool[i % len(pool)] for i in range(sum(counts))]
    nouns = C.NounVectors(G.vectors(meta, arr, "sct_subgc"), voc, device=None)
    refs = C.ControlReferences(gt, nouns, voc, device=DEV)
    sc = C.ControlScorer(refs)
    firsts = np.concatenate([[0], np.cumsum(counts)]).tolist()
    arg = {"scorer": sc, "index": {info["id"]: firsts[i] for i, info in enumerate(infos)}}
    preds = eval_glue.caption_images(m, images, infos, voc, kw, controllability=arg)
    for p0, p1 in zip(plain, preds):
        assert set(p1) - set(p0) == {"controllability"}
        for key, v in p0.items():                                           # omitting the argument changes nothing that was there
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(p1[key], v)
            else:
                assert p1[key] == v
    # the strings are already trimmed: scoring them stand-alone, without trimming, is the same computation
    _, alone = C.score_predictions(preds, [info["id"] for info in infos], refs, voc, verbose=False)
    flat = [e for p in preds for e in p["controllability"]]
    assert len(flat) == len(alone) == sum(counts) and [e["group"] for e in flat] == list(range(sum(counts)))

    def same(a, b):
        for key in ("pair_iou", "pair_mn", "assign"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert np.float32(a["noun_iou"]).tobytes() == np.float32(b["noun_iou"]).tobytes() and a["group"] == b["group"]
        np.testing.assert_array_equal(a["accuracy"]["material"], b["accuracy"]["material"])
        assert a["accuracy"]["values"].tobytes() == b["accuracy"]["values"].tobytes()
    for a, b in zip(flat, alone):
        same(a, b)
    assert max(float(e["noun_iou"]) for e in flat) > 0                      # the check is not about zeros
    for group in (1, 2):                                                    # the chunk an image falls into cannot change its entries
        split = eval_glue.caption_images(m, images, infos, voc, kw, group=group, controllability=arg)
        for a, b in zip(flat, [e for p in split for e in p["controllability"]]):
            same(a, b)
    s = C.summarize(flat)
    assert s["rows"] == sum(counts) and 0 <= float(s["Noun_IoU"]) <= 1
    with pytest.raises(ValueError, match="only in sct"):
        eval_glue.caption_images(m, images, infos, voc, dict(kw, sct=0), controllability=arg)
    with pytest.raises(ValueError, match=r"no first group for image ids \[502\]"):
        eval_glue.caption_images(m, images, infos, voc, kw, controllability={"scorer": sc, "index": {500: 0, 501: firsts[1]}})
    with pytest.raises(ValueError, match="image 500 has 6 kept rows and 5 ground-truth groups"):
        eval_glue.caption_images(m, images, infos, voc, kw, controllability={"scorer": sc, "index": {500: 0, 501: 5, 502: firsts[2]}})
