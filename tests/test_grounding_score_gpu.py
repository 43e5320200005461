"""Grounding scores on the device against the fixture the reference's own evaluator wrote (tests/golden/make_golden_grounding.py):
every event code of the score kernel, the material kernel against `eval_glue.grounding_material` and the reference-written golden, and
`caption_images(..., return_att=1, grounding=...)` end to end on the two `grd` golden models.  Codes, counts, classes, indices and boxes
are exact; the six numbers are within 4 * num_vocab * 2^-53 relative of the reference's (they are equal: `summarize` walks the images in
reference order)."""
import argparse

import numpy as np
import pytest
import torch

import grounding_golden as G
from subgc import grounding, synthetic
from subgc.grounding import SubgcError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def case():
    return G.load()


@pytest.fixture(scope="module")
def cooked(case):
    """tag -> (references on the device, scorer, the fixture's expected entries), cooked once."""
    meta, arr = case
    memo = {}

    def get(tag):
        if tag not in memo:
            refs = G.references(meta, arr, tag, device=DEV)
            memo[tag] = (refs, grounding.GroundingScorer(refs), G.expected_entries(meta, arr, tag, refs))
        return memo[tag]
    return get


def _same_numbers(meta, arr, tag, entries, refs):
    s = grounding.summarize(entries, refs)
    got, want = G.numbers(s), arr[tag + "_numbers"].tolist()
    print(tag, "numbers", got, "reference", want)
    assert s["num_vocab"] == meta["sets"][tag]["num_vocab"]
    G.close(got, want, s["num_vocab"])
    return got


@pytest.mark.parametrize("tag", ["edge", "rnd", "nan", "grd_subgc_0", "grd_subgc_1", "grd_fullgc_0", "grd_fullgc_1"])
def test_score_kernel_writes_the_reference_events(case, cooked, tag):
    meta, arr = case
    refs, sc, want = cooked(tag)
    res = G.grd_results(tag) if tag.startswith("grd_") else G.results(meta, arr, tag)
    got = sc.score_submission(res)                                         # all images in one call, reference order
    G.same_events(got, want)
    n0 = _same_numbers(meta, arr, tag, got, refs)
    for g in got:                                                          # the material rides along unchanged
        e = res[refs.image_ids[g["ref"]]][0]
        assert [refs.class_names[c] for c in g["clss"]] == list(e["clss"]) and g["idx_in_sent"].tolist() == list(e["idx_in_sent"])
        np.testing.assert_array_equal(g["bbox"], np.asarray(e["bbox"], np.float64).reshape(-1, 4).astype(np.float32))
    items = [(g["ref"], res[refs.image_ids[g["ref"]]][0]) for g in got]
    rev = sc.score_entries(items[::-1])                                    # reversed order
    G.same_events(rev[::-1], want)
    one = [sc.score_entries([it])[0] for it in items]                      # one image per call
    G.same_events(one, want)
    for other in (rev, one):
        n = G.numbers(grounding.summarize(other, refs))
        assert all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(n, n0)), (n, n0)
    again = sc.score_submission(res)                                       # equal inputs, equal bits
    for a, b in zip(got, again):
        assert all(np.array_equal(a[k], b[k]) for k in ("precision", "recall", "bbox"))


def test_score_submission_ignores_foreign_images_and_refuses_unknown_classes(case, cooked):
    meta, arr = case
    refs, sc, want = cooked("edge")
    res = G.results(meta, arr, "edge")
    assert str(meta["edges"]["submitted_but_not_annotated"]) in res and str(meta["edges"]["outside_the_split"]) in res
    assert len(sc.score_submission(res)) == len(want) == refs.n_img - 1
    with pytest.raises(SubgcError, match="class word 'zebra' .reference image 0. is not in the cooked class list"):
        sc.score_entries([(0, {"clss": ["zebra"], "idx_in_sent": [0], "bbox": [[0, 0, 1, 1]]})])
    with pytest.raises(SubgcError, match="65 predicted words; the limit is 64"):
        sc.score_entries([(0, {"clss": ["c1"] * 65, "idx_in_sent": list(range(65)), "bbox": [[0, 0, 1, 1]] * 65})])
    with pytest.raises(SubgcError, match="has 2 submission entries"):
        sc.score_submission({"9000": res["9000"] * 2})
    assert sc.score_submission({}) == []


def _host_material(rows, pick, node, n_words, boxes, wh, rbe, det_wd):
    """eval_glue.grounding_material on the prediction entry these token rows would have made."""
    from subgc import eval_glue
    entry = {"caption": eval_glue.decode_sequence(G.VOCAB, rows, rbe), "grounding": {"subg_index": pick, "node_ind": node[:n_words]}}
    return eval_glue.grounding_material(entry, boxes, G.WD_TO_LEMMA, G.LEMMA_DET, det_wd, img_wh=wh)


def _material_batch():
    """Token rows with every case of the word rule: an empty caption, a 64-word caption, trailing bad endings (one of them a class word), a
    caption of bad endings only, words without a lemma or a class, a second-ranked pick, an image without rows, an image without boxes."""
    rng = np.random.default_rng(11)
    T = 64
    imgs = [[[]], [[(q % 12) + 1 for q in range(64)]], [[1, 16, 2, 15, 13, 14]], [[15, 15]], [[3, 18, 17, 4]], [[5, 6], [7, 8, 9, 15]], [],
            [[10, 11]], [[12, 13, 1, 15]]]
    pick = [0, 0, 0, 0, 0, 1, 0, 0, 0]
    n_box = [3, 36, 5, 1, 4, 7, 2, 0, 6]
    bounds = np.concatenate([[0], np.cumsum([len(i) for i in imgs])]).tolist()
    seq = np.zeros((bounds[-1], T), np.int64)
    for r, row in enumerate(r for i in imgs for r in i):
        seq[r, :len(row)] = row
    boxes = [rng.random((n, 4)) * 500 for n in n_box]
    boxes[2] = boxes[2].astype(np.float32)                                  # an array of its own dtype
    wh = [(int(rng.integers(300, 900)), int(rng.integers(300, 900))) for _ in imgs]
    wh[4] = None
    return imgs, pick, bounds, seq, boxes, wh


@pytest.mark.parametrize("rbe", [0, 1])
@pytest.mark.parametrize("tok64", [False, True])
def test_material_kernel_equals_the_host_function(case, cooked, rbe, tok64):
    from subgc import ops
    meta, arr = case
    refs, sc, _ = cooked("rnd")
    det_wd = {int(k): v for k, v in meta["det_id_to_det_wd"].items()}
    imgs, pick, bounds, seq, boxes, wh = _material_batch()
    I, T1 = len(imgs), 65
    rng = np.random.default_rng(5)
    n_words = np.array([(len(i[p]) if i else 0) for i, p in zip(imgs, pick)], np.int32)
    node = np.full((I, T1), -1, np.int32)
    for i in range(I):
        node[i, :n_words[i]] = rng.integers(0, max(len(boxes[i]), 1), size=n_words[i])
    prep = [grounding.prepare_boxes(b, w) for b, w in zip(boxes, wh)]
    box_off = np.concatenate([[0], np.cumsum([len(b) for b in prep])]).astype(np.int32)
    plan = sc.plan([0] * I)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    arena = torch.full((sc.arena_words(plan),), 0x3fffffff, dtype=torch.int32, device=DEV)
    sc.enqueue_material(d(seq, torch.int64 if tok64 else torch.int32), d(bounds, torch.int32), d(pick, torch.int32), I, d(node, torch.int32), T1,
                        d(n_words, torch.int32), d(box_off, torch.int32), d(np.concatenate(prep), torch.float32), int(box_off[-1]), rbe, arena, plan)
    mat_n, cls, idx, box, _, _ = sc.views(arena.cpu().numpy(), plan)
    counts = []
    for i in range(I):
        n = int(mat_n[i])
        counts.append(n)
        if not imgs[i]:
            assert n == 0
            continue
        if len(boxes[i]) == 0:                                              # no boxes: the host function would raise; the device writes zeros
            assert n == 2 and (box[i, :n] == 0).all()
            continue
        want = _host_material(seq[bounds[i]:bounds[i + 1]], pick[i], node[i], int(n_words[i]), boxes[i], wh[i], rbe, det_wd)
        assert [refs.class_names[c] for c in cls[i, :n]] == want["clss"], i
        assert idx[i, :n].tolist() == want["idx_in_sent"], i
        np.testing.assert_array_equal(box[i, :n], np.asarray(want["bbox"], np.float64).reshape(-1, 4).astype(np.float32), err_msg=str(i))
    # empty, 64 words, bad endings trimmed (the class word "with" among them) or not, bad endings only, unknown ids, the picked row
    assert counts == ([0, 64, 2, 2, 2, 3, 0, 2, 2] if rbe else [0, 64, 3, 2, 2, 4, 0, 2, 3])
    # the same lists straight from the pick-less launch: row 0 of every image
    arena2 = torch.full_like(arena, 0x3fffffff)
    sc.enqueue_material(d(seq, torch.int64 if tok64 else torch.int32), d(bounds, torch.int32), None, I, d(node, torch.int32), T1,
                        d(n_words, torch.int32), d(box_off, torch.int32), d(np.concatenate(prep), torch.float32), int(box_off[-1]), rbe, arena2, plan)
    m2 = sc.views(arena2.cpu().numpy(), plan)[0]
    assert m2[5] == 2 and m2[1] == 64


def _grd_case(golden, name):
    g = golden("grd")
    meta = g.meta
    opt = dict(meta["opt"][name])
    opt.setdefault("obj_name_path", None); opt.setdefault("rel_name_path", None)
    w = golden("subgc_beam").group("weights") if name == "subgc" else golden("fullgc_train").group("weights")
    if name == "subgc":
        w["logit.bias"][0] += 0.5
    det_wd = {int(k): v for k, v in meta["det_id_to_det_wd"].items()}
    return g.group("out"), meta, argparse.Namespace(**opt), w, det_wd


@pytest.mark.parametrize("name", ["subgc", "fullgc"])
def test_caption_images_scores_grounding_in_the_decode_pass(golden, case, cooked, name):
    import subgc.models as models
    from subgc import eval_glue
    fmeta, arr = case
    out, meta, opt, w, det_wd = _grd_case(golden, name)
    opt.caption_model = "topdown"
    m = models.setup(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = m.to(DEV).eval()
    imgs = meta["cases"][name]
    cpu = [synthetic.make_test_batch(i["M"], D=opt.att_feat_size, seed=i["seed"], fc_size=opt.att_feat_size, node_pool=i["pool"]) for i in imgs]
    dev = [{k: v.to(DEV) for k, v in b.items()} for b in cpu]
    infos = [{"id": i["id"]} for i in imgs]
    kw = dict(sample_max=1, beam_size=1, return_att=1)
    for consensus in (0, 1):
        tag = f"grd_{name}_{consensus}"
        refs, sc, want = cooked(tag)
        arg = {"scorer": sc, "index": {i["id"]: refs.index[str(i["id"])] for i in imgs}, "boxes": {i["id"]: out[f"{name}_{i['id']}_boxes"] for i in imgs},
               "img_wh": {i["id"]: i["wh"] for i in imgs}}
        pick = [i["pick"] for i in imgs] if consensus else None
        plain = eval_glue.caption_images(m, dev, infos, meta["vocab"], kw, grd_pick=pick)
        preds = eval_glue.caption_images(m, dev, infos, meta["vocab"], kw, grd_pick=pick, grounding=arg)
        for p0, p1, img in zip(plain, preds, imgs):
            assert sorted(p1) == sorted(list(p0) + ["grounding_score"])
            for key in p0:                                                  # every other key is what it is without grounding=
                if key == "grounding":
                    assert sorted(p0[key]) == sorted(p1[key]) and all(np.array_equal(p0[key][k], p1[key][k]) for k in p0[key])
                else:
                    assert np.array_equal(np.asarray(p0[key]), np.asarray(p1[key])), key
            g = p1["grounding_score"]
            host = eval_glue.grounding_material(p1, out[f"{name}_{img['id']}_boxes"], meta["wd_to_lemma"], meta["lemma_det_id_dict"], det_wd,
                                                img_wh=img["wh"])
            t = f"{name}_{img['id']}_{consensus}"
            for ref_list in (host, {"clss": [str(c) for c in out[t + "_clss"]], "idx_in_sent": out[t + "_idx_in_sent"].tolist(),
                                    "bbox": out[t + "_bbox"].tolist()}):
                assert [refs.class_names[c] for c in g["clss"]] == list(ref_list["clss"]), t
                assert g["idx_in_sent"].tolist() == list(ref_list["idx_in_sent"]), t
                np.testing.assert_array_equal(g["bbox"], np.asarray(ref_list["bbox"], np.float64).reshape(-1, 4).astype(np.float32), err_msg=t)
        entries = [p["grounding_score"] for p in preds]
        G.same_events(entries, want)
        n0 = _same_numbers(fmeta, arr, tag, entries, refs)
        if consensus == 0:                                                  # one image per decode batch: the same entries
            single = eval_glue.caption_images(m, dev, infos, meta["vocab"], kw, group=1, grounding=arg)
            G.same_events([p["grounding_score"] for p in single], want)
            assert G.numbers(grounding.summarize([p["grounding_score"] for p in single][::-1], refs))[:2] == n0[:2]
    with pytest.raises(ValueError, match="return_att"):
        eval_glue.caption_images(m, dev, infos, meta["vocab"], dict(sample_max=1, beam_size=1), grounding=arg)
    with pytest.raises(ValueError, match="sct"):
        eval_glue.caption_images(m, dev, infos, meta["vocab"], dict(kw, sct=1), grounding=arg)
    with pytest.raises(ValueError, match="no reference image or no boxes for image ids"):
        eval_glue.caption_images(m, dev, infos, meta["vocab"], kw, grounding=dict(arg, index={}))


def _collect(sc, refs, sizes, N, rng, rbe=0, pick=None):
    """ops.eval_collect on a fabricated decode batch with grounding=; -> (its output, per image boxes, the reference-image indices)."""
    from subgc import ops
    T, T1 = 20, 21
    I = len(sizes)
    bounds = [0] + np.cumsum(sizes).astype(int).tolist()
    rows = bounds[-1]
    AL = rng.random((T1, max(rows, 1), N)).astype(np.float32)               # (a batch without rows keeps one spare row: unit strides)
    seq = rng.integers(1, 19, size=(rows, T))
    for r in range(rows):
        seq[r, rng.integers(0, T + 1):] = 0
    score = rng.random(rows).astype(np.float32)
    keep = rng.integers(0, 1000, size=rows)
    idx = np.stack([np.sort(rng.permutation(N)) for _ in range(max(rows, 1))])
    boxes = [grounding.prepare_boxes(rng.random((N, 4)) * 300, (640, 480)) for _ in range(I)]
    index = [int(x) for x in rng.integers(0, refs.n_img, size=I)]
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    h = ops.eval_collect(d(score, torch.float32), d(keep, torch.int64), d(seq, torch.int64), bounds, AL=d(AL, torch.float32), idx=d(idx, torch.int64),
                         pick=pick, grounding={"scorer": sc, "index": index, "boxes": boxes, "remove_bad_endings": rbe})
    plain = ops.eval_collect(d(score, torch.float32), d(keep, torch.int64), d(seq, torch.int64), bounds, AL=d(AL, torch.float32), idx=d(idx, torch.int64),
                             pick=pick)
    for k in plain:                                                         # nothing else changes
        np.testing.assert_array_equal(plain[k], h[k], err_msg=k)
    assert sorted(set(h) - set(plain)) == ["g_plan", "g_words"]
    return h, bounds, boxes, index


@pytest.mark.parametrize("sizes,pick", [([], None), ([4], None), ([3, 0, 10, 1, 0, 7, 2], None), ([3, 0, 10, 1, 0, 7, 2], [2, 0, 9, 0, 0, 3, 1])])
def test_eval_collect_batch_extremes(case, cooked, sizes, pick):
    """Zero images, one image and a mixed batch with images that have no rows: the in-pass lists equal the host function on the pass's own
    outputs, and the in-pass events equal the score kernel fed those lists on its own (which the fixture pins).  An image without rows
    gets `empty_entry`, which is also what caption_images hands out for a decode batch without any row (it makes no launch then)."""
    from subgc import eval_glue
    meta, arr = case
    refs, sc, _ = cooked("rnd")
    det_wd = {int(k): v for k, v in meta["det_id_to_det_wd"].items()}
    for rbe in (0, 1):
        h, bounds, boxes, index = _collect(sc, refs, sizes, 12, np.random.default_rng(100 + len(sizes)), rbe, pick)
        got = sc.unpack(h["g_words"], h["g_plan"])
        assert len(got) == len(sizes)
        items = []
        for i, g in enumerate(got):
            assert g["ref"] == index[i]
            if sizes[i] == 0:
                e = sc.empty_entry(index[i])
                assert all(np.array_equal(g[k], e[k]) for k in e), i
                items.append((index[i], {"clss": [], "idx_in_sent": [], "bbox": []}))
                continue
            sub = 0 if pick is None else pick[i]
            w = int(h["n_words"][i])
            entry = {"caption": eval_glue.decode_sequence(G.VOCAB, h["seq"][bounds[i]:bounds[i + 1]], rbe),
                     "grounding": {"subg_index": sub, "node_ind": h["node"][i, :w]}}
            want = eval_glue.grounding_material(entry, boxes[i], G.WD_TO_LEMMA, G.LEMMA_DET, det_wd)
            assert [refs.class_names[c] for c in g["clss"]] == want["clss"] and g["idx_in_sent"].tolist() == want["idx_in_sent"], i
            np.testing.assert_array_equal(g["bbox"], np.asarray(want["bbox"], np.float32).reshape(-1, 4))
            items.append((index[i], want))
        G.same_events(got, sc.score_entries(items))


def test_debug_bounds_reports_instead_of_reading(case, cooked):
    from subgc import ops
    meta, arr = case
    refs, sc, _ = cooked("edge")
    res = G.results(meta, arr, "edge")
    items = [(refs.index[k], res[k][0]) for k in ("9000", "9001", "9002")]
    plan = sc.plan([j for j, _ in items], [len(e["clss"]) for _, e in items])
    I, P = plan["I"], plan["P"]
    arena = torch.zeros(sc.arena_words(plan), dtype=torch.int32, device=DEV)
    good = torch.from_numpy(plan["table"]).to(DEV)
    with ops.debug_bounds():
        sc.enqueue_score(good, arena, plan)                                 # the clean tables pass
        bad = plan["table"].copy()
        bad[1] = refs.n_img + 5                                             # img_ref of batch image 1
        with pytest.raises(SubgcError, match="img_ref"):
            sc.enqueue_score(torch.from_numpy(bad).to(DEV), arena, plan)
        bad = plan["table"].copy()
        bad[I + 1] = bad[I + 2] + 1                                         # pair_off goes down
        with pytest.raises(SubgcError, match="pair_off .pairs of the batch images. is not monotone inside .0, 3."):
            sc.enqueue_score(torch.from_numpy(bad).to(DEV), arena, plan)
        bad = plan["table"].copy()
        bad[2 * I + 1 + P + 1 + 1] = 10 ** 6                                # rec_off leaves its buffer
        with pytest.raises(SubgcError, match="rec_off .recall event offsets. is not monotone"):
            sc.enqueue_score(torch.from_numpy(bad).to(DEV), arena, plan)
        d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
        seq, node = np.ones((3, 4), np.int64), np.zeros((3, 5), np.int32)
        with pytest.raises(SubgcError, match="box_off .box rows of the images. is not monotone"):
            sc.enqueue_material(d(seq, torch.int64), d([0, 1, 2, 3], torch.int32), None, 3, d(node, torch.int32), 5, d([4, 4, 4], torch.int32),
                                d([0, 2, 1, 3], torch.int32), d(np.zeros((3, 4)), torch.float32), 3, 0, arena, plan)
        node[1, 2] = 7
        with pytest.raises(SubgcError, match="node"):
            sc.enqueue_material(d(seq, torch.int64), d([0, 1, 2, 3], torch.int32), None, 3, d(node, torch.int32), 5, d([4, 4, 4], torch.int32),
                                d([0, 1, 2, 3], torch.int32), d(np.zeros((3, 4)), torch.float32), 3, 0, arena, plan)
    torch.cuda.synchronize()
