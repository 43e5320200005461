"""Controlled captioning from region boxes on the device (subgc.control_input, include/subgc_control_input_hip.h) against the arrays the
reference's own loaders returned (tests/golden/make_golden_sct_loader.py): every index array, mask, pool matrix, match index and status
exactly and the IoUs bit for bit; one launch chain against image by image; the plain test loader; poisoned outputs; and, with the golden
`sct` model of tests/test_eval_glue.py, the captions and scores of the assembled items against those of the reference-built items."""
import numpy as np
import pytest
import torch

import sct_loader_golden as G
from subgc import control_input as CI

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = {"greedy37": ("g0", "g1", "g2", "g4"), "greedy65": ("g3",), "gt": ("t0", "t1")}


@pytest.fixture(scope="module")
def case():
    return G.load()


def _assemble(meta, arr, tags, only_ok=True, **kw):
    raw, sets, off, wh, gt = G.raw_batch(meta, arr, tags, DEV, only_ok=only_ok, **kw)
    info = meta["images"][tags[0]]
    items, table = CI.assemble_sct_batch(raw, sets, off, wh, info["obj_num"], info["rel_num"], mode=info["mode"], gt=gt)
    return items, table, off


def _check_item(item, want, tag):
    for k in G.ROWS + G.GRAPH:
        got = item[k].cpu().numpy()
        w = want[k]
        if k == "obj_dist" and got.shape[-1] != w.shape[-1]:                                 # the batch's one class width: zero columns behind
            assert not got[..., w.shape[-1]:].any(), (tag, k)
            got = got[..., :w.shape[-1]]
        assert got.shape == w.shape and got.dtype == w.dtype, (tag, k, got.shape, w.shape, got.dtype, w.dtype)
        assert got.tobytes() == np.ascontiguousarray(w).tobytes(), (tag, k)
    assert item["this_mini_batch"] == int(want["this_mini_batch"][0])


@pytest.mark.parametrize("name", list(BATCHES))
def test_device_items_equal_the_reference_loader(case, name):
    meta, arr = case
    tags = BATCHES[name]
    items, table, off = _assemble(meta, arr, tags)
    assert not table["status"].any()
    for b, tag in enumerate(tags):
        _check_item(items[b], G.expected(meta, arr, tag), tag)
        seed, idx, iou, _ = CI.restate_match(arr[f"{tag}_boxes"], meta["images"][tag]["wh"], G.sets_of(meta, arr, tag, only_ok=True))
        a, e = off[b], off[b + 1]
        assert (table["seed_mask"][a:e] == seed).all() and (table["idx"][a:e] == idx).all(), tag
        assert table["iou"][a:e].tobytes() == iou.tobytes(), tag                             # bit for bit (the CPU test pins `iou` on the reference's log)


@pytest.mark.parametrize("name", ["greedy37", "gt"])
def test_status_rows_of_sets_the_reference_cannot_process(case, name):
    """Low level: the status array and padding rows of the bad sets; high level: the error names the image id and the set."""
    meta, arr = case
    tags = BATCHES[name]
    raw, sets, off, wh, gt = G.raw_batch(meta, arr, tags, DEV)
    d_off = torch.tensor(off, dtype=torch.int64, device=DEV)
    seed, idx, iou, status = CI.match_regions(raw["boxes"], torch.tensor(wh, dtype=torch.float32, device=DEV), sets, d_off)
    want = []
    for tag in tags:
        want += [(CI.NO_OVERLAP if name == "greedy37" else CI.NO_GT) if i in meta["images"][tag]["bad_sets"] else CI.OK
                 for i in range(meta["images"][tag]["n_sets"])]
    if name == "greedy37":
        cls, obj, att, pool, pred, nrel = CI.extract_greedy(raw["object_dist"], raw["rel_ind"], raw["rel_off"], d_off, seed, status, 37, 65)
        assert status.cpu().tolist() == want
        bad = [i for i, w in enumerate(want) if w]
        assert (seed.cpu()[bad] == 0).all() and (obj.cpu()[bad] == 36).all() and not att.cpu()[bad].any() and not pool.cpu()[bad].any()
        assert (pred.cpu()[bad] == 64).all() and (nrel.cpu()[bad] == 36).all()
        for b, tag in enumerate(tags):
            assert (cls[b].cpu().numpy() == np.argmax(arr[f"{tag}_object_dist"], 1)).all(), tag
        msg = r"image 1004, region set 1: no region overlaps any detection box; the reference raises ValueError"
    else:
        assert not status.cpu().any()
        choice = CI.gt_lookup(gt["seed"], gt["seed_off"], 36, d_off, seed, status)
        assert status.cpu().tolist() == want and choice.cpu().tolist() == [3, 0, 4, 1, 0, 1, -1, 4]
        msg = r"image 1006, region set 1: none of the image's five precomputed seed lists equals the matched nodes; the reference indexes"
    with pytest.raises(ValueError, match=msg):
        _assemble(meta, arr, tags, only_ok=False)


def test_one_launch_chain_and_image_by_image_give_the_same_bits(case):
    meta, arr = case
    for tags in (BATCHES["greedy37"], BATCHES["gt"]):
        items, table, off = _assemble(meta, arr, tags, widen_classes=40)
        for b, tag in enumerate(tags):
            one, t1, _ = _assemble(meta, arr, (tag,), widen_classes=40)
            for k in G.ROWS + G.GRAPH:
                assert torch.equal(one[0][k], items[b][k]), (tag, k)
            for k in ("idx", "iou", "seed_mask", "status"):
                assert t1[k].tobytes() == table[k][off[b]:off[b + 1]].tobytes(), (tag, k)


def test_assemble_test_batch_equals_the_reference_test_loader(case):
    meta, arr = case
    raw, _, _, _, _ = G.raw_batch(meta, arr, G.PLAIN, DEV)
    items = CI.assemble_test_batch(raw, 37, 65)
    assert [it["this_mini_batch"] for it in items] == [3, 2]
    for it, tag in zip(items, G.PLAIN):
        _check_item(it, G.expected(meta, arr, tag), tag)
    assert arr["p1_rel_ind"].shape[0] > 64                                                   # more relations than fit: the first rel_num - 1


def test_no_output_element_is_left_unwritten(case, monkeypatch):
    """Every output buffer starts as a sentinel (NaN / 0x3fffffff...): none survives, whatever the set's status."""
    meta, arr = case
    real = torch.empty

    def poisoned(*a, **k):
        t = real(*a, **k)
        if t.is_cuda and t.numel():
            t.fill_(float("nan")) if t.is_floating_point() else t.fill_(0x3fffffff if t.dtype != torch.uint8 else 255)
        return t
    for name, tags in BATCHES.items():
        raw, sets, off, wh, gt = G.raw_batch(meta, arr, tags, DEV)
        d_off = torch.tensor(off, dtype=torch.int64, device=DEV)
        d_wh = torch.tensor(wh, dtype=torch.float32, device=DEV)
        info = meta["images"][tags[0]]
        monkeypatch.setattr(torch, "empty", poisoned)
        try:
            outs = list(CI.match_regions(raw["boxes"], d_wh, sets, d_off))
            if name == "gt":
                outs.append(CI.gt_lookup(gt["seed"], gt["seed_off"], 36, d_off, outs[0], outs[3]))
            else:
                outs += list(CI.extract_greedy(raw["object_dist"], raw["rel_ind"], raw["rel_off"], d_off, outs[0], outs[3], info["obj_num"], info["rel_num"]))
        finally:
            monkeypatch.setattr(torch, "empty", real)
        for i, t in enumerate(outs):
            t = t.cpu()
            assert not (torch.isnan(t).any() if t.is_floating_point() else (t == 0x3fffffff).any()), (name, i)


def test_captions_of_assembled_items_equal_those_of_the_reference_built_items(golden, case):
    """The golden `sct` model of tests/test_eval_glue.py: `caption_images` on the assembled items returns the tokens and scores it returns on
    the fixture's reference-built items; `control_images(..., controllability=...)` yields `caption_images`' entries for those items."""
    import controllability_golden as CG
    import subgc.models as models
    from subgc import controllability as C
    from subgc import eval_glue
    meta, arr = case
    g = golden("subgc_greedy")
    w = golden("subgc_beam").group("weights")
    w["logit.bias"][0] += 2.0
    m = models.setup(g.opt(caption_model="topdown", gpn_drop_prob=0.0, sct=1))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = m.to(DEV).eval()
    tags = G.GREEDY37
    n_cls = w["sg_obj_embed.weight"].shape[0]
    assert arr["g0_object_fmap"].shape[1] == g.meta["opt"]["att_feat_size"] and arr["g0_pred_dist"].shape[1] == w["sg_pred_embed.weight"].shape[0]
    ref_items = []
    for tag in tags:                                                                          # the reference's arrays, classes widened with zero columns
        want = G.expected(meta, arr, tag)
        it = {k: torch.from_numpy(np.ascontiguousarray(want[k])) for k in G.ROWS + G.GRAPH}
        it["obj_dist"] = torch.nn.functional.pad(it["obj_dist"], (0, n_cls - it["obj_dist"].size(-1)))
        ref_items.append({k: v.to(DEV) for k, v in it.items()})
    cmeta, carr = CG.load()
    voc = CG.vocab(cmeta)
    infos = [{"id": meta["images"][t]["id"]} for t in tags]
    kw = dict(sample_max=1, beam_size=1, sct=1, remove_bad_endings=1)
    counts = [meta["images"][t]["n_sets"] for t in tags]
    pool = CG.groups(cmeta, carr, "sct_subgc") + CG.groups(cmeta, carr, "rnd")
    refs = C.ControlReferences([pool[i % len(pool)] for i in range(sum(counts))], C.NounVectors(CG.vectors(cmeta, carr, "sct_subgc"), voc, device=None), voc, device=DEV)
    firsts = np.concatenate([[0], np.cumsum(counts)]).tolist()
    arg = {"scorer": C.ControlScorer(refs), "index": {info["id"]: firsts[i] for i, info in enumerate(infos)}}
    want = eval_glue.caption_images(m, ref_items, infos, voc, kw, controllability=arg)
    assert [len(p["caption"]) for p in want] == counts and len({c for p in want for c in p["caption"]}) > 3     # not one caption everywhere
    raw, sets, off, wh, _ = G.raw_batch(meta, arr, tags, DEV, widen_classes=n_cls)
    items, table = CI.assemble_sct_batch(raw, sets, off, wh, 37, 65)
    got = eval_glue.caption_images(m, items, infos, voc, kw, controllability=arg)
    ctl = eval_glue.control_images(m, raw, sets, off, wh, infos, voc, dict(sample_max=1, beam_size=1, remove_bad_endings=1), controllability=arg)

    def same(p, q):
        assert p["image_id"] == q["image_id"] and p["caption"] == q["caption"]
        assert p["subgraph_score"].tobytes() == q["subgraph_score"].tobytes()
        np.testing.assert_array_equal(p["sorted_subgraph_ind"], q["sorted_subgraph_ind"])
        for a, b in zip(p["controllability"], q["controllability"]):
            assert a["group"] == b["group"] and np.float32(a["noun_iou"]).tobytes() == np.float32(b["noun_iou"]).tobytes()
            assert a["pair_iou"].tobytes() == b["pair_iou"].tobytes() and a["accuracy"]["values"].tobytes() == b["accuracy"]["values"].tobytes()
    for b, (p, q, c) in enumerate(zip(want, got, ctl)):
        same(p, q)
        same(p, c)
        assert set(c) - set(p) == {"match"}
        assert c["match"]["idx"].tobytes() == table["idx"][off[b]:off[b + 1]].tobytes() and c["match"]["iou"].tobytes() == table["iou"][off[b]:off[b + 1]].tobytes()
    # the tokens themselves, not only their strings
    r_ref, r_got = m.sample_images(ref_items, opt=kw), m.sample_images(items, opt=kw)
    for a, b in zip(r_ref, r_got):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
