"""Controlled captioning from region boxes without a GPU: the ninth header and its binding, the numpy restatement of the header's contract
(subgc.control_input.restate_*) against the fixture the reference's own loaders wrote (tests/golden/make_golden_sct_loader.py) element for
element, IoU bits included, and the refusals that happen on the host."""
import ctypes

import numpy as np
import pytest
import torch

import sct_loader_golden as G
from subgc import _lib
from subgc import control_input as CI
from subgc._lib import SubgcError

NAMES = {
    "subgc_sct_match": ["boxes", "img_wh", "B", "n_obj", "regions", "set_off", "n_sets", "R", "seed_mask", "match_idx", "match_iou", "status", "stream"],
    "subgc_sct_extract_greedy": ["object_dist", "C", "rel_ind", "rel_off", "B", "n_obj", "set_off", "seed_mask", "status", "n_sets", "obj_num", "rel_num",
                                 "object_cls", "gpn_obj_ind", "att_masks", "gpn_pool_mtx", "gpn_pred_ind", "gpn_nrel_ind", "stream"],
    "subgc_sct_gt_lookup": ["gt_seed", "gt_seed_off", "n_seed", "B", "n_obj", "set_off", "seed_mask", "n_sets", "choice", "status", "stream"],
}


@pytest.fixture(scope="module")
def case():
    return G.load()


def test_ninth_header_parses_and_the_other_eight_keep_their_counts():
    protos = _lib.parse_header(_lib.CONTROL_INPUT_HEADER)
    assert sorted(protos) == sorted(NAMES)
    for name, want in NAMES.items():
        ret, args = protos[name]
        assert ret is ctypes.c_int and [a for _, a in args] == want, name
        t = dict((a, ty) for ty, a in args)
        assert t["stream"] is ctypes.c_void_p and t["set_off"] is ctypes.c_void_p and t["seed_mask"] is ctypes.c_void_p
        assert all(t[a] is ctypes.c_int for a in ("B", "n_obj", "n_sets"))
    src = open(_lib.CONTROL_INPUT_HEADER).read()
    for cite in ("dataloader_test_sct.py:207-228", "dataloader_test_sct.py:261-295", "dataloader_test_sct.py:314-355", "dataloader_test_sct.py:356-368",
                 ":290-291", "numpy 1.x", "ninth public header"):
        assert cite in src, cite
    # every prototype's own comment cites the reference lines it replaces
    for name in NAMES:
        head = src[:src.index("int " + name + "(")]
        assert "dataloader_test_sct.py:" in head[head.rindex("/*"):], name


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same_rows(rows, want, n):
    """The reference's [S, 2, n, ...] arrays hold `rows` [n, ...] in every (sentence, half) copy."""
    for k in G.ROWS:
        assert want[k].shape[:3] == (5, 2, n), (k, want[k].shape)
        for i in range(5):
            for h in range(2):
                np.testing.assert_array_equal(want[k][i, h], rows[k], err_msg=k)
        assert want[k].dtype == rows[k].dtype or k in ("gpn_obj_ind", "gpn_pred_ind", "gpn_nrel_ind"), k


@pytest.mark.parametrize("tag", G.GREEDY + G.GT)
def test_restatement_equals_the_reference_loader(case, tag):
    meta, arr = case
    info = meta["images"][tag]
    assert meta["numpy"].split(".")[0] >= "2" and set(meta["iou_types"]) == {"numpy.float32", "builtins.float"}
    sets, boxes, n_obj = arr[f"{tag}_sets"], arr[f"{tag}_boxes"], info["obj_num"] - 1
    seed, idx, iou, status = CI.restate_match(boxes, info["wh"], sets)
    # every IoU the reference computed, bit for bit, in its loop order (a raising run stops after its first bad set)
    f = np.float32
    sg = (boxes * f(max(info["wh"]))).astype(f) / f(592)
    log, pos = arr[f"{tag}_iou_log"], 0
    for i in range(sets.shape[0]):
        if pos >= len(log):
            break
        for j in range(int(np.count_nonzero(sets[i][:, 4]))):
            mine = np.array([CI._iou_f32(sets[i][j, :4], sg[k]) for k in range(n_obj)], f)
            assert _bits(mine).tolist() == _bits(log[pos:pos + n_obj].astype(f)).tolist(), (tag, i, j)
            assert (log[pos:pos + n_obj] == log[pos:pos + n_obj].astype(f)).all()
            if pos + n_obj <= len(arr[f"{tag}_iou_is_f32"]):                                 # a non-zero IoU is an np.float32 (numpy >= 2)
                assert ((mine != 0) <= arr[f"{tag}_iou_is_f32"][pos:pos + n_obj]).all()
            if idx[i, j] >= 0:
                assert _bits(iou[i, j]) == _bits(mine.max()) and idx[i, j] == int(np.argmax(mine))
            else:
                assert mine.max() == 0
            pos += n_obj
    assert pos == len(log)
    bad = info.get("bad_sets", [])
    if info["mode"] == "greedy":
        assert status.tolist() == [CI.NO_OVERLAP if i in bad else CI.OK for i in range(sets.shape[0])]
        assert all(seed[i] == 0 for i in bad)
        rows = CI.restate_greedy(seed, status, arr[f"{tag}_object_dist"], arr[f"{tag}_rel_ind"], info["obj_num"], info["rel_num"])
        for i in bad:                                                                         # a bad set's rows are padding alone
            assert (rows["gpn_obj_ind"][i] == info["obj_num"] - 1).all() and not rows["att_masks"][i].any() and not rows["gpn_pool_mtx"][i].any()
            assert (rows["gpn_pred_ind"][i] == info["rel_num"] - 1).all() and (rows["gpn_nrel_ind"][i] == info["obj_num"] - 1).all()
    else:
        assert not status.any()
        off = arr[f"{tag}_seed_off"]
        choice, status = CI.restate_gt_lookup(seed, status, [arr[f"{tag}_seed"][off[j]:off[j + 1]] for j in range(5)], n_obj)
        assert status.tolist() == [CI.NO_GT if i in bad else CI.OK for i in range(sets.shape[0])] and all(choice[i] == -1 for i in bad)
        noff = arr[f"{tag}_nrel_off"]
        one = [CI.restate_subgraph_rows(arr[f"{tag}_node_masks"][c], arr[f"{tag}_pred_masks"][c], arr[f"{tag}_nrel"][noff[c]:noff[c + 1]],
                                        info["obj_num"], info["rel_num"]) for c in choice if c >= 0]
        rows = {k: np.stack([o[k] for o in one]) for k in G.ROWS}
    if info["mode"] == "greedy":
        ok = [i for i in range(sets.shape[0]) if i not in bad]
        rows = {k: rows[k][ok] for k in G.ROWS}
    want = G.expected(meta, arr, tag)
    assert int(want["this_mini_batch"][0]) == sets.shape[0] - len(bad)
    _same_rows(rows, want, sets.shape[0] - len(bad))
    if bad:
        assert info["raised"]["type"] == ("ValueError" if info["mode"] == "greedy" else "TypeError")


def test_the_planted_cases_are_what_they_claim(case):
    meta, arr = case
    seed, idx, iou, status = CI.restate_match(arr["g0_boxes"], meta["images"]["g0"]["wh"], arr["g0_sets"])
    nodes = lambda m: [k for k in range(64) if (int(m) >> k) & 1]
    assert _bits(iou[0, 0]) == _bits(0.5) and nodes(seed[0]) == [0]                          # exactly 0.5 is kept
    assert idx[1, 0] == 3 and iou[1, 0] == 1 and (arr["g0_boxes"][3] == arr["g0_boxes"][5]).all()
    assert idx[2, :3].tolist() == [7, 7, 9] and nodes(seed[2]) == [7, 9]                      # a duplicate seed is one node
    assert iou[3, :3].tolist() == [0.25, 0.25, float(np.float32(0.2))] and nodes(seed[3]) == [1, 2]             # all below 0.5: the two tied at the best
    assert idx[4, :3].tolist() == [11, -1, 12] and nodes(seed[4]) == [11, 12]
    assert idx[5].tolist() == [20, 21, -1, -1, -1, -1]
    assert idx[6].tolist() == [30, 31, -1, -1, -1, -1]                                       # flags 1 0 1: the first TWO rows
    assert idx[7, :2].tolist() == [-1, 35]
    g = meta["images"]
    assert [g[t]["obj_num"] for t in G.GREEDY] == [37, 37, 37, 65, 37] and g["g3"]["rel_num"] == 131
    assert [arr[f"{t}_rel_ind"].shape[0] for t in G.GREEDY[:4]] == [0, 17, 64, 100]
    assert arr["g1_object_dist"].shape[1] == 7 and arr["g2_object_dist"].shape[1] == 40
    assert (arr["g1_rel_ind"][:, 0] == arr["g1_rel_ind"][:, 1]).sum() >= 3                   # self-loops
    # class expansion bites with 7 classes: some set keeps more nodes than it matched
    s1, _, _, st1 = CI.restate_match(arr["g1_boxes"], g["g1"]["wh"], arr["g1_sets"])
    rows = CI.restate_greedy(s1, st1, arr["g1_object_dist"], arr["g1_rel_ind"], 37, 65)
    assert any(int(rows["att_masks"][i].sum()) > bin(int(s1[i])).count("1") for i in range(len(s1)))
    # the gt look-ups land on several positions, the first of two equal lists wins
    st, _, _, stt = CI.restate_match(arr["t0_boxes"], g["t0"]["wh"], arr["t0_sets"])
    off = arr["t0_seed_off"]
    choice, _ = CI.restate_gt_lookup(st, stt, [arr["t0_seed"][off[j]:off[j + 1]] for j in range(5)], 36)
    assert choice.tolist() == [3, 0, 4, 1, 0]


@pytest.mark.parametrize("tag", G.PLAIN)
def test_plain_test_loader_restatement(case, tag):
    meta, arr = case
    want = G.expected(meta, arr, tag)
    n_c = arr[f"{tag}_node_masks"].shape[0] - 5
    mb = n_c // 2
    assert int(want["this_mini_batch"][0]) == mb and want["gpn_obj_ind"].shape[:3] == (5, 2, mb)
    noff = arr[f"{tag}_nrel_off"]
    for h in range(2):
        for k in range(mb):
            c = 5 + h * mb + k
            r = CI.restate_subgraph_rows(arr[f"{tag}_node_masks"][c], arr[f"{tag}_pred_masks"][c], arr[f"{tag}_nrel"][noff[c]:noff[c + 1]], 37, 65)
            for key in G.ROWS:
                for i in range(5):
                    np.testing.assert_array_equal(want[key][i, h, k], r[key], err_msg=key)


FAKE = 1 << 20                                                           # never dereferenced: the argument checks come first


def test_entry_points_refuse_on_the_host_and_nothing_to_do_is_ok():
    L = _lib.lib()
    assert L.subgc_sct_match(FAKE, FAKE, 2, 65, FAKE, FAKE, 3, 6, FAKE, FAKE, FAKE, FAKE, None) == -1
    assert b"sct_match: 1 <= n_obj <= 64 detection boxes per image, one lane each (got 65)" in L.subgc_last_error()
    assert L.subgc_sct_match(FAKE, FAKE, 2, 36, FAKE, FAKE, 3, 65, FAKE, FAKE, FAKE, FAKE, None) == -1 and b"1 <= R <= 64 region rows per set (got 65)" in L.subgc_last_error()
    assert L.subgc_sct_match(FAKE, FAKE, 0, 36, FAKE, FAKE, 3, 6, FAKE, FAKE, FAKE, FAKE, None) == -1 and b"3 region sets without an image" in L.subgc_last_error()
    assert L.subgc_sct_match(FAKE, None, 2, 36, FAKE, FAKE, 3, 6, FAKE, FAKE, FAKE, FAKE, None) == -1 and b"sct_match: null pointer" in L.subgc_last_error()
    assert L.subgc_sct_match(None, None, 0, 36, None, None, 0, 6, None, None, None, None, None) == 0
    ex = lambda **o: L.subgc_sct_extract_greedy(FAKE, o.get("C", 7), FAKE, FAKE, 2, o.get("n_obj", 36), FAKE, FAKE, FAKE, 3, o.get("obj_num", 37),
                                                o.get("rel_num", 65), FAKE, FAKE, FAKE, None, FAKE, FAKE, None)
    assert ex(n_obj=65, obj_num=66) == -1 and b"1 <= n_obj <= 64 nodes per image, one lane each (got 65)" in L.subgc_last_error()
    assert ex(obj_num=36) == -1 and b"obj_num = 36 leaves no dummy node behind n_obj = 36" in L.subgc_last_error()
    assert ex(rel_num=1025) == -1 and b"2 <= rel_num <= 1024 (got 1025)" in L.subgc_last_error()
    assert ex(C=0) == -1 and b"C >= 1" in L.subgc_last_error()
    assert L.subgc_sct_extract_greedy(None, 7, None, None, 0, 36, None, None, None, 0, 37, 65, None, None, None, None, None, None, None) == 0
    assert L.subgc_sct_gt_lookup(FAKE, FAKE, 9, 2, 70, FAKE, FAKE, 3, FAKE, FAKE, None) == -1 and b"(got 70)" in L.subgc_last_error()
    assert L.subgc_sct_gt_lookup(FAKE, None, 9, 2, 36, FAKE, FAKE, 3, FAKE, FAKE, None) == -1 and b"sct_gt_lookup: null pointer" in L.subgc_last_error()
    assert L.subgc_sct_gt_lookup(None, None, 0, 0, 36, None, None, 0, None, None, None) == 0


def test_assemble_refuses_on_the_host(case):
    meta, arr = case
    raw, sets, off, wh, _ = G.raw_batch(meta, arr, ("g0", "g1"), "cpu")
    with pytest.raises(ValueError, match="mode 'greedy' or 'gt'"):
        CI.assemble_sct_batch(raw, sets, off, wh, 37, 65, mode="best")
    with pytest.raises(ValueError, match="needs the image's precomputed sub-graphs"):
        CI.assemble_sct_batch(raw, sets, off, wh, 37, 65, mode="gt")
    big = dict(raw, boxes=torch.zeros(2, 65, 4))
    with pytest.raises(ValueError, match="at most 64 objects per image .one lane each., got 65"):
        CI.assemble_sct_batch(big, sets, off, wh, 66, 65)
    many = dict(raw, rel_ind=torch.zeros(70, 2, dtype=torch.int64), rel_off=torch.tensor([0, 5, 70]))
    with pytest.raises(ValueError, match=r"image 1001 has 65 relation rows, more than rel_num - 1 = 64.*dataloader_test_sct.py:352"):
        CI.assemble_sct_batch(many, sets, off, wh, 37, 65)
    nan = dict(raw, boxes=raw["boxes"].clone())
    nan["boxes"][1, 3, 2] = float("inf")
    bad_sets = sets.clone()
    bad_sets[2, 0, 1] = float("nan")
    with pytest.raises(ValueError, match="2 non-finite box coordinates"):
        CI.assemble_sct_batch(nan, bad_sets, off, wh, 37, 65)
    with pytest.raises(ValueError, match=r"1 <= R <= 64 region rows per set, got 65"):
        CI.assemble_sct_batch(raw, torch.zeros(14, 65, 5), off, wh, 37, 65)
    with pytest.raises(ValueError, match="set_off: offsets must ascend from 0 to 14"):
        CI.assemble_sct_batch(raw, sets, [0, 8, 13], wh, 37, 65)
    with pytest.raises(ValueError, match="fp32 represents exactly"):
        CI.assemble_sct_batch(raw, sets, off, [(592, 400), (16777217, 3)], 37, 65)
    with pytest.raises(SubgcError, match="no CPU fallback"):                                  # past the checks: the device path, and only that
        CI.assemble_sct_batch(raw, sets, off, wh, 37, 65)
