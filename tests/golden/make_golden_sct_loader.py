#!/usr/bin/env python
"""Write the controlled-captioning loader fixture by RUNNING THE REFERENCE's own loaders where the reference lies (never copied):
sct_loader_case.npz + sct_loader_meta.json.  Data only: fabricated raw dataset entries and the arrays `DataLoader.__getitem__` returned.

    python tests/golden/make_golden_sct_loader.py

`dataloaders/dataloader_test_sct.py` (:230-394) and `dataloaders/dataloader_test.py` (:216-309) are driven the way make_golden.py drives
the training loader: `h5py` (absent, only used by `__init__`) is stubbed, the object is made with `object.__new__(DataLoader)` and given
exactly the attributes `__getitem__` / `get_captions` read.  `bb_intersection_over_union` is wrapped (on the instance) so that every IoU
the loader saw is stored with its Python type.  A set the reference cannot process makes `__getitem__` raise: the exception's type and
text are stored, and the image is run once more without its bad sets so that the good ones have expected rows (`<tag>ok`).

Images (see `meta["images"]`): g0-g4 greedy (`--use_greedy_subg`), t0-t1 ground truth (`--use_gt_subg`), p0-p1 the plain test loader.
Planted in g0 (integer boxes, max(w, h) = 592: exact scaling): IoU exactly 0.5; two identical detection boxes; two regions on one node;
all matches below 0.5 with two tied at the best; a non-overlapping region among matching ones; flag columns with fewer valid rows than
R, one of them with a zero flag INSIDE the counted prefix.  g1: 17 relations with self-loops; g2: 40 classes, 64 relations, a 640 x 480
image (inexact scaling); g3: obj_num 65 / rel_num 131, 100 relations; g4: sets without any overlap (the reference raises)."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SUBGC_REFERENCE", "/root/reference")
S, LQ, D, PD, R = 5, 16, 64, 21, 6
NAMES = ("fc_feats", "att_feats", "obj_dist", "rel_ind", "pred_dist", "labels", "masks", "ix", "gpn_obj_ind", "gpn_pred_ind", "gpn_nrel_ind",
         "att_masks", "gpn_pool_mtx", "this_mini_batch")
FAR = [560, 560, 580, 580]                                     # behind every detection box of the grid


def det_boxes(rng, n_obj):
    """Integer boxes on an 8-column grid of pitch 70 (nothing overlaps, everything ends at or before 550)."""
    b = np.zeros((n_obj, 4), np.float32)
    for k in range(n_obj):
        x, y = 70 * (k % 8), 70 * (k // 8)
        w, h = 2 * int(rng.integers(10, 31)), 2 * int(rng.integers(10, 31))
        b[k] = [x, y, x + w - 1, y + h - 1]
    return b


def jitter(rng, box, amount):
    return (np.asarray(box, np.float32) + rng.integers(-amount, amount + 1, size=4)).astype(np.float32)


def pack_sets(sets):
    """[[(box, flag), ...], ...] -> [n, R, 5] fp32; unused rows keep a DETECTION-LIKE box with flag 0 (reading one would match)."""
    out = np.zeros((len(sets), R, 5), np.float32)
    out[:, :, :4] = [0, 0, 9, 9]
    for i, rows in enumerate(sets):
        for j, (box, flag) in enumerate(rows):
            out[i, j, :4], out[i, j, 4] = box, flag
    return out


def scene(rng, n_obj, C, n_rel, d=D):
    sg = dict(object_fmap=rng.standard_normal((n_obj, d)).astype(np.float32), object_dist=rng.random((n_obj, C)).astype(np.float32),
              pred_dist=rng.random((n_rel, PD)).astype(np.float32), rel_ind=rng.integers(0, n_obj, size=(n_rel, 2)), boxes=det_boxes(rng, n_obj))
    sg["object_dist"][2, :] = 0.25                              # every class ties: the first wins
    sg["object_dist"][4, [1, C - 1]] = 2.0                      # two equal maxima
    return sg


def random_sets(rng, boxes, n, amount=12):
    sets = []
    for _ in range(n):
        rows = [(jitter(rng, boxes[int(rng.integers(0, boxes.shape[0]))], amount), 1.0) for _ in range(int(rng.integers(1, R + 1)))]
        sets.append(rows)
    return sets


def greedy_images(rng):
    ims = {}
    # g0: the planted matching cases, no relations
    sg = scene(rng, 36, 7, 0)
    b = sg["boxes"]
    b[0], b[1], b[2], b[3] = [0, 0, 9, 9], [70, 0, 89, 19], [140, 0, 159, 19], [210, 0, 249, 29]
    b[5] = b[3]
    sets = [
        [([0, 0, 9, 4], 1.0)],                                                                  # IoU exactly 0.5: kept (>=)
        [(b[3].copy(), 1.0)],                                                                   # two identical boxes: the first (3) wins
        [(jitter(rng, b[7], 3), 1.0), (jitter(rng, b[7], 3), 1.0), (jitter(rng, b[9], 3), 1.0)],  # two regions, one node
        [([70, 0, 79, 9], 1.0), ([140, 0, 149, 9], 1.0), ([0, 0, 4, 3], 1.0)],                  # 0.25, 0.25, 0.2: the two tied stay
        [(jitter(rng, b[11], 2), 1.0), (FAR, 1.0), (jitter(rng, b[12], 2), 1.0)],               # one region overlaps nothing: skipped
        [(jitter(rng, b[20], 2), 1.0), (jitter(rng, b[21], 2), 2.0)],                           # 2 valid rows of R, any non-zero flag counts
        [(jitter(rng, b[30], 2), 1.0), (jitter(rng, b[31], 2), 0.0), (jitter(rng, b[32], 2), 1.0)],   # flags 1 0 1: the FIRST two rows
        [(FAR, 1.0), (jitter(rng, b[35], 2), 1.0)],                                             # the last node, behind a non-overlapping row
    ]
    ims["g0"] = dict(sg=sg, wh=(592, 400), sets=pack_sets(sets), obj_num=37, rel_num=65, mode="greedy")
    # g1: few classes, 17 relations with self-loops
    sg = scene(rng, 36, 7, 17)
    sg["rel_ind"][3], sg["rel_ind"][9], sg["rel_ind"][16] = [5, 5], [0, 0], [35, 35]
    ims["g1"] = dict(sg=sg, wh=(592, 592), sets=pack_sets(random_sets(rng, sg["boxes"], 6)), obj_num=37, rel_num=65, mode="greedy")
    # g2: many classes, exactly rel_num - 1 relations, inexact scaling
    sg = scene(rng, 36, 40, 64)
    scaled = (sg["boxes"] * 640 / 592).astype(np.float32)
    ims["g2"] = dict(sg=sg, wh=(640, 480), sets=pack_sets(random_sets(rng, scaled, 7, amount=8)), obj_num=37, rel_num=65, mode="greedy")
    # g3: a full wave of nodes, two relation chunks
    sg = scene(rng, 64, 7, 100, d=8)
    sg["rel_ind"][70], sg["rel_ind"][99] = [63, 63], [63, 0]
    sets = random_sets(rng, sg["boxes"], 5) + [[(jitter(rng, sg["boxes"][63], 2), 1.0)], [(jitter(rng, sg["boxes"][0], 2), 1.0), (jitter(rng, sg["boxes"][62], 2), 1.0)]]
    ims["g3"] = dict(sg=sg, wh=(400, 592), sets=pack_sets(sets), obj_num=65, rel_num=131, mode="greedy")
    # g4: sets the reference cannot process (np.max of an empty list)
    sg = scene(rng, 36, 7, 17)
    sets = [[(jitter(rng, sg["boxes"][6], 2), 1.0)], [(FAR, 1.0), ([570, 10, 590, 30], 1.0)], [(sg["boxes"][8].copy(), 0.0)], [(jitter(rng, sg["boxes"][14], 2), 1.0)]]
    ims["g4"] = dict(sg=sg, wh=(592, 300), sets=pack_sets(sets), obj_num=37, rel_num=65, mode="greedy", bad=[1, 2])
    return ims


def mask_list(rng, n_obj, rel_num, seeds, n_cand):
    """subgraph_mask_list: [id, node mask, predicate mask, renumbered endpoints, seed nodes] per entry; the first 5 are the sentences'."""
    out = []
    for j in range(5 + n_cand):
        nm = rng.random(n_obj) < 0.25
        if j == 6:
            nm[:] = False                                        # an empty sub-graph among the candidates
        pm = rng.random(rel_num - 1) < 0.1
        nrel = rng.integers(0, max(1, int(nm.sum())), size=(int(pm.sum()), 2))
        out.append([j, nm, pm, nrel, np.array(seeds[j] if j < 5 else [], dtype=np.int64)])
    return out


def gt_images(rng):
    ims = {}
    sg = scene(rng, 36, 7, 30)
    b = sg["boxes"]
    seeds = [[3, 3, 8], [1], [8, 3], [10, 11, 12], [20, 20, 20, 21]]       # repeats; list 2 holds the same nodes as list 0: the first wins
    on = lambda *nodes: [(jitter(rng, b[k], 2), 1.0) for k in nodes]
    sets = [on(12, 10, 11), on(8, 3), on(20, 21, 21), on(1), on(3, 8, 8)]
    ims["t0"] = dict(sg=sg, wh=(592, 444), sets=pack_sets(sets), obj_num=37, rel_num=65, mode="gt", masks=mask_list(rng, 36, 65, seeds, 7))
    sg = scene(rng, 36, 7, 5)
    b = sg["boxes"]
    seeds = [[2, 5, 6], [4], [7, 7], [2], [9, 30]]
    sets = [on(4), on(2, 5), on(30, 9)]                                    # {2, 5}: a subset of list 0 and a superset of list 3, equal to none
    ims["t1"] = dict(sg=sg, wh=(592, 592), sets=pack_sets(sets), obj_num=37, rel_num=65, mode="gt", masks=mask_list(rng, 36, 65, seeds, 4), bad=[1])
    return ims


def captions(rng, n_img):
    labels, start, end = [], [], []
    for _ in range(n_img):
        caps = rng.integers(1, 50, size=(S, LQ))
        for r in range(S):
            caps[r, rng.integers(0, LQ + 1):] = 0
        start.append(len(labels) + 1)
        labels.extend(list(caps))
        end.append(len(labels))
    return np.stack(labels).astype(np.int64), np.array(start), np.array(end)


def main():
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    from dataloaders.dataloader_test_sct import DataLoader as SctLoader
    from dataloaders.dataloader_test import DataLoader as TestLoader
    rng = np.random.default_rng(20260918)
    ims = {**greedy_images(rng), **gt_images(rng)}
    # the plain test loader: t0's mask list (7 candidates: 3 + 3, the odd one unused) and a short list over more relations than fit
    sg = scene(rng, 36, 7, 70)
    ims["p0"] = dict(sg=ims["t0"]["sg"], masks=ims["t0"]["masks"], obj_num=37, rel_num=65, mode="plain")
    ims["p1"] = dict(sg=sg, masks=mask_list(rng, 36, 65, [[0]] * 5, 4), obj_num=37, rel_num=65, mode="plain")
    tags = list(ims)
    label, start, end = captions(rng, len(tags))
    arrays, meta = {}, {"numpy": np.__version__, "torch": torch.__version__, "seq_per_img": S, "seq_length": LQ, "R": R, "tags": tags, "images": {}}
    arrays.update(label=label, label_start_ix=start, label_end_ix=end)
    type_names = {}

    def run(tag, ix, keep=None):
        """-> (returned arrays or None, exception or None, IoU log) of the reference's __getitem__ for image `tag`, sets `keep` only."""
        im = ims[tag]
        plain = im["mode"] == "plain"
        dl = object.__new__(TestLoader if plain else SctLoader)
        dl.info = {"images": [{"id": 1000 + i} for i in range(len(tags))]}
        dl.seq_per_img, dl.seq_length, dl.obj_num, dl.rel_num = S, LQ, im["obj_num"], im["rel_num"]
        dl.label_start_ix, dl.label_end_ix = start, end
        dl.trip_loader = types.SimpleNamespace(get=lambda key: im["sg"])
        if "masks" in im:
            iou_mtx = np.zeros((S, len(im["masks"])))
            dl.subgraph_mask = types.SimpleNamespace(get=lambda key: {"node_iou_mtx": iou_mtx, "subgraph_mask_list": im["masks"]})
        log = []
        if plain:
            dl.label = label
        else:
            sets = im["sets"] if keep is None else im["sets"][keep]
            dl.h5_label_file = {"labels": label}
            dl.sct_dict = {str(1000 + ix): torch.from_numpy(sets)}
            dl.img_wh = {1000 + ix: im["wh"]}
            dl.use_greedy_subg, dl.use_gt_subg = int(im["mode"] == "greedy"), int(im["mode"] == "gt")
            inner = SctLoader.bb_intersection_over_union

            def logged(boxA, boxB):
                v = inner(dl, boxA, boxB)
                log.append(v)
                return v
            dl.bb_intersection_over_union = logged
        try:
            return dl.__getitem__(ix), None, log
        except Exception as e:                                   # noqa: BLE001 -- the exception IS the recorded result
            return None, e, log

    for ix, tag in enumerate(tags):
        im = ims[tag]
        info = dict(id=1000 + ix, ix=ix, mode=im["mode"], obj_num=im["obj_num"], rel_num=im["rel_num"])
        for k, v in im["sg"].items():
            arrays[f"{tag}_{k}"] = v
        if "masks" in im:
            arrays[f"{tag}_node_masks"] = np.stack([m[1] for m in im["masks"]])
            arrays[f"{tag}_pred_masks"] = np.stack([m[2] for m in im["masks"]])
            arrays[f"{tag}_nrel"] = np.concatenate([m[3] for m in im["masks"]]).reshape(-1, 2).astype(np.int64)
            arrays[f"{tag}_nrel_off"] = np.cumsum([0] + [m[3].shape[0] for m in im["masks"]])
            arrays[f"{tag}_seed"] = np.concatenate([m[4] for m in im["masks"][:5]]).astype(np.int64)
            arrays[f"{tag}_seed_off"] = np.cumsum([0] + [m[4].shape[0] for m in im["masks"][:5]])
        if im["mode"] != "plain":
            arrays[f"{tag}_sets"] = im["sets"]
            info.update(wh=list(im["wh"]), n_sets=int(im["sets"].shape[0]), bad_sets=im.get("bad", []))
        ret, exc, log = run(tag, ix)
        if im.get("bad"):
            assert ret is None and exc is not None, tag
            info["raised"] = {"type": type(exc).__name__, "text": str(exc)}
            good = [i for i in range(im["sets"].shape[0]) if i not in im["bad"]]
            info["ok_sets"] = good
            ret, exc, log_ok = run(tag, ix, keep=good)
            assert exc is None, (tag, exc)
            out_tag = tag + "ok"
        else:
            assert exc is None, (tag, exc)
            out_tag = tag
        for nme, arr in zip(NAMES, ret):
            arrays[f"{out_tag}_out_{nme}"] = np.asarray(arr)
        if im["mode"] != "plain":
            for v in log:
                type_names[type(v).__module__ + "." + type(v).__name__] = type_names.get(type(v).__module__ + "." + type(v).__name__, 0) + 1
            arrays[f"{tag}_iou_log"] = np.array([float(v) for v in log], np.float64)          # every value is an fp32 or 0.0: exact
            arrays[f"{tag}_iou_is_f32"] = np.array([isinstance(v, np.float32) for v in log], np.bool_)
            if im.get("bad"):                                    # the run without the bad sets saw these
                arrays[f"{out_tag}_iou_log"] = np.array([float(v) for v in log_ok], np.float64)
        meta["images"][tag] = info
    meta["iou_types"] = type_names
    np.savez_compressed(os.path.join(HERE, "sct_loader_case.npz"), **arrays)
    with open(os.path.join(HERE, "sct_loader_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote sct_loader_case.npz (%d arrays, %d bytes), iou types %s" % (len(arrays), os.path.getsize(os.path.join(HERE, "sct_loader_case.npz")), type_names))
    for tag, info in meta["images"].items():
        print(tag, {k: v for k, v in info.items() if k in ("mode", "n_sets", "raised")})


if __name__ == "__main__":
    main()
