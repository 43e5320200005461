"""Helpers shared by the CPU and GPU replays of tests/golden/sct_loader_case.npz / sct_loader_meta.json: the fabricated dataset entries the
reference's `dataloader_test_sct.py` / `dataloader_test.py` `__getitem__` were driven on (make_golden_sct_loader.py) and what they returned."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = ("gpn_obj_ind", "att_masks", "gpn_pool_mtx", "gpn_pred_ind", "gpn_nrel_ind")
GRAPH = ("fc_feats", "att_feats", "obj_dist", "rel_ind", "pred_dist", "labels", "masks")
GREEDY, GREEDY37, GT, PLAIN = ("g0", "g1", "g2", "g3", "g4"), ("g0", "g1", "g2"), ("t0", "t1"), ("p0", "p1")


def load():
    with open(os.path.join(GOLDEN, "sct_loader_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "sct_loader_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def sets_of(meta, arr, tag, only_ok=False):
    """The image's region sets [n, R, 5]; only_ok: without the sets the reference cannot process."""
    s = arr[f"{tag}_sets"]
    return s[meta["images"][tag]["ok_sets"]] if only_ok and meta["images"][tag].get("bad_sets") else s


def expected(meta, arr, tag):
    """What the reference's __getitem__ returned for the image (run without its bad sets when it has some)."""
    out = tag + "ok" if meta["images"][tag].get("bad_sets") else tag
    return {k: arr[f"{out}_out_{k}"] for k in ROWS + GRAPH + ("this_mini_batch",)}


def captions(meta, arr, tag):
    ix, S, Lq = meta["images"][tag]["ix"], meta["seq_per_img"], meta["seq_length"]
    a = int(arr["label_start_ix"][ix]) - 1
    return arr["label"][a:a + S, :Lq]


def raw_batch(meta, arr, tags, device, only_ok=False, widen_classes=None):
    """-> (raw, region_sets, set_off, img_wh, gt) for `assemble_sct_batch` over the images `tags` (one obj_num / rel_num), or with PLAIN
    tags the raw of `assemble_test_batch` (region_sets .. gt None).  widen_classes: zero columns behind object_dist up to that width."""
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
    dist = [arr[f"{g}_object_dist"] for g in tags]
    widen_classes = widen_classes or max(d.shape[1] for d in dist)                       # one width per batch: zero columns change no arg-max
    if widen_classes:
        dist = [np.concatenate([d, np.zeros((d.shape[0], widen_classes - d.shape[1]), np.float32)], 1) for d in dist]
    rels = [arr[f"{g}_rel_ind"].reshape(-1, 2) for g in tags]
    raw = dict(object_fmap=t(np.stack([arr[f"{g}_object_fmap"] for g in tags])), object_dist=t(np.stack(dist)),
               rel_ind=t(np.concatenate(rels), torch.int64), pred_dist=t(np.concatenate([arr[f"{g}_pred_dist"] for g in tags])),
               rel_off=t(np.cumsum([0] + [r.shape[0] for r in rels]), torch.int64), boxes=t(np.stack([arr[f"{g}_boxes"] for g in tags])),
               captions=t(np.concatenate([captions(meta, arr, g) for g in tags]), torch.int64), image_ids=[meta["images"][g]["id"] for g in tags])
    if meta["images"][tags[0]]["mode"] == "plain":
        nm = [arr[f"{g}_node_masks"][5:] for g in tags]
        off = [arr[f"{g}_nrel_off"] for g in tags]
        nrel = [arr[f"{g}_nrel"][o[5]:] for g, o in zip(tags, off)]
        cnt = np.concatenate([np.diff(o[5:]) for o in off])
        raw.update(cand_node_mask=t(np.concatenate(nm), torch.uint8), cand_pred_mask=t(np.concatenate([arr[f"{g}_pred_masks"][5:] for g in tags]), torch.uint8),
                   cand_off=np.cumsum([0] + [m.shape[0] for m in nm]).tolist(), cand_nrel=t(np.concatenate(nrel).reshape(-1, 2), torch.int64),
                   cand_nrel_off=t(np.cumsum(np.concatenate([[0], cnt])), torch.int64))
        return raw, None, None, None, None
    sets = [sets_of(meta, arr, g, only_ok) for g in tags]
    gt = None
    if meta["images"][tags[0]]["mode"] == "gt":
        off = [arr[f"{g}_nrel_off"] for g in tags]
        gt = dict(node_mask=t(np.stack([arr[f"{g}_node_masks"][:5] for g in tags]), torch.uint8),
                  pred_mask=t(np.stack([arr[f"{g}_pred_masks"][:5] for g in tags]), torch.uint8),
                  nrel=t(np.concatenate([arr[f"{g}_nrel"][:o[5]] for g, o in zip(tags, off)]).reshape(-1, 2), torch.int64),
                  nrel_off=t(np.cumsum(np.concatenate([[0]] + [np.diff(o[:6]) for o in off])), torch.int64),
                  seed=t(np.concatenate([arr[f"{g}_seed"] for g in tags]), torch.int64),
                  seed_off=t(np.cumsum(np.concatenate([[0]] + [np.diff(arr[f"{g}_seed_off"]) for g in tags])), torch.int64))
    return (raw, t(np.concatenate(sets)), np.cumsum([0] + [s.shape[0] for s in sets]).tolist(), [meta["images"][g]["wh"] for g in tags], gt)
