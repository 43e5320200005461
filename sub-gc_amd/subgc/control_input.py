"""Controlled captioning from region boxes: the batch assembly of `test.py --sct 1` on the device, and the plain test loader's item.

The reference turns a user's control signal -- a set of region boxes per wanted caption -- into the model's inputs inside
`dataloaders/dataloader_test_sct.py` `DataLoader.__getitem__` (:261-380): a Python triple loop matches every region to the scene graph's
detection boxes by IoU (:267-284, `bb_intersection_over_union` :207-228), a threshold / best-match filter follows (:287-293), and the
sub-graph of every set is extracted greedily (`--use_greedy_subg`, :314-355) or looked up among the image's five precomputed ground-truth
sub-graphs (`--use_gt_subg`, :356-380).  Here the caller hands over the RAW per-image arrays (on the device) and the packed region sets;
`assemble_sct_batch` runs one launch chain over the whole batch (include/subgc_control_input_hip.h: subgc_sct_match,
subgc_sct_extract_greedy, subgc_sct_gt_lookup, then the training loader's padding kernels) and returns one loader item per image, ready
for `model.sample_images` / `eval_glue.caption_images` in `sct` mode.  `assemble_test_batch` is the plain test loader
(`dataloaders/dataloader_test.py:216-309`) from the existing kernels.  Pinned on what the reference's own `__getitem__` returns
(tests/golden/sct_loader_*.npz/json), IoU bits included.

`restate_match` / `restate_greedy` / `restate_gt_lookup` / `restate_subgraph_rows` are numpy restatements of the header's contract, one
image at a time (the CPU test compares them with the fixture element for element; nothing on the product path calls them).

Limits, all refused with the numbers in the text: at most 64 objects per image (one lane each), at most `rel_num - 1` relation rows per
image (the reference's row assignment :352 cannot hold more), at most 64 region rows per set, finite boxes.  numpy >= 2 semantics: the
IoU quotient is fp32 (numpy 1.x would divide in fp64; not built).  The reference's "keep all SG nodes" branch (:290-291) is dead code
(np.max of an empty list raises first) and is not invented here: such a set is an error, as is a gt set without an equal seed list.
Out of scope: the input files themselves (sct_dict_*.npy, flickr30k_img_wh.npy, the gt graph masks), BlobFetcher and the iterators.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call_control_input
from .assemble import caption_labels, pad_rows, pad_segments, subgraph_indices
from .ops import _ptr, _stream

MAX_OBJ, MAX_REGIONS, GT_LISTS = 64, 64, 5
OK, NO_OVERLAP, NO_GT = 0, 1, 2


# ---- numpy restatement of the contract (one image) ------------------------------------------------------------------------------------

def _iou_f32(a, b):
    """subgc_control_input_hip.h's IoU of region `a` and detection box `b` (fp32 rows), every operation rounded on its own."""
    f = np.float32
    xA, yA, xB, yB = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    iw = f(f(xB - xA) + f(1))
    ih = f(f(yB - yA) + f(1))
    iw = iw if iw > 0 else f(0)
    ih = ih if ih > 0 else f(0)
    inter = f(iw * ih)
    areaA = f(f(f(a[2] - a[0]) + f(1)) * f(f(a[3] - a[1]) + f(1)))
    areaB = f(f(f(b[2] - b[0]) + f(1)) * f(f(b[3] - b[1]) + f(1)))
    with np.errstate(divide="ignore", invalid="ignore"):
        return f(inter / f(f(areaA + areaB) - inter))


def restate_match(boxes, wh, region_sets):
    """boxes [n_obj, 4] fp32, wh (w, h), region_sets [n, R, 5] fp32 -> (seed_mask [n] uint64, idx [n, R] int32, iou [n, R] fp32, status [n])."""
    f = np.float32
    boxes = np.asarray(boxes, f)
    m = f(max(f(wh[0]), f(wh[1])))
    sg = (boxes * m).astype(f) / f(592)
    n, R = region_sets.shape[:2]
    seed, idx, iou, status = np.zeros(n, np.uint64), np.full((n, R), -1, np.int32), np.zeros((n, R), f), np.zeros(n, np.int32)
    for i in range(n):
        valid = int(np.count_nonzero(region_sets[i][:, 4]))
        for j in range(valid):
            best, at = f(0), -1
            for k in range(sg.shape[0]):
                v = _iou_f32(region_sets[i][j, :4].astype(f), sg[k])
                if v > best:
                    best, at = v, k
            idx[i, j], iou[i, j] = at, best
        hit = idx[i] >= 0
        if not hit.any():
            status[i] = NO_OVERLAP
            continue
        keep = hit & (iou[i] >= f(0.5))
        if not keep.any():
            keep = hit & (iou[i] >= iou[i][hit].max())
        for k in idx[i][keep]:
            seed[i] |= np.uint64(1) << np.uint64(k)
    return seed, idx, iou, status


def _rows(nodes, rels, nrel, obj_num, rel_num):
    obj = np.full(obj_num, obj_num - 1, np.int64)
    att = np.zeros(obj_num, np.float32)
    pool = np.zeros((obj_num, obj_num), np.float32)
    pred = np.full(rel_num, rel_num - 1, np.int64)
    nr = np.full((rel_num, 2), obj_num - 1, np.int64)
    obj[:len(nodes)] = nodes
    att[:len(nodes)] = 1
    pool[np.arange(len(nodes)), np.arange(len(nodes))] = 1
    pred[:len(rels)] = rels
    nr[:len(nrel)] = np.asarray(nrel, np.int64).reshape(-1, 2)
    return dict(gpn_obj_ind=obj, att_masks=att, gpn_pool_mtx=pool, gpn_pred_ind=pred, gpn_nrel_ind=nr)


def restate_greedy(seed_mask, status, object_dist, rel_ind, obj_num, rel_num):
    """One image's sets -> stacked rows {gpn_obj_ind [n, obj_num], att_masks, gpn_pool_mtx, gpn_pred_ind, gpn_nrel_ind} + object_cls."""
    n_obj = object_dist.shape[0]
    cls = np.argmax(object_dist, axis=1).astype(np.int32)
    rel = np.asarray(rel_ind, np.int64).reshape(-1, 2)[:rel_num - 1]
    out = []
    for s, st in zip(seed_mask, status):
        bits = [k for k in range(n_obj) if (int(s) >> k) & 1] if st == OK else []
        kinds = {int(cls[k]) for k in bits}
        nodes0 = {k for k in range(n_obj) if int(cls[k]) in kinds}
        kept = [r for r in range(rel.shape[0]) if int(rel[r, 0]) in nodes0 or int(rel[r, 1]) in nodes0]
        nodes = sorted(nodes0 | {int(e) for r in kept for e in rel[r]})
        new = {k: i for i, k in enumerate(nodes)}
        out.append(_rows(nodes, kept, [[new[int(rel[r, 0])], new[int(rel[r, 1])]] for r in kept], obj_num, rel_num))
    rows = {k: np.stack([o[k] for o in out]) for k in out[0]} if out else {}
    rows["object_cls"] = cls
    return rows


def restate_gt_lookup(seed_mask, status, seed_lists, n_obj):
    """-> (choice [n] int32, status [n]) for one image's sets against its five seed lists."""
    masks = []
    for lst in seed_lists:
        lst = [int(v) for v in lst]
        masks.append(None if any(v < 0 or v >= n_obj for v in lst) else sum(1 << v for v in set(lst)))
    choice, status = np.full(len(seed_mask), -1, np.int32), np.array(status, np.int32)
    for i, s in enumerate(seed_mask):
        if status[i] != OK:
            continue
        hit = [j for j, m in enumerate(masks) if m is not None and m == int(s)]
        if hit:
            choice[i] = hit[0]
        else:
            status[i] = NO_GT
    return choice, status


def restate_subgraph_rows(node_mask, pred_mask, nrel, obj_num, rel_num):
    """The rows of one precomputed sub-graph (dataloader_test_sct.py:371-380, dataloader_test.py:243-273)."""
    return _rows(np.flatnonzero(node_mask), np.flatnonzero(pred_mask), nrel, obj_num, rel_num)


# ---- the device path -------------------------------------------------------------------------------------------------------------------

def _host_offsets(off, what, n_top=None):
    h = [int(v) for v in (off.tolist() if hasattr(off, "tolist") else off)]
    if not h or h[0] != 0 or any(b < a for a, b in zip(h, h[1:])) or (n_top is not None and h[-1] != n_top):
        raise ValueError(f"{what}: offsets must ascend from 0" + ("" if n_top is None else f" to {n_top}") + f" (got {h[:8]}{'...' if len(h) > 8 else ''})")
    return h


def _graph_part(raw, obj_num, rel_num, captions, seq_per_img):
    """The scene-graph half both test loaders share (dataloader_test.py:276-305) -> (batched dict, rel counts on the host)."""
    fmap, dist = raw["object_fmap"], raw["object_dist"]
    B, n_obj, D = fmap.shape
    if n_obj > MAX_OBJ:
        raise ValueError(f"control_input: at most {MAX_OBJ} objects per image (one lane each), got {n_obj}")
    if n_obj != obj_num - 1:
        raise ValueError(f"the loader pads exactly one dummy node: expected {obj_num - 1} objects per image, got {n_obj}")
    dev = fmap.device
    rel_off = _host_offsets(raw["rel_off"], "rel_off", int(raw["rel_ind"].size(0)))
    if len(rel_off) != B + 1:
        raise ValueError(f"rel_off holds {len(rel_off)} entries for {B} images")
    per_img = torch.arange(B + 1, device=dev, dtype=torch.int64) * n_obj
    d_rel_off = raw["rel_off"].to(device=dev, dtype=torch.int64)
    rel, pdist = raw["rel_ind"], raw["pred_dist"]
    if rel.size(0) == 0:                                        # a batch without any relation: one row nobody reads keeps the pointers non-null
        rel, pdist = torch.zeros(1, 2, device=dev, dtype=torch.int64), torch.zeros(1, pdist.size(1), device=dev)
    out = {
        "fc_feats": torch.zeros(B, D, device=dev),
        "att_feats": pad_rows(fmap.reshape(B * n_obj, D), per_img, obj_num, n_obj),
        "obj_dist": pad_rows(dist.reshape(B * n_obj, -1), per_img, obj_num, n_obj, onehot0=True),
        "rel_ind": pad_rows(rel, d_rel_off, rel_num, rel_num - 1, pad=obj_num - 1),
        "pred_dist": pad_rows(pdist, d_rel_off, rel_num, rel_num - 1, onehot0=True),
    }
    if captions is not None:
        if captions.size(0) != B * seq_per_img:
            raise ValueError(f"captions: {captions.size(0)} rows for {B} images x seq_per_img = {seq_per_img}")
        out["labels"], out["masks"] = caption_labels(captions)
    return out, rel_off, d_rel_off


def _items(graph, rows, seg, S, materialize):
    """Per image: the graph's own slice and the sub-graph rows seg[b] .. seg[b+1] as [S, 2, mb, ...] (`get_batch`'s views, :182-194).
    rows: {key: (tensor [n, ...], two_halves)}: two_halves False -> both halves show the same rows (sct), True -> first / second half."""
    items = []
    for b, (a, e) in enumerate(zip(seg, seg[1:])):
        it = {k: v[b:b + 1] for k, v in graph.items() if k not in ("labels", "masks")}
        if "labels" in graph:
            it["labels"], it["masks"] = graph["labels"][b * S:(b + 1) * S], graph["masks"][b * S:(b + 1) * S]
        for k, (t, halves) in rows.items():
            x = t[a:e]
            if halves:
                mb = (e - a) // 2
                x = x[:2 * mb].reshape(2, mb, *t.shape[1:])
            else:
                mb = e - a
                x = x.unsqueeze(0).expand(2, mb, *t.shape[1:])
            x = x.unsqueeze(0).expand(S, *x.shape)
            it[k] = x.contiguous() if materialize else x
        it["this_mini_batch"] = mb
        items.append(it)
    return items


def match_regions(boxes, wh, region_sets, set_off):
    """subgc_sct_match on device tensors: boxes [B, n_obj, 4] f32, wh [B, 2] f32, region_sets [n, R, 5] f32, set_off [B+1] i64
    -> (seed_mask [n] int64 holding the 64-bit masks, match_idx [n, R] int32, match_iou [n, R] f32, status [n] int32); nothing is read back."""
    B, n_obj = boxes.shape[:2]
    n_sets, R = int(region_sets.size(0)), int(region_sets.size(1))
    e = lambda *sh, dt: torch.empty(*sh, device=boxes.device, dtype=dt)
    seed, idx, iou, status = e(n_sets, dt=torch.int64), e(n_sets, R, dt=torch.int32), e(n_sets, R, dt=torch.float32), e(n_sets, dt=torch.int32)
    call_control_input("subgc_sct_match", _ptr(boxes, torch.float32), _ptr(wh, torch.float32), B, n_obj, _ptr(region_sets, torch.float32),
                       _ptr(set_off, torch.int64), n_sets, R, _ptr(seed), _ptr(idx), _ptr(iou), _ptr(status), _stream())
    return seed, idx, iou, status


def extract_greedy(object_dist, rel_ind, rel_off, set_off, seed, status, obj_num, rel_num, want_pool_mtx=True):
    """subgc_sct_extract_greedy -> (object_cls [B, n_obj] int32, gpn_obj_ind [n, obj_num], att_masks, gpn_pool_mtx | None, gpn_pred_ind
    [n, rel_num], gpn_nrel_ind [n, rel_num, 2]): one row per region set."""
    dist = object_dist.to(torch.float32).contiguous()
    rel = rel_ind.contiguous()
    B, n_obj, C = dist.shape
    n_sets = int(seed.numel())
    e = lambda *sh, dt: torch.empty(*sh, device=dist.device, dtype=dt)
    cls = e(B, n_obj, dt=torch.int32)
    obj, att = e(n_sets, obj_num, dt=torch.int64), e(n_sets, obj_num, dt=torch.float32)
    pool = e(n_sets, obj_num, obj_num, dt=torch.float32) if want_pool_mtx else None
    pred, nrel = e(n_sets, rel_num, dt=torch.int64), e(n_sets, rel_num, 2, dt=torch.int64)
    call_control_input("subgc_sct_extract_greedy", _ptr(dist), C, _ptr(rel, torch.int64) if rel.numel() else None, _ptr(rel_off, torch.int64), B, n_obj,
                       _ptr(set_off, torch.int64), _ptr(seed, torch.int64), _ptr(status, torch.int32), n_sets, obj_num, rel_num, _ptr(cls), _ptr(obj),
                       _ptr(att), _ptr(pool), _ptr(pred), _ptr(nrel), _stream())
    return cls, obj, att, pool, pred, nrel


def gt_lookup(gt_seed, gt_seed_off, n_obj, set_off, seed, status):
    """subgc_sct_gt_lookup -> choice [n] int32 (the first equal seed list of the set's image, -1: none); `status` is updated in place."""
    dev = seed.device
    g_seed, g_off = gt_seed.to(device=dev, dtype=torch.int64).contiguous(), gt_seed_off.to(device=dev, dtype=torch.int64).contiguous()
    B, n_sets = (int(g_off.numel()) - 1) // GT_LISTS, int(seed.numel())
    choice = torch.empty(n_sets, device=dev, dtype=torch.int32)
    call_control_input("subgc_sct_gt_lookup", _ptr(g_seed) if g_seed.numel() else None, _ptr(g_off), int(g_seed.numel()), B, n_obj,
                       _ptr(set_off, torch.int64), _ptr(seed, torch.int64), n_sets, _ptr(choice), _ptr(status, torch.int32), _stream())
    return choice


def assemble_sct_batch(raw, region_sets, set_off, img_wh, obj_num, rel_num, mode="greedy", gt=None, captions=None, seq_per_img=5,
                       materialize=False, want_pool_mtx=True):
    """raw (all on the device): `assemble_train_batch`'s scene-graph entries -- object_fmap [B, obj_num-1, D] f32, object_dist
         [B, obj_num-1, C] f32, rel_ind [sum_k, 2] i64, pred_dist [sum_k, P] f32, rel_off [B+1] i64 -- plus boxes [B, obj_num-1, 4] f32
         (the detector's boxes, dataloader_test_sct.py:262) and optionally image_ids (a list, for error texts; default 0 .. B-1).
       region_sets [sum_sets, R, 5] f32 (x1, y1, x2, y2, flag) with set_off [B+1]: image b's sets are rows set_off[b] .. set_off[b+1]-1.
       img_wh [B, 2]: (w, h) per image, numbers an fp32 holds exactly (:261, 263).
       mode "greedy" (--use_greedy_subg) or "gt" (--use_gt_subg) with gt = {node_mask [B, 5, obj_num-1] u8, pred_mask [B, 5, rel_num-1]
         u8, nrel [sum, 2] i64 + nrel_off [5 B + 1] i64, seed [n_seed] i64 + seed_off [5 B + 1] i64}: subgraph_mask_list[:5] of every image.
       captions [B * seq_per_img, seq_length] i64 or None (default: raw's, if it has them): labels / masks of the item.
       -> (items, table): items[b] holds the keys `get_batch` returns (:182-194) for image b with its own number of sets as
          `this_mini_batch`; the [seq_per_img, 2, sets, ...] tensors are stride-0 views of one row per set (`materialize=True`: copies).
          table = {"idx" [sum_sets, R] int32, "iou" [sum_sets, R] fp32, "seed_mask" [sum_sets] uint64, "status" [sum_sets] int32} on the
          host (numpy): per region the matched detection box (-1: none) and its IoU before the filter.
       A set without any overlapping region, or (gt) without an equal seed list, raises ValueError naming the image id and the set."""
    if mode not in ("greedy", "gt"):
        raise ValueError(f"assemble_sct_batch: mode 'greedy' or 'gt', got {mode!r}")
    if mode == "gt" and gt is None:
        raise ValueError("assemble_sct_batch: mode 'gt' needs the image's precomputed sub-graphs (gt=)")
    boxes = raw["boxes"]
    B, n_obj = boxes.shape[:2]
    dev = boxes.device
    if n_obj > MAX_OBJ:
        raise ValueError(f"assemble_sct_batch: at most {MAX_OBJ} objects per image (one lane each), got {n_obj}")
    if region_sets.dim() != 3 or region_sets.size(2) != 5:
        raise ValueError(f"assemble_sct_batch: region_sets [sum_sets, R, 5], got {tuple(region_sets.shape)}")
    n_sets, R = int(region_sets.size(0)), int(region_sets.size(1))
    if R > MAX_REGIONS or R < 1:
        raise ValueError(f"assemble_sct_batch: 1 <= R <= {MAX_REGIONS} region rows per set, got {R}")
    seg = _host_offsets(set_off, "set_off", n_sets)
    if len(seg) != B + 1:
        raise ValueError(f"assemble_sct_batch: set_off holds {len(seg)} entries for {B} images")
    ids = list(raw.get("image_ids", range(B)))
    captions = raw.get("captions") if captions is None else captions
    rel_cnt = np.diff(_host_offsets(raw["rel_off"], "rel_off"))
    if rel_cnt.size and int(rel_cnt.max()) > rel_num - 1:
        b = int(rel_cnt.argmax())
        raise ValueError(f"assemble_sct_batch: image {ids[b]!r} has {int(rel_cnt[b])} relation rows, more than rel_num - 1 = {rel_num - 1}: the "
                         "reference's row assignment (dataloader_test_sct.py:352) cannot hold them")
    region_sets = region_sets.to(torch.float32).contiguous()
    boxes = boxes.to(torch.float32).contiguous()
    bad = int((~torch.isfinite(boxes)).sum()) + int((~torch.isfinite(region_sets[:, :, :4])).sum()) if n_sets else int((~torch.isfinite(boxes)).sum())
    if bad:
        raise ValueError(f"assemble_sct_batch: {bad} non-finite box coordinates (detection boxes and region sets must be finite)")
    wh = torch.as_tensor(np.asarray(img_wh, dtype=np.float64).reshape(B, 2))
    if not bool((wh.float().double() == wh).all()):
        raise ValueError("assemble_sct_batch: img_wh must hold numbers an fp32 represents exactly")
    wh = wh.float().to(dev)
    graph, _, d_rel_off = _graph_part(raw, obj_num, rel_num, captions, seq_per_img)
    d_set_off = torch.tensor(seg, dtype=torch.int64, device=dev)
    seed, idx, iou, status = match_regions(boxes, wh, region_sets, d_set_off)
    if mode == "greedy":
        cls, obj, att, pool, pred, nrel = extract_greedy(raw["object_dist"], raw["rel_ind"], d_rel_off, d_set_off, seed, status, obj_num, rel_num,
                                                         want_pool_mtx=want_pool_mtx)
    else:
        if gt["seed_off"].numel() != GT_LISTS * B + 1 or gt["nrel_off"].numel() != GT_LISTS * B + 1:
            raise ValueError(f"assemble_sct_batch: gt seed_off / nrel_off hold {gt['seed_off'].numel()} / {gt['nrel_off'].numel()} entries, expected "
                             f"5 B + 1 = {GT_LISTS * B + 1}")
        choice = gt_lookup(gt["seed"], gt["seed_off"], n_obj, d_set_off, seed, status)
    table = {"idx": idx.cpu().numpy(), "iou": iou.cpu().numpy(), "seed_mask": seed.cpu().numpy().view(np.uint64), "status": status.cpu().numpy()}
    if table["status"].any():                                                    # the one host read of the chain decides
        s = int(np.flatnonzero(table["status"])[0])
        b = int(np.searchsorted(seg, s, side="right")) - 1
        if table["status"][s] == NO_OVERLAP:
            raise ValueError(f"assemble_sct_batch: image {ids[b]!r}, region set {s - seg[b]}: no region overlaps any detection box; the reference raises "
                             "ValueError there (np.max of an empty list, dataloader_test_sct.py:289; its 'keep all SG nodes' branch :290-291 is never reached)")
        raise ValueError(f"assemble_sct_batch: image {ids[b]!r}, region set {s - seg[b]}: none of the image's five precomputed seed lists equals the "
                         "matched nodes; the reference indexes its mask list with None there (dataloader_test_sct.py:368-371) and raises TypeError")
    if mode == "gt":
        img = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(np.diff(seg), device=dev))
        sel = img * GT_LISTS + choice.long()
        obj, att, pool = subgraph_indices(gt["node_mask"].reshape(B * GT_LISTS, -1)[sel], obj_num, want_pool_mtx=want_pool_mtx)
        pred, _, _ = subgraph_indices(gt["pred_mask"].reshape(B * GT_LISTS, -1)[sel], rel_num, want_att_mask=False)
        n_off = gt["nrel_off"].to(device=dev, dtype=torch.int64)
        nrel = pad_segments(gt["nrel"], n_off[sel], n_off[sel + 1] - n_off[sel], rel_num, obj_num - 1)
    rows = {"gpn_obj_ind": (obj, False), "att_masks": (att, False), "gpn_pred_ind": (pred, False), "gpn_nrel_ind": (nrel, False)}
    if pool is not None:
        rows["gpn_pool_mtx"] = (pool, False)
    return _items(graph, rows, seg, seq_per_img, materialize), table


def assemble_test_batch(raw, obj_num, rel_num, seq_per_img=5, materialize=False, want_pool_mtx=True):
    """The plain test loader's items (dataloaders/dataloader_test.py:216-309), from the training loader's kernels alone.
    raw (on the device): the scene-graph entries of `assemble_train_batch`, optional captions [B * seq_per_img, seq_length], and every
      candidate of the images' `subgraph_mask_list[5:]` packed: cand_node_mask [sum_c, obj_num-1] u8, cand_pred_mask [sum_c, rel_num-1] u8,
      cand_off [B+1] (image b's candidates), cand_nrel [sum, 2] i64 + cand_nrel_off [sum_c + 1] i64.
    -> items: per image the first half of its candidates in the "positive" slot and the second half in the "negative" slot
       (this_mini_batch = candidates // 2, :224-230; an odd last candidate is not used), [seq_per_img, 2, this_mini_batch, ...] views."""
    n_c = int(raw["cand_node_mask"].size(0))
    seg = _host_offsets(raw["cand_off"], "cand_off", n_c)
    graph, _, _ = _graph_part(raw, obj_num, rel_num, raw.get("captions"), seq_per_img)
    if len(seg) != graph["fc_feats"].size(0) + 1:
        raise ValueError(f"assemble_test_batch: cand_off holds {len(seg)} entries for {graph['fc_feats'].size(0)} images")
    dev = graph["fc_feats"].device
    obj, att, pool = subgraph_indices(raw["cand_node_mask"], obj_num, want_pool_mtx=want_pool_mtx)
    pred, _, _ = subgraph_indices(raw["cand_pred_mask"], rel_num, want_att_mask=False)
    n_off = raw["cand_nrel_off"].to(device=dev, dtype=torch.int64)
    nrel = pad_segments(raw["cand_nrel"], n_off[:-1], n_off[1:] - n_off[:-1], rel_num, obj_num - 1)
    rows = {"gpn_obj_ind": (obj, True), "att_masks": (att, True), "gpn_pred_ind": (pred, True), "gpn_nrel_ind": (nrel, True)}
    if pool is not None:
        rows["gpn_pool_mtx"] = (pool, True)
    return _items(graph, rows, seg, seq_per_img, materialize)
