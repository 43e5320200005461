"""Grounding accuracy on ground-truth sentences on the device: `FlickrGrdEval.gt_grd_eval`
(misc/grounding/eval_grd_flickr30k_entities.py:63-109), the evaluator's default mode (`--eval_mode GT`, line 246).

The reference decodes every reference caption of an image teacher-forced, writes for every word the box of the node it attended to most
into `grounding_file.json` ({image id: five {'idx_in_sent', 'bbox'} lists}), and a second program compares, for every annotated object,
the box at the object's word index with the object's box.  Here `forced.forced_decode(return_att=True)` is the teacher-forced pass,
`subgc_grounding_argmax` (one row per "image") the arg-max, `subgc_gt_grounding_material` the lists and `subgc_gt_grounding_score` one
byte per annotated object (include/subgc_forced_hip.h); `eval_glue.ground_gt_images` runs the four in one pass with one host copy per
batch.  The corpus number (line 97) is formed on the host from those codes with the reference's own expression (`summarize`), so it
accumulates across batches and ranks.

`GtCaptionRows` builds the token rows: position j of a row is annotation word j, so `process_idx` addresses both.  `GtGroundingScorer`
reads the tables of `grounding.GroundingReferences` (caption and object offsets, `process_idx`, `process_bnd_box`, classes); the list form
is the score kernel's input, so a finished GT-mode `grounding_file.json` goes through the same launch (`score_submission`).
`restatement` is the contract in numpy, for tests and for reading.
"""
from __future__ import annotations

import numpy as np

from . import _scoring
from ._lib import SubgcError, call_forced
from ._scoring import csr as _csr

# the codes and limits of subgc_forced_hip.h
MISS, HIT, UNGROUNDED, NOROW, NONE = 0, 1, 2, 3, 255
MAX_WORDS = 64           # SUBGC_FORCED_MAX_T: entries of a list
MAX_OBJ = 64             # SUBGC_GTG_MAX_OBJ: annotated objects of a reference caption
N_SENT = 5               # "Each image must have five caption predictions!" (line 84-85)


class GtCaptionRows:
    """Token rows of the reference captions of a split.  annotations / split_ids: as `GroundingReferences` takes them (the same filter
    and order, so image j here is image j there); ix_to_word: {id: word}; unk: the id (or the word) unknown and empty tokens map to.
    Row s of an image holds caption s: column j = the id of `tokens[j]` for j < min(len(tokens), seq_length), then zeros; seq_length + 1
    columns, so the end token of a full-length caption is scored as LanguageModelCriterion scores it."""

    def __init__(self, annotations, split_ids, ix_to_word, seq_length, unk):
        w2i = {w: int(k) for k, w in ix_to_word.items()}
        if isinstance(unk, str):
            if unk not in w2i:
                raise SubgcError(f"gt caption rows: the unknown word {unk!r} is not in the vocabulary")
            unk = w2i[unk]
        self.unk, self.seq_length = int(unk), int(seq_length)
        if not 1 <= self.seq_length < MAX_WORDS:
            raise SubgcError(f"gt caption rows: 1 <= seq_length <= {MAX_WORDS - 1} (got {seq_length}); a forced row holds seq_length + 1 columns")
        split = {str(i) for i in split_ids}
        self.image_ids, self.index, self._rows = [], {}, []
        for a in annotations:
            if str(a["image_id"]) not in split:
                continue
            rows = np.zeros((len(a["captions"]), self.seq_length + 1), np.int64)
            for s, c in enumerate(a["captions"]):
                for j, t in enumerate(c["tokens"][:self.seq_length]):
                    rows[s, j] = w2i.get(t, self.unk) if t != "" else self.unk
                if (rows[s, :min(len(c["tokens"]), self.seq_length)] <= 0).any():
                    raise SubgcError(f"gt caption rows: image {a['image_id']}, caption {s}: a word maps to id 0, the end token")
            self.index.setdefault(str(a["image_id"]), len(self.image_ids))
            self.image_ids.append(str(a["image_id"]))
            self._rows.append(rows)

    def rows_of(self, image_id):
        """int64 [captions, seq_length + 1] of an image of the split."""
        j = self.index.get(str(image_id))
        if j is None:
            raise SubgcError(f"gt caption rows: image {image_id!r} is not in the split")
        return self._rows[j]

    __getitem__ = rows_of


def iou_f32(p, g):
    """bbox_overlaps_batch for N = K = 1 (bbox_transform.py:194-220) in fp32, every operation rounded on its own: the device function."""
    f = np.float32
    p, g = [f(x) for x in p], [f(x) for x in g]
    one = f(1)
    gx, gy = f(f(g[2] - g[0]) + one), f(f(g[3] - g[1]) + one)
    ga = f(gx * gy)
    px, py = f(f(p[2] - p[0]) + one), f(f(p[3] - p[1]) + one)
    pa = f(px * py)
    iw = f(f(min(p[2], g[2]) - max(p[0], g[0])) + one)
    iw = f(0) if iw < 0 else iw
    ih = f(f(min(p[3], g[3]) - max(p[1], g[1])) + one)
    ih = f(0) if ih < 0 else ih
    inter = f(iw * ih)
    ua = f(f(pa + ga) - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        ov = f(inter / ua)
    if gx == one and gy == one:
        ov = f(0)
    if px == one and py == one:
        ov = f(-1)
    return ov


def restatement(lists, pair_cap, pair_row, obj_off, obj_idx, obj_box, iou_thresh=0.5):
    """subgc_gt_grounding_score in numpy.  lists: per row (idx_in_sent, bbox [n, 4]); -> one uint8 array of codes per pair."""
    thr = np.float32(iou_thresh)
    out = []
    for s, r in zip(pair_cap, pair_row):
        q0, q1 = int(obj_off[s]), int(obj_off[s + 1])
        codes = np.full(q1 - q0, NONE, np.uint8)
        for k in range(min(q1 - q0, MAX_OBJ)):
            if r < 0:
                codes[k] = NOROW
                continue
            idx = [int(x) for x in lists[r][0]][:MAX_WORDS]
            want = int(obj_idx[q0 + k])
            if want not in idx:
                codes[k] = UNGROUNDED
                continue
            ov = iou_f32(np.asarray(lists[r][1], np.float32).reshape(-1, 4)[idx.index(want)], obj_box[q0 + k])
            codes[k] = HIT if ov > thr else MISS
        out.append(codes)
    return out


class GtGroundingScorer:
    """`FlickrGrdEval.gt_grd_eval` for batches of forced rows.  refs: `grounding.GroundingReferences` of the split; iou_thresh: the
    reference's `--iou_thresh`, compared in fp32 like `torch.max(overlap) > self.iou_thresh`."""

    def __init__(self, refs, iou_thresh=0.5):
        self.refs, self.iou_thresh = refs, float(iou_thresh)

    def check_index(self, image_index):
        return _scoring.check_index("gt grounding", image_index, self.refs.n_img)

    def plan(self, image_index, rows_per_image, has_rows=None):
        """The host side of a batch.  image_index: the reference image of every batch image; rows_per_image: the forced rows it brings,
        exactly one per reference caption; has_rows (optional, `score_submission`): False for an image without rows, whose pairs get no
        row.  -> {"I", "P", "rows", "idx", "pair_off", "pair_cap", "pair_row", "out_off", "n_out", "table" (int32: pair_cap | pair_row |
        out_off, uploaded with the batch)}."""
        r = self.refs
        idx = np.array(self.check_index(image_index), np.int64)
        I = len(idx)
        counts = np.asarray(list(rows_per_image), np.int64)
        if len(counts) != I:
            raise SubgcError("gt grounding: one row count per batch image")
        ncap = (r.cap_off[idx + 1] - r.cap_off[idx]) if I else np.zeros(0, np.int64)
        has = np.ones(I, bool) if has_rows is None else np.asarray(list(has_rows), bool)
        for i in range(I):
            if has[i] and counts[i] != ncap[i]:
                raise SubgcError(f"gt grounding: batch image {i} (reference image {idx[i]}, id {r.image_ids[idx[i]]}) brings {counts[i]} rows and has "
                                 f"{ncap[i]} reference captions; a row per caption")
        row_off = _csr(np.where(has, counts, 0))
        pair_off = _csr(ncap)
        P = int(pair_off[-1])
        pair_img = np.repeat(np.arange(I), ncap)
        local = (np.arange(P) - pair_off[pair_img]) if P else np.zeros(0, np.int64)
        pair_cap = (r.cap_off[idx][pair_img] + local) if P else np.zeros(0, np.int64)
        pair_row = np.where(has[pair_img], row_off[pair_img] + local, -1) if P else np.zeros(0, np.int64)
        out_off = _csr(r.obj_off[pair_cap + 1] - r.obj_off[pair_cap]) if P else np.zeros(1, np.int64)
        table = np.concatenate([pair_cap, pair_row, out_off]).astype(np.int32)
        return {"I": I, "P": P, "rows": int(row_off[-1]), "idx": idx, "pair_off": pair_off, "pair_cap": pair_cap, "pair_row": pair_row,
                "row_off": row_off, "out_off": out_off, "n_out": int(out_off[-1]), "table": table}

    @staticmethod
    def arena_words(plan):
        """int32 words of a batch's results: count, word index and box (fp32) lists of every row, then the code bytes."""
        return plan["rows"] + 5 * plan["rows"] * MAX_WORDS + (plan["n_out"] + 3) // 4

    @staticmethod
    def views(arena, plan):
        """(mat_n [rows], mat_idx [rows, 64], mat_box fp32 [rows, 64, 4], codes uint8 [n_out]) views of an arena (torch or numpy)."""
        f32, u8 = (ns := _scoring.dtypes(arena)).float32, ns.uint8
        R, W = plan["rows"], MAX_WORDS
        o = R
        idx = arena[o:o + R * W].reshape(R, W); o += R * W
        box = arena[o:o + 4 * R * W].view(f32).reshape(R, W, 4); o += 4 * R * W
        codes = arena[o:o + (plan["n_out"] + 3) // 4].view(u8)[:plan["n_out"]]
        return arena[:R], idx, box, codes

    def _need_device(self):
        if self.refs.device is None:
            raise SubgcError("gt grounding: the references are not on a device (GroundingReferences(..., device=...) or .to(device))")

    def enqueue_material(self, node, T1, n_words, row_img, box_off, n_img, boxes, n_boxes, arena, plan):
        """subgc_gt_grounding_material on the current stream.  node int32 [rows, T1] / n_words int32 [rows]: what subgc_grounding_argmax
        wrote with one row per "image"; row_img int32 [rows]; box_off int32 [n_img + 1] / boxes fp32 [n_boxes, 4] on the device."""
        import torch
        from . import ops
        if arena.numel() < self.arena_words(plan):
            raise SubgcError("gt grounding: the result arena is too short")
        mat_n, idx, box, _ = self.views(arena, plan)
        P = ops._ptr
        call_forced("subgc_gt_grounding_material", P(node, torch.int32), int(T1), P(n_words, torch.int32), plan["rows"], P(row_img, torch.int32),
                    P(box_off, torch.int32), int(n_img), P(boxes, torch.float32), int(n_boxes), P(mat_n), P(idx), P(box), MAX_WORDS, ops._stream())

    def enqueue_score(self, table, arena, plan):
        """subgc_gt_grounding_score on the current stream over the lists in `arena`.  table: the device copy of plan["table"] (or a
        longer int32 tensor that starts with it)."""
        import torch
        from . import ops
        self._need_device()
        r = self.refs
        P_ = plan["P"]
        if P_ == 0:
            return
        if arena.numel() < self.arena_words(plan):
            raise SubgcError("gt grounding: the result arena is too short")
        mat_n, idx, box, codes = self.views(arena, plan)
        P = ops._ptr
        have = plan["rows"] > 0
        call_forced("subgc_gt_grounding_score", P(mat_n) if have else None, P(idx) if have else None, P(box) if have else None, MAX_WORDS,
                    plan["rows"], P(table[:P_], torch.int32), P(table[P_:2 * P_], torch.int32), int(P_), P(r.d_obj_off, torch.int32), r.n_caps,
                    P(r.d_obj_idx, torch.int32), P(r.d_obj_box, torch.float32), r.n_obj, self.iou_thresh, P(table[2 * P_:3 * P_ + 1], torch.int32),
                    P(codes) if plan["n_out"] else None, plan["n_out"], ops._stream())

    def enqueue(self, node, T1, n_words, tables, n_img, boxes, n_boxes, arena, plan):
        """The two launches behind the arg-max.  tables: the device copy of plan["table"] followed by row_img [rows] and box_off
        [n_img + 1]."""
        n_t, R = len(plan["table"]), plan["rows"]
        if R:
            self.enqueue_material(node, T1, n_words, tables[n_t:n_t + R], tables[n_t + R:n_t + R + n_img + 1], n_img, boxes, n_boxes, arena, plan)
        self.enqueue_score(tables, arena, plan)

    def unpack(self, host, plan):
        """The host copy of an arena -> per batch image a dict of plain numpy data: "ref" (its image in the references), "image_id" (the
        references' id string), "rows": per reference caption {"idx_in_sent", "bbox" fp32 [n, 4]} (None for an image without rows) and
        "events": int32 [objects, 2] rows of (class id, code), caption by caption, objects in annotation order."""
        r = self.refs
        host = np.ascontiguousarray(host)
        mat_n, idx, box, codes = self.views(host, plan)
        out = []
        for i in range(plan["I"]):
            ev, rows = [], []
            for p in range(int(plan["pair_off"][i]), int(plan["pair_off"][i + 1])):
                s, g0, g1 = int(plan["pair_cap"][p]), int(plan["out_off"][p]), int(plan["out_off"][p + 1])
                ev.append(np.stack([r.obj_cls[r.obj_off[s]:r.obj_off[s + 1]], codes[g0:g1].astype(np.int32)], 1))
                q = int(plan["pair_row"][p])
                if q >= 0:
                    n = int(mat_n[q])
                    rows.append({"idx_in_sent": idx[q, :n].copy(), "bbox": box[q, :n].copy()})
            j = int(plan["idx"][i])
            out.append({"ref": j, "image_id": r.image_ids[j], "rows": rows if rows or plan["pair_off"][i] == plan["pair_off"][i + 1] else None,
                        "events": np.concatenate(ev + [np.zeros((0, 2), np.int32)]).astype(np.int32)})
        return out

    def score_lists(self, items, device="auto"):
        """items: [(reference image index, its list of {'idx_in_sent', 'bbox'} dicts -- one per reference caption -- or None: no rows)]
        -> the per-image entries of `unpack` in that order.  The lists are packed on the host the way subgc_gt_grounding_material leaves
        them; one launch, one host copy."""
        import torch
        r = self.refs
        if r.device is None:
            r.to(_scoring.resolve_device(device))
        flat = []
        for j, lst in items:
            for e in (lst or []):
                n = len(e["idx_in_sent"])
                if n > MAX_WORDS:
                    raise SubgcError(f"gt grounding: reference image {j} has a list of {n} entries; the limit is {MAX_WORDS}")
                b = np.asarray(e["bbox"], np.float64).reshape(-1, 4) if n else np.zeros((0, 4))
                if len(b) != n:
                    raise SubgcError(f"gt grounding: reference image {j} has {n} word indices and {len(b)} boxes")
                flat.append((np.asarray(e["idx_in_sent"], np.int64), b.astype(np.float32)))       # `torch.Tensor(...['bbox'][pred_ind])`
        plan = self.plan([j for j, _ in items], [len(lst or []) for _, lst in items], [lst is not None for _, lst in items])
        if plan["P"] == 0:
            return self.unpack(np.zeros(self.arena_words(plan), np.int32), plan)
        host = np.zeros(self.arena_words(plan), np.int32)
        mat_n, widx, box, _ = self.views(host, plan)
        for q, (ix, b) in enumerate(flat):
            mat_n[q] = len(ix)
            widx[q, :len(ix)] = ix
            box[q, :len(ix)] = b
        arena = torch.from_numpy(host).to(r.device)
        self.enqueue_score(torch.from_numpy(plan["table"]).to(r.device), arena, plan)
        return self.unpack(arena.cpu().numpy(), plan)

    def score_submission(self, results, device="auto"):
        """The drop-in for `grounding_score.py --eval_mode GT` on a finished grounding_file.json: `results` = its 'results' dict ({image
        id: five {'idx_in_sent', 'bbox'} lists}).  Every image of the split gets an entry, in reference order; an image absent from the
        submission is "not grounded" (NOROW); images outside the split are not looked at.  Raises the reference's own exception where the
        reference raises it: at the first annotated object of an image whose submission does not hold five lists."""
        r = self.refs
        by_id = {str(k): v for k, v in results.items()}
        items = []
        for j, img in enumerate(r.image_ids):
            s0, s1 = int(r.cap_off[j]), int(r.cap_off[j + 1])
            if img not in by_id:
                items.append((j, None))
                continue
            pred = by_id[img]
            if r.obj_off[s1] > r.obj_off[s0] and len(pred) != N_SENT:
                raise Exception("Each image must have five caption predictions!")
            if s1 - s0 > len(pred):
                raise SubgcError(f"gt grounding: image {img} has {s1 - s0} reference captions and {len(pred)} submission lists")
            items.append((j, list(pred[:s1 - s0])))
        return self.score_lists(items, device)


def summarize(entries, refs):
    """Per-image entries (`GtGroundingScorer.unpack` / `score_lists` / `score_submission`, or the `"gt_grounding"` entries of
    `eval_glue.ground_gt_images`) -> {"grd_accu", "n_classes", "per_class": {class word: (hits, count)}} as line 97 forms it:
    `np.mean([sum(hm) * 1. / len(hm) for hm in results.values()])` with the classes in first appearance.  The images are walked in
    reference order whatever the order of `entries`, so batching and sharding cannot change a bit; an image of the split without an
    entry is "not grounded": a 0 for each of its objects (lines 82-83)."""
    by_ref = {}
    for e in entries:
        by_ref.setdefault(int(e["ref"]), e)
    results = {}
    for j in range(refs.n_img):
        e = by_ref.get(j)
        if e is None:
            s0, s1 = int(refs.cap_off[j]), int(refs.cap_off[j + 1])
            for c in refs.obj_cls[refs.obj_off[s0]:refs.obj_off[s1]].tolist():
                results.setdefault(c, []).append(0)
            continue
        for c, code in np.asarray(e["events"]).reshape(-1, 2).tolist():
            if code != NONE:
                results.setdefault(c, []).append(1 if code == HIT else 0)
    accu = np.mean([sum(hm) * 1. / len(hm) for hm in results.values()]) if results else np.float64("nan")   # (an empty split: the reference's NaN)
    return {"grd_accu": float(accu), "n_classes": len(results),
            "per_class": {refs.class_names[c]: (int(sum(hm)), len(hm)) for c, hm in results.items()}}


def to_submission(entries, refs=None):
    """Entries with rows (`unpack`'s, which carry "image_id"; entries without one need `refs`) -> the dict the reference evaluator reads:
    {"results": {image id: five {'idx_in_sent', 'bbox'} lists}}; an image with fewer than five reference captions is padded with empty
    lists (the evaluator asks for five and reads one per caption)."""
    out = {}
    for e in entries:
        if e.get("rows") is None:
            continue
        lst = [{"idx_in_sent": [int(x) for x in r_["idx_in_sent"]], "bbox": [[float(v) for v in b] for b in r_["bbox"]]} for r_ in e["rows"]]
        if len(lst) > N_SENT:
            raise SubgcError(f"gt grounding: reference image {e['ref']} has {len(lst)} rows; the evaluator reads five lists per image")
        img = str(e["image_id"]) if "image_id" in e else refs.image_ids[int(e["ref"])]
        out[img] = lst + [{"idx_in_sent": [], "bbox": []} for _ in range(N_SENT - len(lst))]
    return {"results": out}
