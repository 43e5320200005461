"""Grounding scores (F1_all, F1_loc) of a decode batch on the device: the Flickr30k-Entities table.

The reference finishes an evaluation run with a second program, run twice over a JSON file (misc/grounding/grounding_score.py ->
misc/grounding/eval_grd_flickr30k_entities.py `FlickrGrdEval.grd_eval(mode='all' | 'loc')`): per reference caption one Stanford CoreNLP
call per token and per predicted class word, and one `torch.Tensor` + `bbox_overlaps_batch` call per box pair.  Here everything the score
needs is on the device when the decode batch ends: `subgc_grounding_material` turns the chosen caption's tokens and arg-max nodes into the
{'clss','idx_in_sent','bbox'} list (misc/grd_utils.py:49-60) and `subgc_grounding_score` writes one byte code per precision / recall
event (lines 129-198); both are declared in include/subgc_grounding_hip.h.  Corpus numbers are formed on the host from those codes with
the reference's own expressions (`summarize`, lines 200-205), so they accumulate across batches and ranks.

`GroundingReferences` is the one-time cook (numpy allowed) of `flickr30k_cleaned_class.json`'s annotations for a split: classes, lemmas
and words become integer ids.  `lemmatize` stands where CoreNLP stands: a dict (a token it does not hold is its own lemma) or a callable;
it is asked for reference tokens and class words only, at cook time, never per batch.  `GroundingScorer.enqueue` / `unpack` and the
`grounding=` argument of `eval_glue.caption_images` are the per-batch path and issue only C-ABI launches; `score_submission` is the drop-in
for grounding_score.py on a finished `grounding_file.json`.

`gt_grd_eval` (grounding accuracy on ground-truth sentences, the evaluator's default mode) is subgc.grounding_gt: a forced decode plus
its own score kernel on these same reference tables.  Out of scope: CoreNLP itself (the controllability scores: subgc.controllability).
"""
from __future__ import annotations

import numpy as np

from . import _scoring
from ._lib import SubgcError, call_grounding
from ._scoring import csr as _csr

# the codes and limits of subgc_grounding_hip.h
MISS, HIT, SKIP, HALLUCINATED, ABSENT, NONE = 0, 1, 2, 3, 4, 255
MAX_WORDS = 64           # SUBGC_GRD_MAX_WORDS: predicted words of an image
MAX_OBJ = 64             # SUBGC_GRD_MAX_OBJ: annotated objects of a reference caption
NAMES = ("prec_all", "recall_all", "f1_all", "prec_loc", "recall_loc", "f1_loc")


def prepare_boxes(boxes, img_wh=None):
    """The detector's boxes of an image as the evaluator sees them: `boxes * max(w, h) / 592` in the array's own dtype (grd_utils.py:27),
    then -- after the JSON round trip -- rounded once to fp32 by `torch.Tensor` (eval_grd_flickr30k_entities.py:159)."""
    b = np.asarray(boxes)
    if b.ndim != 2 or b.shape[1] != 4:
        raise SubgcError(f"grounding: boxes are [n, 4], got {b.shape}")
    if img_wh is not None:
        b = b * max(img_wh) / 592
    return np.ascontiguousarray(b, dtype=np.float32)


class GroundingReferences:
    """annotations: the `annotations` list of flickr30k_cleaned_class.json ({'image_id', 'captions': [{'process_clss', 'process_idx',
    'process_bnd_box', 'tokens'}]}); split_ids: the image ids of the evaluated split(s) (`import_ref`'s filter: str(image_id) in split).
    The class list is the detection words (ascending detection id) followed by the `process_clss` words they do not hold, in first
    appearance.  `device="auto"`: the current GPU; `device=None`: the host tables only (`.to(device)` finishes the job)."""

    def __init__(self, annotations, split_ids, det_id_to_det_wd, wd_to_lemma, lemma_det_id_dict, ix_to_word, lemmatize, device="auto"):
        from .eval_glue import BAD_ENDINGS
        lem = (lambda t: lemmatize.get(t, t)) if isinstance(lemmatize, dict) else lemmatize
        split = {str(i) for i in split_ids}
        anns = [a for a in annotations if str(a["image_id"]) in split]
        det = {int(k): v for k, v in det_id_to_det_wd.items()}
        self.class_names = []
        self.class_id = {}
        for k in sorted(det):
            self._class(det[k])
        self.image_ids = [str(a["image_id"]) for a in anns]
        self.index = {}
        for j, i in enumerate(self.image_ids):
            self.index.setdefault(i, j)
        self.lemma_id = {}
        cap_n, obj_n, ex_n = [], [], []
        obj_cls, obj_idx, obj_box, ex_lemma = [], [], [], []
        self.img_classes = []
        for a in anns:
            cap_n.append(len(a["captions"]))
            seen = set()
            for s, c in enumerate(a["captions"]):
                clss, idx = list(c["process_clss"]), [int(x) for x in c["process_idx"]]
                where = f"image {a['image_id']}, caption {s}"
                if len(idx) != len(set(idx)):
                    raise SubgcError(f"grounding: a duplicate process_idx ({where}: {idx}); the reference asserts one object per word index")
                if len(clss) > MAX_OBJ:
                    raise SubgcError(f"grounding: {len(clss)} objects ({where}); the limit is {MAX_OBJ}")
                box = np.asarray(c["process_bnd_box"], np.float64)
                if len(clss) == 0 and box.size == 0:
                    box = box.reshape(0, 4)
                if box.ndim != 2 or box.shape[1] != 4 or box.shape[0] != len(clss) or len(idx) != len(clss):
                    raise SubgcError(f"grounding: process_bnd_box is [n_obj, 4] with one process_idx and process_clss per row ({where}: boxes "
                                     f"{box.shape}, {len(idx)} indices, {len(clss)} classes)")
                obj_n.append(len(clss))
                obj_cls += [self._class(w) for w in clss]
                obj_idx += idx
                obj_box.append(box.astype(np.float32))                      # `torch.Tensor(ann['process_bnd_box'])`: rounded once
                seen.update(obj_cls[len(obj_cls) - len(clss):])
                mine = set(idx)
                ex = sorted({self._lemma(lem(t)) for q, t in enumerate(c["tokens"]) if q not in mine and t != ""})
                ex_n.append(len(ex))
                ex_lemma += ex
            self.img_classes.append(sorted(seen))
        self.n_img, self.n_caps, self.n_obj = len(anns), int(sum(cap_n)), len(obj_cls)
        self.cap_off, self.obj_off, self.ex_off = _csr(cap_n), _csr(obj_n), _csr(ex_n)
        self.obj_cls, self.obj_idx = np.array(obj_cls, np.int32), np.array(obj_idx, np.int32)
        self.obj_box = np.concatenate(obj_box + [np.zeros((0, 4), np.float32)]).astype(np.float32)
        self.ex_lemma = np.array(ex_lemma, np.int32)
        self.class_lemma = np.array([self._lemma(lem(w)) for w in self.class_names], np.int32)
        self.n_class = len(self.class_names)
        V = max((int(k) for k in ix_to_word), default=0)
        self.tok_class = np.full(V + 1, -1, np.int32)
        self.bad = np.zeros(V + 1, np.uint8)
        for k, w in ix_to_word.items():
            self.bad[int(k)] = w in BAD_ENDINGS
            if w in wd_to_lemma and wd_to_lemma[w] in lemma_det_id_dict:
                self.tok_class[int(k)] = self.class_id[det[int(lemma_det_id_dict[wd_to_lemma[w]])]]
        self.device = None
        if device is not None:
            self.to(_scoring.resolve_device(device))

    def _class(self, w):
        c = self.class_id.get(w)
        if c is None:
            c = self.class_id[w] = len(self.class_names)
            self.class_names.append(w)
        return c

    def _lemma(self, l):
        return self.lemma_id.setdefault(l, len(self.lemma_id))

    def to(self, device):
        """Upload the tables; done once."""
        import torch
        dev = torch.device(device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(4 if a.ndim == 2 else 1, a.dtype)).astype(dt)).to(dev)
        self.d_tok_class, self.d_bad = up(self.tok_class, np.int32), up(self.bad, np.uint8)
        self.d_cap_off, self.d_obj_off, self.d_ex_off = up(self.cap_off, np.int32), up(self.obj_off, np.int32), up(self.ex_off, np.int32)
        self.d_obj_cls, self.d_obj_idx, self.d_obj_box = up(self.obj_cls, np.int32), up(self.obj_idx, np.int32), up(self.obj_box, np.float32)
        self.d_ex_lemma, self.d_class_lemma = up(self.ex_lemma, np.int32), up(self.class_lemma, np.int32)
        self.device = dev
        return self


class GroundingScorer:
    """`FlickrGrdEval.grd_eval` for a decode batch (both modes come out of one set of event codes).  iou_thresh: the reference's
    `--iou_thresh`, compared in fp32 like `torch.max(overlap) > self.iou_thresh`."""

    def __init__(self, refs, iou_thresh=0.5):
        self.refs, self.iou_thresh = refs, float(iou_thresh)

    def check_index(self, image_index):
        return _scoring.check_index("grounding", image_index, self.refs.n_img)

    def plan(self, image_index, counts=None):
        """The host side of a batch: which (image, caption) pairs it holds and where their events go.  counts: the predicted words of
        every image when the host knows them (`score_submission`); None: every precision slot holds MAX_WORDS codes.
        -> {"I", "P", "idx", "table" (int32: img_ref | pair_off | prec_off | rec_off, uploaded with the batch), "n_prec", "n_rec", ...}."""
        r = self.refs
        idx = np.array(self.check_index(image_index), np.int64)
        I = len(idx)
        ncap = (r.cap_off[idx + 1] - r.cap_off[idx]) if I else np.zeros(0, np.int64)
        pair_off = _csr(ncap)
        P = int(pair_off[-1])
        pair_img = np.repeat(np.arange(I), ncap)
        pair_cap = (r.cap_off[idx][pair_img] + (np.arange(P) - pair_off[pair_img])) if P else np.zeros(0, np.int64)
        rec_off = _csr(r.obj_off[pair_cap + 1] - r.obj_off[pair_cap]) if P else np.zeros(1, np.int64)
        prec_off = _csr(np.full(P, MAX_WORDS) if counts is None else np.asarray(counts, np.int64)[pair_img]) if P else np.zeros(1, np.int64)
        table = np.concatenate([idx, pair_off, prec_off, rec_off]).astype(np.int32)
        return {"I": I, "P": P, "idx": idx, "pair_off": pair_off, "prec_off": prec_off, "rec_off": rec_off, "pair_cap": pair_cap,
                "n_prec": int(prec_off[-1]), "n_rec": int(rec_off[-1]), "table": table}

    @staticmethod
    def arena_words(plan):
        """int32 words of a batch's results: count, class, word index and box (fp32) lists of every image, then the two byte buffers."""
        I = plan["I"]
        return I + 6 * I * MAX_WORDS + (plan["n_prec"] + 3) // 4 + (plan["n_rec"] + 3) // 4

    @staticmethod
    def views(arena, plan):
        """(mat_n [I], mat_cls [I, 64], mat_idx [I, 64], mat_box fp32 [I, 64, 4], prec uint8, rec uint8) views of an arena (torch or numpy)."""
        f32, u8 = (ns := _scoring.dtypes(arena)).float32, ns.uint8
        I, W = plan["I"], MAX_WORDS
        o = I
        cls = arena[o:o + I * W].reshape(I, W); o += I * W
        idx = arena[o:o + I * W].reshape(I, W); o += I * W
        box = arena[o:o + 4 * I * W].view(f32).reshape(I, W, 4); o += 4 * I * W
        wp = (plan["n_prec"] + 3) // 4
        prec = arena[o:o + wp].view(u8)[:plan["n_prec"]]; o += wp
        rec = arena[o:o + (plan["n_rec"] + 3) // 4].view(u8)[:plan["n_rec"]]
        return arena[:I], cls, idx, box, prec, rec

    def _need_device(self):
        if self.refs.device is None:
            raise SubgcError("grounding: the references are not on a device (GroundingReferences(..., device=...) or .to(device))")

    def enqueue_material(self, seq, seg, pick, I, node, T1, n_words, box_off, boxes, n_boxes, remove_bad_endings, arena, plan):
        """subgc_grounding_material on the current stream.  seq: device RANKED token rows [rows, T] (int32 / int64); seg: device int32 row
        boundaries; pick: device int32 [I] or None; node / n_words: what subgc_grounding_argmax wrote; box_off int32 [I + 1] / boxes fp32
        [n_boxes, 4]: the images' boxes on the device."""
        import torch
        from . import ops
        self._need_device()
        r = self.refs
        t64, T = _scoring.token_rows("grounding", seq, MAX_WORDS)
        rows = seq.size(0)
        if arena.numel() < self.arena_words(plan):
            raise SubgcError("grounding: the result arena is too short")
        mat_n, cls, idx, box, _, _ = self.views(arena, plan)
        bad = r.d_bad if remove_bad_endings else None
        P = ops._ptr
        call_grounding("subgc_grounding_material", P(seq), t64, int(T), P(bad, torch.uint8), 0 if bad is None else bad.numel(),
                       int(rows), P(seg, torch.int32), P(pick, torch.int32), int(I), P(node, torch.int32), int(T1), P(n_words, torch.int32),
                       P(r.d_tok_class, torch.int32), len(r.tok_class), P(box_off, torch.int32), P(boxes, torch.float32), int(n_boxes), P(mat_n),
                       P(cls), P(idx), P(box), MAX_WORDS, ops._stream())

    def enqueue_score(self, table, arena, plan):
        """subgc_grounding_score on the current stream over the lists in `arena`.  table: the device copy of plan["table"] (or a longer
        int32 tensor that starts with it)."""
        import torch
        from . import ops
        self._need_device()
        r = self.refs
        I, P_ = plan["I"], plan["P"]
        if I == 0 or P_ == 0:
            return
        mat_n, cls, _, box, prec, rec = self.views(arena, plan)
        P = ops._ptr
        t_ref, t_pair, t_prec, t_rec = table[:I], table[I:2 * I + 1], table[2 * I + 1:2 * I + P_ + 2], table[2 * I + P_ + 2:2 * I + 2 * P_ + 3]
        call_grounding("subgc_grounding_score", P(mat_n), P(cls), P(box), MAX_WORDS, int(I), P(t_ref, torch.int32), r.n_img, P(t_pair, torch.int32), int(P_),
                       P(r.d_cap_off, torch.int32), r.n_caps, P(r.d_obj_off, torch.int32), P(r.d_obj_cls, torch.int32), P(r.d_obj_idx, torch.int32),
                       P(r.d_obj_box, torch.float32), r.n_obj, P(r.d_ex_off, torch.int32), P(r.d_ex_lemma, torch.int32), len(r.ex_lemma),
                       P(r.d_class_lemma, torch.int32), r.n_class, self.iou_thresh, P(t_prec, torch.int32), P(prec) if plan["n_prec"] else None,
                       plan["n_prec"], P(t_rec, torch.int32), P(rec) if plan["n_rec"] else None, plan["n_rec"], ops._stream())

    def enqueue(self, seq, seg, pick, I, node, T1, n_words, tables, boxes, n_boxes, remove_bad_endings, arena, plan):
        """The two launches behind the grounding arg-max (`ops.eval_collect`).  tables: the device copy of plan["table"] followed by box_off."""
        n_t = len(plan["table"])
        self.enqueue_material(seq, seg, pick, I, node, T1, n_words, tables[n_t:n_t + I + 1], boxes, n_boxes, remove_bad_endings, arena, plan)
        self.enqueue_score(tables, arena, plan)

    def batch_pass(self, arg, batch, slots):
        """The grounding pass of `eval_collect` (arg: its `grounding=`), behind the grounding arg-max: the plan's table and the box offsets
        go up with the batch, the boxes in an upload of their own; reads `batch.pick` / `node` / `n_words`."""
        import torch
        from . import ops
        if not batch.ground:
            raise SubgcError("eval_collect: grounding scores need the decode loop's attention buffer (AL / idx)")
        I, plan = batch.I, self.plan(arg["index"])
        if plan["I"] != I or len(arg["boxes"]) != I:
            raise SubgcError("eval_collect: grounding needs one reference-image index and one box array per image")
        boxes = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 4) for b in arg["boxes"]]
        lens = [len(b) for b in boxes]
        n_box, s_tab, w = sum(lens), slots.ints(plan["table"].tolist() + _csr(lens).tolist()), slots.words(self.arena_words(plan))

        def enqueue():
            if I:
                d_box = ops.upload(np.concatenate(boxes).ravel() if n_box else np.zeros(4, np.float32), torch.float32, slots.arena.device)
                self.enqueue(batch.seq_s, batch.seg, batch.pick, I, batch.node, batch.T1, batch.n_words, slots.seg[s_tab], d_box, n_box,
                             arg.get("remove_bad_endings", 0), slots.arena[w], plan)

        return enqueue, lambda host: {"g_words": host[w].copy(), "g_plan": plan}

    def unpack(self, host, plan):
        """The host copy of an arena -> per image a dict of plain numpy data: "ref" (its image in the references), "clss" (class ids),
        "idx_in_sent", "bbox" (fp32 [n, 4]) -- the material -- and "precision" / "recall": int32 [events, 2] rows of (class id, code), caption
        by caption, predicted words in submission order / objects in annotation order."""
        r = self.refs
        host = np.ascontiguousarray(host)
        mat_n, cls, idx, box, prec, rec = self.views(host, plan)
        out = []
        for i in range(plan["I"]):
            n = int(mat_n[i])
            j = int(plan["idx"][i])
            pe, re_ = [], []
            for p in range(int(plan["pair_off"][i]), int(plan["pair_off"][i + 1])):
                a = int(plan["prec_off"][p])
                m = min(n, int(plan["prec_off"][p + 1]) - a)
                pe.append(np.stack([cls[i, :m], prec[a:a + m].astype(np.int32)], 1))
                s = int(plan["pair_cap"][p])
                g0, g1 = int(plan["rec_off"][p]), int(plan["rec_off"][p + 1])
                re_.append(np.stack([r.obj_cls[r.obj_off[s]:r.obj_off[s + 1]], rec[g0:g1].astype(np.int32)], 1))
            z = np.zeros((0, 2), np.int32)
            out.append({"ref": j, "clss": cls[i, :n].copy(), "idx_in_sent": idx[i, :n].copy(), "bbox": box[i, :n].copy(),
                        "precision": np.concatenate(pe + [z]).astype(np.int32), "recall": np.concatenate(re_ + [z]).astype(np.int32)})
        return out

    def empty_entry(self, ref):
        """The entry of an image without captions: nothing predicted, every object of its captions ABSENT."""
        r = self.refs
        s0, s1 = int(r.cap_off[ref]), int(r.cap_off[ref + 1])
        c = r.obj_cls[r.obj_off[s0]:r.obj_off[s1]]
        return {"ref": int(ref), "clss": np.zeros(0, np.int32), "idx_in_sent": np.zeros(0, np.int32), "bbox": np.zeros((0, 4), np.float32),
                "precision": np.zeros((0, 2), np.int32), "recall": np.stack([c, np.full(len(c), ABSENT, np.int32)], 1).astype(np.int32)}

    def score_entries(self, items, device="auto"):
        """items: [(reference image index, {'clss', 'idx_in_sent', 'bbox'})] in any order -> the per-image entries of `unpack` in that
        order.  The lists are packed on the host the way subgc_grounding_material leaves them; one launch, one host copy."""
        import torch
        r = self.refs
        if r.device is None:
            r.to(_scoring.resolve_device(device))
        I = len(items)
        host = np.zeros(I + 6 * I * MAX_WORDS, np.int32)
        mat_n, cls, widx, box, _, _ = self.views(host, {"I": I, "n_prec": 0, "n_rec": 0})
        for i, (j, e) in enumerate(items):
            n = len(e["clss"])
            if n > MAX_WORDS:
                raise SubgcError(f"grounding: reference image {j} has {n} predicted words; the limit is {MAX_WORDS}")
            b = np.asarray(e["bbox"], np.float64).reshape(-1, 4) if n else np.zeros((0, 4))
            if len(b) != n:
                raise SubgcError(f"grounding: reference image {j} has {n} classes and {len(b)} boxes")
            for q, w in enumerate(e["clss"]):
                if w not in r.class_id:
                    raise SubgcError(f"grounding: class word {w!r} (reference image {j}) is not in the cooked class list")
                cls[i, q] = r.class_id[w]
            widx[i, :n] = np.asarray(e.get("idx_in_sent", list(range(n))), np.int32)[:n]
            box[i, :n] = b.astype(np.float32)                             # `torch.Tensor(pred[img][0]['bbox'][pred_idx])`
            mat_n[i] = n
        plan = self.plan([j for j, _ in items], [len(e["clss"]) for _, e in items])
        if I == 0:
            return []
        full = np.zeros(self.arena_words(plan), np.int32)
        full[:len(host)] = host
        arena = torch.from_numpy(full).to(r.device)
        self.enqueue_score(torch.from_numpy(plan["table"]).to(r.device), arena, plan)
        return self.unpack(arena.cpu().numpy(), plan)

    def score_submission(self, results, device="auto"):
        """The drop-in for grounding_score.py: `results` = the 'results' dict of a grounding_file.json ({image id: [{'clss', 'idx_in_sent',
        'bbox'}]}, one entry per image).  Images outside the references are not looked at, like the reference; -> the per-image entries of
        `unpack`, in reference order (`summarize` makes the six numbers)."""
        r = self.refs
        picked = sorted((r.index[str(k)], k) for k in results if str(k) in r.index)
        for j, k in picked:
            if len(results[k]) != 1:
                raise SubgcError(f"grounding: image {k} has {len(results[k])} submission entries; the evaluator asserts exactly 1")
        return self.score_entries([(j, results[k][0]) for j, k in picked], device)


def chunk_arg(arg, opt, ids, sizes):
    """`caption_images(grounding=opt)`: the chunk's list-keyed argument with its boxes prepared."""
    wh = opt.get("img_wh")
    return dict(arg, boxes=[prepare_boxes(b, None if wh is None else wh[k]) for b, k in zip(arg["boxes"], ids)])


def chunk_entries(arg, h, bounds):
    """What every image's entry gains from `eval_collect`'s outputs `h` (None: a batch without rows, `empty_entry` of every image)."""
    sc = arg["scorer"]
    if h is None:
        return [{"grounding_score": sc.empty_entry(j)} for j in sc.check_index(arg["index"])]
    return [{"grounding_score": e} for e in sc.unpack(h["g_words"], h["g_plan"])]


def summarize(entries, refs):
    """Per-image entries (`GroundingScorer.unpack`, `score_submission`, or the `"grounding_score"` entries of `caption_images`) -> the six
    numbers of the two evaluator runs, exactly as lines 200-205: per class sum(hm) / len(hm), summed over the classes in their first
    appearance, divided by num_vocab; f1 is NaN when both are 0, as numpy gives.
      num_vocab counts the distinct classes of the reference captions of images that HAVE an entry (line 135's `continue` comes before
      line 143); an image of the split without an entry adds a 0 to recall for each of its objects in BOTH modes (line 187) and nothing to
      precision; a class that only ever appears hallucinated adds 0 to the sum and nothing to num_vocab.
    The images are walked in reference order whatever the order of `entries`, so batching and sharding cannot change a bit."""
    by_ref = {}
    for e in entries:
        by_ref.setdefault(int(e["ref"]), e)
    vocab = set()
    for j in by_ref:
        vocab.update(int(c) for c in refs.img_classes[j])
    num_vocab = len(vocab)
    out = {"num_vocab": num_vocab, "images": len(by_ref), "missing": refs.n_img - len(by_ref)}
    for mode in ("all", "loc"):
        prec, recall = {}, {}
        for j in range(refs.n_img):
            e = by_ref.get(j)
            if e is None:
                continue
            for c, code in np.asarray(e["precision"]).reshape(-1, 2).tolist():
                if code in (HIT, MISS) or (code == HALLUCINATED and mode == "all"):
                    prec.setdefault(c, []).append(1 if code == HIT else 0)
        for j in range(refs.n_img):
            e = by_ref.get(j)
            if e is None:
                s0, s1 = int(refs.cap_off[j]), int(refs.cap_off[j + 1])
                for c in refs.obj_cls[refs.obj_off[s0]:refs.obj_off[s1]].tolist():
                    recall.setdefault(c, []).append(0)
                continue
            for c, code in np.asarray(e["recall"]).reshape(-1, 2).tolist():
                if code in (HIT, MISS) or (code == ABSENT and mode == "all"):
                    recall.setdefault(c, []).append(1 if code == HIT else 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.sum([sum(hm) * 1. / len(hm) for hm in prec.values()]) * 1. / np.float64(num_vocab)
            r = np.sum([sum(hm) * 1. / len(hm) for hm in recall.values()]) * 1. / np.float64(num_vocab)
            f1 = 2. * p * r / (p + r)
        out["prec_" + mode], out["recall_" + mode], out["f1_" + mode] = float(p), float(r), float(f1)
        out["per_class_" + mode] = {"precision": {refs.class_names[c]: hm for c, hm in prec.items()},
                                    "recall": {refs.class_names[c]: hm for c, hm in recall.items()}}
    return out
