#!/usr/bin/env python
"""Write the GT-sentence grounding fixture by RUNNING THE REFERENCE's own evaluator where the reference lies (never copied):
grounding_gt_case.npz + grounding_gt_meta.json.  Data only: fabricated annotations and GT-mode submissions as arrays, the expected event
codes, the per-class lists and the number `FlickrGrdEval.gt_grd_eval` returned.

    python tests/golden/make_golden_grounding_gt.py

The arrangement is make_golden_grounding.py's (imported, not repeated: the stand-in `stanfordcorenlp` module, the synthetic word world,
`misc/grounding` first on sys.path): the evaluator runs unmodified on temporary reference / split / submission JSON files and its
`results` dictionary (per class the list of 0 / 1 it averaged) is captured from `gt_grd_eval`'s frame when it returns (sys.setprofile).
The expected codes are derived here -- list look-ups and the reference's own `bbox_overlaps_batch` on `torch.Tensor` boxes -- and then
CHECKED against the captured dictionary: replaying the codes in the evaluator's order must rebuild every per-class list, or this script
fails.

Sets: `rnd` (random, 30 images x up to 5 captions), `edge` (the planted cases; see `edges` in the meta), `bad5` (the edge annotations
with one image's submission cut to four lists: the evaluator's own exception, whose text is stored) and, when forced_case.npz exists,
`model`: the arg-max boxes of the reference model's teacher-forced pass (make_golden_forced.py) against fabricated annotations."""
import contextlib
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_grounding as M                                      # noqa: E402

REF = M.REF
MISS, HIT, UNGROUNDED, NOROW = 0, 1, 2, 3


def run_reference(tmp, anns, split_ids, results):
    """-> (grd_accu, {class: [0 / 1, ...]} in the evaluator's order) from the evaluator itself."""
    from eval_grd_flickr30k_entities import FlickrGrdEval
    paths = [os.path.join(tmp, n) for n in ("reference.json", "split.json", "submission.json")]
    for p, obj in zip(paths, ({"annotations": anns}, {"val": [str(i) for i in split_ids]}, {"results": results})):
        with open(p, "w") as f:
            json.dump(obj, f)
    ev = FlickrGrdEval(reference_file=paths[0], submission_file=paths[2], split_file=paths[1], val_split=["val"], iou_thresh=0.5)
    got = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "gt_grd_eval" and "results" in frame.f_locals:
            got["results"] = [(k, list(v)) for k, v in frame.f_locals["results"].items()]
    sys.setprofile(prof)
    try:
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            accu = ev.gt_grd_eval()
    finally:
        sys.setprofile(None)
    assert isinstance(accu, np.float64), type(accu)
    return float(accu), got["results"]


def expected_codes(anns, split, results, thresh=0.5):
    """Per split image in reference order: (image id, [(class word, code)] caption by caption, objects in annotation order)."""
    out = []
    for a in anns:
        img = str(a["image_id"])
        if img not in split:
            continue
        ev = []
        for s, c in enumerate(a["captions"]):
            for q, w in enumerate(c["process_clss"]):
                if img not in results:
                    ev.append((w, NOROW))
                    continue
                lst = results[img][s]
                idx = c["process_idx"][q]
                if idx not in lst["idx_in_sent"]:
                    ev.append((w, UNGROUNDED))
                    continue
                k = lst["idx_in_sent"].index(idx)
                ev.append((w, HIT if M.overlap(lst["bbox"][k], c["process_bnd_box"][q]) > thresh else MISS))
        out.append((a["image_id"], ev))
    return out


def replay(codes):
    res = {}
    for _, ev in codes:
        for w, code in ev:
            res.setdefault(w, []).append(1 if code == HIT else 0)
    return [(k, v) for k, v in res.items()]


def store_annotations(arr, words, tag, anns, split_ids):
    i64 = lambda x: np.asarray(x, np.int64)
    caps = [c for a in anns for c in a["captions"]]
    arr[tag + "_img_ids"], arr[tag + "_split"] = i64([a["image_id"] for a in anns]), i64(list(split_ids))
    arr[tag + "_cap_off"] = i64(np.concatenate([[0], np.cumsum([len(a["captions"]) for a in anns])]))
    arr[tag + "_tok_off"] = i64(np.concatenate([[0], np.cumsum([len(c["tokens"]) for c in caps])]))
    arr[tag + "_tok"] = np.asarray([words(t) for c in caps for t in c["tokens"]], np.int32)
    arr[tag + "_obj_off"] = i64(np.concatenate([[0], np.cumsum([len(c["process_clss"]) for c in caps])]))
    arr[tag + "_obj_cls"] = np.asarray([words(w) for c in caps for w in c["process_clss"]], np.int32)
    arr[tag + "_obj_idx"] = np.asarray([q for c in caps for q in c["process_idx"]], np.int32)
    arr[tag + "_obj_box"] = np.asarray([b for c in caps for b in c["process_bnd_box"]], np.float64).reshape(-1, 4)


def store_submission(arr, tag, results):
    i64 = lambda x: np.asarray(x, np.int64)
    subs = list(results.items())
    lists = [l for _, v in subs for l in v]
    arr[tag + "_sub_ids"] = i64([int(k) for k, _ in subs])
    arr[tag + "_sub_list_off"] = i64(np.concatenate([[0], np.cumsum([len(v) for _, v in subs])]))
    arr[tag + "_sub_ent_off"] = i64(np.concatenate([[0], np.cumsum([len(l["idx_in_sent"]) for l in lists])]))
    arr[tag + "_sub_idx"] = np.asarray([q for l in lists for q in l["idx_in_sent"]], np.int32)
    arr[tag + "_sub_box"] = np.asarray([b for l in lists for b in l["bbox"]], np.float64).reshape(-1, 4)


def record(arr, meta, words, tag, tmp, anns, split_ids, results):
    split = {str(i) for i in split_ids}
    accu, ref = run_reference(tmp, anns, split_ids, results)
    codes = expected_codes(anns, split, results)
    assert replay(codes) == ref, (tag, "the derived codes do not rebuild the evaluator's lists")
    assert accu == float(np.mean([sum(hm) * 1. / len(hm) for _, hm in ref]))
    store_annotations(arr, words, tag, anns, split_ids)
    store_submission(arr, tag, results)
    arr[tag + "_ent_ids"] = np.asarray([i for i, _ in codes], np.int64)
    arr[tag + "_code_off"] = np.asarray(np.concatenate([[0], np.cumsum([len(ev) for _, ev in codes])]), np.int64)
    arr[tag + "_code_cls"] = np.asarray([words(w) for _, ev in codes for w, _ in ev], np.int32)
    arr[tag + "_code"] = np.asarray([c for _, ev in codes for _, c in ev], np.uint8)
    arr[tag + "_accu"] = np.asarray([accu], np.float64)
    meta["sets"][tag] = {"annotations": tag, "n_classes": len(ref), "per_class": [[k, v] for k, v in ref],
                         "code_counts": [int(sum(1 for _, ev in codes for _, c in ev if c == v)) for v in range(4)]}
    return accu, ref, codes


def lst(entries):
    """entries: [(word index, box)]."""
    return {"idx_in_sent": [int(e[0]) for e in entries], "bbox": [[float(x) for x in e[1]] for e in entries]}


def rnd_box(rng):
    x1, y1 = rng.random(2) * 200
    w, h = 5 + rng.random(2) * 150
    return [x1, y1, x1 + w, y1 + h] if rng.random() < 0.7 else [round(x1), round(y1), round(x1 + w), round(y1 + h)]


def random_set(rng):
    anns, results = [], {}
    for i in range(30):
        img = 6000 + i
        caps = []
        for _ in range(int(rng.integers(1, 6))):
            n_tok = int(rng.integers(4, 15))
            toks = [M.FILL[int(rng.integers(len(M.FILL)))] if rng.random() > 0.1 else "" for _ in range(n_tok)]
            pos = rng.permutation(n_tok)[:int(rng.integers(0, 5))]
            caps.append(M.cap(toks, [(M.CLASSES[int(rng.integers(len(M.CLASSES)))], int(q), rnd_box(rng)) for q in pos]))
        anns.append({"image_id": img, "captions": caps})
        if rng.random() < 0.1:
            continue                                                        # not in the submission: "image not grounded"
        lists = []
        for s in range(5):
            c = caps[s] if s < len(caps) else None
            n_tok = len(c["tokens"]) if c else int(rng.integers(3, 9))
            gt = dict(zip(c["process_idx"], c["process_bnd_box"])) if c else {}
            ents = []
            for j in range(n_tok):
                if rng.random() < 0.12:
                    continue                                                # a word the row does not ground
                if j in gt:
                    b, u = gt[j], rng.random()
                    if u < 0.4:
                        box = list(b)
                    elif u < 0.7:
                        d = (rng.random(4) - 0.5) * 40
                        box = [b[0] + d[0], b[1] + d[1], b[2] + d[2], b[3] + d[3]]
                    elif u < 0.85:
                        box = [b[0], b[1], b[0] + (b[2] - b[0]) * 0.4, b[3]]
                    else:
                        box = rnd_box(rng)
                else:
                    box = rnd_box(rng)
                ents.append((j, box))
                if rng.random() < 0.05:
                    ents.append((j, rnd_box(rng)))                          # the index a second time: the first wins
            lists.append(lst(ents))
        results[str(img)] = lists
    return anns, [a["image_id"] for a in anns], results


def edge_set():
    edges = {}
    big = [0, 0, 9, 9]
    y, k = np.float32(4), 0
    while True:                                                             # the nearest hit above the exact 0.5
        y = np.nextafter(y, np.float32(np.inf)); k += 1
        if M.overlap([0, 0, 9, float(y)], big) > 0.5:
            break
    assert M.overlap([0, 0, 9, 4], big) == 0.5
    plain, other = [10.5, 20.25, 110.75, 220.5], [300, 300, 340, 350]
    b2, b5 = [0, 0, 50, 50], [100, 100, 160, 170]
    empty = lst([])
    # image 8000: ONE reference caption (fewer than five), every box case at its own word
    boxes = [("c1", [0, 0, 9, 4], big, MISS, "iou_exactly_at_the_threshold"), ("c2", [0, 0, 9, float(y)], big, HIT, "nearest_hit"),
             ("c4", big, [5, 5, 5, 5], MISS, "gt_box_w_h_1"), ("c5", [5, 5, 5, 5], big, MISS, "pred_box_w_h_1"),
             ("c6", [5, 5, 5, 5], [5, 5, 5, 5], MISS, "both_w_h_1"), ("x1", plain, plain, HIT, "identical")]
    a0 = {"image_id": 8000, "captions": [M.cap([w for w, *_ in boxes] + ["t1"], [(w, q, gt) for q, (w, _, gt, _, _) in enumerate(boxes)])]}
    r0 = [lst([(q, pr) for q, (_, pr, _, _, _) in enumerate(boxes)] + [(len(boxes), plain)])] + [lst([(0, plain)]), empty, empty, empty]
    for q, (w, pr, gt, code, name) in enumerate(boxes):
        assert (M.overlap(pr, gt) > 0.5) == (code == HIT), name
        edges[name] = {"image": 8000, "event": q, "code": code}
    edges["nearest_hit"]["ulps_above"] = k
    edges["fewer_than_five_reference_captions"] = 8000
    # image 8001: in the split, absent from the submission
    a1 = {"image_id": 8001, "captions": [M.cap(["x2", "t1", "x2"], [("x2", 0, b2), ("x2", 2, b5)]), M.cap(["t2", "c1"], [("c1", 1, b2)])]}
    edges["image_absent_from_the_submission"] = {"image": 8001, "codes": [NOROW, NOROW, NOROW]}
    # image 8002: a missing index, a duplicate index (first wins, both ways round), an index beyond the sentence
    a2 = {"image_id": 8002, "captions": [
        M.cap(["t1", "c1", "t2", "c2", "c3", "t3"], [("c1", 1, b2), ("c2", 3, b5), ("c3s", 4, b2), ("c7s", 40, b2)]),
        M.cap(["c1", "t1"], [("c1", 0, b5)]), M.cap(["t1"], []), M.cap(["t1", "c2"], [("c2", 1, plain)]), M.cap(["c8"], [("c8", 0, plain)])]}
    r2 = [lst([(0, plain), (3, b5), (3, b2), (4, b5), (4, b2), (5, plain)]),        # 1 missing; 3: first hits; 4: first misses; 40 beyond
          lst([(0, b5), (1, b2)]), lst([(0, plain)]), lst([(1, other), (0, plain)]), empty]
    edges["index_missing_duplicate_and_beyond"] = {"image": 8002, "codes": [UNGROUNDED, HIT, MISS, UNGROUNDED, HIT, MISS, UNGROUNDED],
                                                   "note": "caption 0: word 1 not grounded; word 3 listed twice, the first box hits; word 4 "
                                                           "listed twice, the first box misses; word 40 lies beyond the sentence"}
    edges["caption_without_objects"] = {"image": 8002, "caption": 2}
    # image 8003: one caption without objects and a submission of TWO lists: the evaluator never reaches its length check
    a3 = {"image_id": 8003, "captions": [M.cap(["t1", "t2"], [])]}
    r3 = [lst([(0, plain)]), empty]
    edges["no_objects_and_not_five_lists_does_not_raise"] = 8003
    # image 8004: annotated and submitted, outside the split; 8999: submitted, not annotated
    a4 = {"image_id": 8004, "captions": [M.cap(["c1"], [("c1", 0, b2)])]}
    edges["submission_image_outside_the_split"], edges["submitted_but_not_annotated"] = 8004, 8999
    anns = [a0, a1, a2, a3, a4]
    results = {"8000": r0, "8002": r2, "8003": r3, "8004": [lst([(0, b2)])] * 5, "8999": [lst([(0, b2)])] * 5}
    return anns, [8000, 8001, 8002, 8003], results, edges


def model_set(arr, meta, words, tmp):
    """The arg-max boxes of the reference model's teacher-forced pass (forced_case.npz) against fabricated annotations."""
    path = os.path.join(HERE, "forced_case.npz")
    if not os.path.exists(path):
        return False
    with np.load(path) as z:
        f = {k: z[k] for k in z.files}
    tok, node, bounds, boxes, box_off = f["subgc_tokens"], f["subgc_node"], f["subgc_bounds"], f["subgc_boxes"], f["subgc_box_off"]
    anns, results = [], {}
    for i in range(len(bounds) - 1):
        img = 5000 + i
        caps, lists = [], []
        for s, r in enumerate(range(bounds[i], bounds[i + 1])):
            n = int((np.cumprod(tok[r] > 0)).sum())
            b = boxes[box_off[i]:box_off[i + 1]]
            ents = [(j, b[node[r, j]].tolist()) for j in range(n)]
            objs = []
            for q, j in enumerate(range(s % 2, n, 2)):                      # every other word is an object
                bx = list(ents[j][1])
                if q % 3 == 1:
                    bx = [bx[0] + 40, bx[1] + 40, bx[2] + 90, bx[3] + 90]
                objs.append((M.CLASSES[(i + s + q) % len(M.CLASSES)], j, bx))
            if s == 0:
                objs.append(("x2", n + 3, [1, 2, 30, 40]))                  # beyond the sentence
            caps.append(M.cap(["t%d" % (1 + (j % 30)) for j in range(n)], objs))
            lists.append(lst(ents))
        anns.append({"image_id": img, "captions": caps})
        results[str(img)] = lists
    record(arr, meta, words, "model", tmp, anns, [a["image_id"] for a in anns], results)
    return True


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    arr, words = {}, M.Words()
    meta = {"det_id_to_det_wd": {str(k): v for k, v in M.DET.items()}, "extra_classes": M.EXTRA, "lemma": M.LEMMA, "classes": M.CLASSES,
            "codes": {"MISS": MISS, "HIT": HIT, "UNGROUNDED": UNGROUNDED, "NOROW": NOROW}, "iou_thresh": 0.5, "sets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "stub"))
        with open(os.path.join(tmp, "stub", "stanfordcorenlp.py"), "w") as f:
            f.write(M.STUB)
        with open(os.path.join(tmp, "stub", "lemma.json"), "w") as f:
            json.dump(M.LEMMA, f)
        sys.path[:0] = [os.path.join(REF, "misc", "grounding"), os.path.join(tmp, "stub")]
        sys.dont_write_bytecode = True
        anns, split_ids, results = random_set(np.random.default_rng(20241117))
        _, _, codes = record(arr, meta, words, "rnd", tmp, anns, split_ids, results)
        assert min(meta["sets"]["rnd"]["code_counts"]) >= 5, meta["sets"]["rnd"]["code_counts"]
        anns, split_ids, results, edges = edge_set()
        _, ref, codes = record(arr, meta, words, "edge", tmp, anns, split_ids, results)
        by_img = {i: [c for _, c in ev] for i, ev in codes}
        for name, e in edges.items():
            if isinstance(e, dict) and "event" in e:
                assert by_img[e["image"]][e["event"]] == e["code"], name
            if isinstance(e, dict) and "codes" in e:
                assert by_img[e["image"]] == e["codes"], (name, by_img[e["image"]])
        assert by_img[8003] == [] and 8004 not in by_img
        meta["edges"] = edges
        # the evaluator's own exception: image 8002 (which has objects) with four lists
        bad = dict(results)
        bad["8002"] = results["8002"][:4]
        try:
            run_reference(tmp, anns, split_ids, bad)
            raise AssertionError("the evaluator accepted four lists")
        except Exception as e:                                              # noqa: BLE001  (the reference raises a bare Exception)
            assert type(e) is Exception, type(e)
            meta["bad5"] = {"annotations": "edge", "message": str(e), "image": 8002}
        store_submission(arr, "bad5", bad)
        meta["has_model_set"] = model_set(arr, meta, words, tmp)
    meta["words"] = words.list
    with zipfile.ZipFile(os.path.join(HERE, "grounding_gt_case.npz"), "w", zipfile.ZIP_DEFLATED) as z:   # np.savez stamps the time of day
        for k in sorted(arr):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    with open(os.path.join(HERE, "grounding_gt_meta.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote grounding_gt_case.npz (%d arrays, %d bytes) and grounding_gt_meta.json (%d bytes)" % (
        len(arr), os.path.getsize(os.path.join(HERE, "grounding_gt_case.npz")), os.path.getsize(os.path.join(HERE, "grounding_gt_meta.json"))))
    for tag, s in meta["sets"].items():
        print(tag, "classes", s["n_classes"], "codes MISS/HIT/UNGROUNDED/NOROW", s["code_counts"], arr[tag + "_accu"])


if __name__ == "__main__":
    main()
