#!/usr/bin/env python
"""Write the grounding-score fixture by RUNNING THE REFERENCE's own evaluator where the reference lies (never copied):
grounding_case.npz + grounding_meta.json.  Data only: fabricated annotations, submissions and boxes as arrays, the expected event codes
and the numbers `FlickrGrdEval.grd_eval` returned in modes 'all' and 'loc'.

    python tests/golden/make_golden_grounding.py

`misc/grounding` goes first on sys.path (its `tools` package must win over the repository's tools/), and a stand-in `stanfordcorenlp`
module is written to a temporary directory: a dictionary lemmatizer (a token it does not hold is its own lemma) whose `annotate` returns
the JSON shape the evaluator reads.  The evaluator itself runs unmodified on temporary reference / split / submission JSON files.  Its
`prec` and `recall` dictionaries (per class the list of 0 / 1 it averaged) are captured from `grd_eval`'s frame when it returns
(sys.setprofile).

The expected event codes are derived here -- dictionary look-ups, and the reference's own `bbox_overlaps_batch` on `torch.Tensor` boxes for
every comparison -- and then CHECKED against the captured dictionaries of both runs: replaying the codes in the evaluator's order must
rebuild every per-class list of both modes, or this script fails.

Sets: `rnd` (random, ~40 images x up to 5 captions), `edge` (the planted cases; see `edges` in the meta), `nan` (two images, precision and
recall both 0: F1 is NaN) and `grd_<model>_<consensus>`: the material the reference's own get_grounding_material wrote for the `grd`
golden cases (tests/golden/grd_out.npz, read, not rewritten) against fabricated annotations for those images."""
import contextlib
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

MISS, HIT, SKIP, HALLUCINATED, ABSENT = 0, 1, 2, 3, 4
STUB = '''import json, os
class StanfordCoreNLP:
    def __init__(self, *a, **k):
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "lemma.json")) as f:
            self.lemma = json.load(f)
    def annotate(self, text, properties=None):
        return json.dumps({"sentences": [{"tokens": [{"lemma": self.lemma.get(text, text)}]}]})
    def close(self):
        pass
'''

# the synthetic word world of the rnd / edge / nan sets
DET = {k: f"c{k}" for k in range(1, 13)}
DET[3], DET[7] = "c3s", "c7s"                                   # class words that are not their own lemma
EXTRA = ["x1", "x2"]                                            # process_clss words outside the detection list
LEMMA = {"c3s": "c3", "c7s": "c7", "t5s": "t5", "c9ing": "c9"}
CLASSES = [DET[k] for k in sorted(DET)] + EXTRA
FILL = [f"t{i}" for i in range(1, 31)] + ["t5s"]
EXCUSE = ["c3", "c7", "c9ing", "c4", "c11"]                     # un-annotated tokens whose lemma is a class word's lemma


def overlap(pred, gt):
    """The evaluator's own comparison: torch.Tensor boxes through the reference's bbox_overlaps_batch."""
    import torch
    from tools.bbox_transform import bbox_overlaps_batch
    return float(torch.max(bbox_overlaps_batch(torch.Tensor(pred).unsqueeze(0), torch.Tensor(gt).unsqueeze(0).unsqueeze(0))))


def overlap64(p, g):
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    iw = max(min(p[2], g[2]) - max(p[0], g[0]) + 1, 0.0)
    ih = max(min(p[3], g[3]) - max(p[1], g[1]) + 1, 0.0)
    pa, ga = (p[2] - p[0] + 1) * (p[3] - p[1] + 1), (g[2] - g[0] + 1) * (g[3] - g[1] + 1)
    return iw * ih / (pa + ga - iw * ih)


def expected_codes(anns, split, results, lemma, thresh=0.5):
    """Per split image WITH a submission entry, in reference order: (image id, [(class word, code)] precision, [(class word, code)] recall)."""
    lem = lambda t: lemma.get(t, t)
    out = []
    for a in anns:
        img = str(a["image_id"])
        if img not in split or img not in results:
            continue
        sub = results[img][0]
        pe, re_ = [], []
        for c in a["captions"]:
            by_cls = {}
            for q, w in enumerate(c["process_clss"]):
                by_cls.setdefault(w, []).append(q)
            ex = {lem(t) for q, t in enumerate(c["tokens"]) if q not in c["process_idx"] and t != ""}
            for k, w in enumerate(sub["clss"]):
                if w in by_cls:
                    q = min(by_cls[w], key=lambda q: c["process_idx"][q])
                    pe.append((w, HIT if overlap(sub["bbox"][k], c["process_bnd_box"][q]) > thresh else MISS))
                elif lem(w) in ex:
                    pe.append((w, SKIP))
                else:
                    pe.append((w, HALLUCINATED))
            for q, w in enumerate(c["process_clss"]):
                if w in sub["clss"]:
                    k = sub["clss"].index(w)
                    re_.append((w, HIT if overlap(sub["bbox"][k], c["process_bnd_box"][q]) > thresh else MISS))
                else:
                    re_.append((w, ABSENT))
        out.append((a["image_id"], pe, re_))
    return out


def replay(anns, split, results, codes, mode):
    """The per-class lists the evaluator must have built, from the event codes, in its own order."""
    by_img = {str(i): (pe, re_) for i, pe, re_ in codes}
    prec, recall = {}, {}
    for a in anns:
        img = str(a["image_id"])
        if img in split and img in by_img:
            for w, code in by_img[img][0]:
                if code in (HIT, MISS) or (code == HALLUCINATED and mode == "all"):
                    prec.setdefault(w, []).append(1 if code == HIT else 0)
    for a in anns:
        img = str(a["image_id"])
        if img not in split:
            continue
        if img not in by_img:
            for c in a["captions"]:
                for w in c["process_clss"]:
                    recall.setdefault(w, []).append(0)
            continue
        for w, code in by_img[img][1]:
            if code in (HIT, MISS) or (code == ABSENT and mode == "all"):
                recall.setdefault(w, []).append(1 if code == HIT else 0)
    return prec, recall


def run_reference(tmp, anns, split_ids, results, lemma):
    """-> {mode: {"numbers": (prec, recall, f1), "prec": {...}, "recall": {...}, "vocab": [...]}} from the evaluator itself."""
    from eval_grd_flickr30k_entities import FlickrGrdEval
    with open(os.path.join(tmp, "stub", "lemma.json"), "w") as f:
        json.dump(lemma, f)
    paths = [os.path.join(tmp, n) for n in ("reference.json", "split.json", "submission.json")]
    for p, obj in zip(paths, ({"annotations": anns}, {"val": [str(i) for i in split_ids]}, {"results": results})):
        with open(p, "w") as f:
            json.dump(obj, f)
    out = {}
    for mode in ("all", "loc"):
        ev = FlickrGrdEval(reference_file=paths[0], submission_file=paths[2], split_file=paths[1], val_split=["val"], iou_thresh=0.5)
        got = {}

        def prof(frame, event, arg):
            if event == "return" and frame.f_code.co_name == "grd_eval":
                got.update(prec={k: list(v) for k, v in frame.f_locals["prec"].items()},
                           recall={k: list(v) for k, v in frame.f_locals["recall"].items()}, vocab=sorted(frame.f_locals["vocab_in_split"]))
        sys.setprofile(prof)
        try:
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()), np.errstate(all="ignore"):
                numbers = ev.grd_eval(mode=mode)
        finally:
            sys.setprofile(None)
        assert all(isinstance(x, np.float64) for x in numbers), numbers
        got["numbers"] = [float(x) for x in numbers]
        out[mode] = got
    return out


class Words:
    def __init__(self):
        self.list, self.id = [], {}

    def __call__(self, w):
        if w not in self.id:
            self.id[w] = len(self.list)
            self.list.append(w)
        return self.id[w]


def record(arr, meta, words, tag, tmp, anns, split_ids, results, lemma, store_sub=True, ann_tag=None):
    """Run the evaluator on a set, check the derived codes against it and store everything under `tag`."""
    split = {str(i) for i in split_ids}
    ref = run_reference(tmp, anns, split_ids, results, lemma)
    codes = expected_codes(anns, split, results, lemma)
    for mode in ("all", "loc"):
        prec, recall = replay(anns, split, results, codes, mode)
        assert prec == ref[mode]["prec"] and list(prec) == list(ref[mode]["prec"]), (tag, mode, "precision")
        assert recall == ref[mode]["recall"] and list(recall) == list(ref[mode]["recall"]), (tag, mode, "recall")
    assert ref["all"]["vocab"] == ref["loc"]["vocab"]
    i64 = lambda x: np.asarray(x, np.int64)
    if ann_tag is None:
        ann_tag = tag
        caps = [c for a in anns for c in a["captions"]]
        arr[tag + "_img_ids"], arr[tag + "_split"] = i64([a["image_id"] for a in anns]), i64(list(split_ids))
        arr[tag + "_cap_off"] = i64(np.concatenate([[0], np.cumsum([len(a["captions"]) for a in anns])]))
        arr[tag + "_tok_off"] = i64(np.concatenate([[0], np.cumsum([len(c["tokens"]) for c in caps])]))
        arr[tag + "_tok"] = np.asarray([words(t) for c in caps for t in c["tokens"]], np.int32)
        arr[tag + "_obj_off"] = i64(np.concatenate([[0], np.cumsum([len(c["process_clss"]) for c in caps])]))
        arr[tag + "_obj_cls"] = np.asarray([words(w) for c in caps for w in c["process_clss"]], np.int32)
        arr[tag + "_obj_idx"] = np.asarray([q for c in caps for q in c["process_idx"]], np.int32)
        arr[tag + "_obj_box"] = np.asarray([b for c in caps for b in c["process_bnd_box"]], np.float64).reshape(-1, 4)
        # the cook's expectations for the split's captions: the excluded lemmas (as words, ascending strings)
        scaps = [c for a in anns if str(a["image_id"]) in split for c in a["captions"]]
        ex = [sorted({lemma.get(t, t) for q, t in enumerate(c["tokens"]) if q not in c["process_idx"] and t != ""}) for c in scaps]
        arr[tag + "_ex_off"] = i64(np.concatenate([[0], np.cumsum([len(e) for e in ex])]))
        arr[tag + "_ex_lemma"] = np.asarray([words(l) for e in ex for l in e], np.int32)
    if store_sub:
        subs = [(k, v[0]) for k, v in results.items()]
        arr[tag + "_sub_ids"] = i64([int(k) for k, _ in subs])
        arr[tag + "_sub_off"] = i64(np.concatenate([[0], np.cumsum([len(s["clss"]) for _, s in subs])]))
        arr[tag + "_sub_cls"] = np.asarray([words(w) for _, s in subs for w in s["clss"]], np.int32)
        arr[tag + "_sub_idx"] = np.asarray([q for _, s in subs for q in s["idx_in_sent"]], np.int32)
        arr[tag + "_sub_box"] = np.asarray([b for _, s in subs for b in s["bbox"]], np.float64).reshape(-1, 4)
    arr[tag + "_ent_ids"] = i64([i for i, _, _ in codes])
    arr[tag + "_prec_off"] = i64(np.concatenate([[0], np.cumsum([len(pe) for _, pe, _ in codes])]))
    arr[tag + "_prec_cls"] = np.asarray([words(w) for _, pe, _ in codes for w, _ in pe], np.int32)
    arr[tag + "_prec_code"] = np.asarray([c for _, pe, _ in codes for _, c in pe], np.uint8)
    arr[tag + "_rec_off"] = i64(np.concatenate([[0], np.cumsum([len(r) for _, _, r in codes])]))
    arr[tag + "_rec_cls"] = np.asarray([words(w) for _, _, r in codes for w, _ in r], np.int32)
    arr[tag + "_rec_code"] = np.asarray([c for _, _, r in codes for _, c in r], np.uint8)
    arr[tag + "_numbers"] = np.asarray(ref["all"]["numbers"] + ref["loc"]["numbers"], np.float64)
    count = lambda key: [int(sum(1 for _, pe, re_ in codes for _, c in (pe if key == "p" else re_) if c == v)) for v in range(5)]
    meta["sets"][tag] = {"annotations": ann_tag, "num_vocab": len(ref["all"]["vocab"]), "vocab": ref["all"]["vocab"],
                         "precision_code_counts": count("p"), "recall_code_counts": count("r"),
                         "per_class": {m: {"prec": ref[m]["prec"], "recall": ref[m]["recall"]} for m in ("all", "loc")}}
    return ref, codes


def f32(x):
    return float(np.float32(x))


def find_rounding_pairs(rng):
    """Box pairs (pred, gt) of fp32 values whose fp32 overlap (the reference's function) and an fp64 evaluation of the same expression fall
    on opposite sides of 0.5: one where only fp32 says hit, one where only fp64 does."""
    up = down = None
    for _ in range(200000):
        x1, y1 = f32(rng.random() * 200), f32(rng.random() * 200)
        w, h = f32(20 + rng.random() * 300), f32(20 + rng.random() * 300)
        gt = [x1, y1, f32(x1 + w), f32(y1 + h)]
        hh = (gt[3] - gt[1] + 1) / 2                                        # half the height: an overlap next to 0.5
        y2 = np.float32(gt[1] + hh - 1)
        for _ in range(int(rng.integers(0, 4))):
            y2 = np.nextafter(y2, np.float32(np.inf if rng.random() < 0.5 else -np.inf))
        pred = [gt[0], gt[1], gt[2], float(y2)]
        a, b = overlap(pred, gt) > 0.5, overlap64(pred, gt) > 0.5
        if a and not b and up is None:
            up = (pred, gt)
        if b and not a and down is None:
            down = (pred, gt)
        if up and down:
            return up, down
    raise AssertionError("no rounding pair found")


def cap(tokens, objs):
    """objs: [(class word, word index, box)] in annotation order."""
    return {"tokens": list(tokens), "process_clss": [o[0] for o in objs], "process_idx": [int(o[1]) for o in objs],
            "process_bnd_box": [[float(x) for x in o[2]] for o in objs]}


def sub(entries):
    """entries: [(class word, word index, box)]."""
    return [{"clss": [e[0] for e in entries], "idx_in_sent": [int(e[1]) for e in entries], "bbox": [[float(x) for x in e[2]] for e in entries]}]


def random_set(rng):
    anns, results = [], {}
    for i in range(40):
        img = 7000 + i
        caps = []
        for _ in range(int(rng.integers(1, 6))):
            n_tok = int(rng.integers(4, 15))
            toks = [FILL[int(rng.integers(len(FILL)))] if rng.random() > 0.25 else (EXCUSE[int(rng.integers(len(EXCUSE)))] if rng.random() < 0.8 else "")
                    for _ in range(n_tok)]
            pos = rng.permutation(n_tok)[:int(rng.integers(0, 5))]
            objs = []
            for q in pos:
                x1, y1 = rng.random(2) * 200
                w, h = 5 + rng.random(2) * 150
                box = [x1, y1, x1 + w, y1 + h] if rng.random() < 0.7 else [round(x1), round(y1), round(x1 + w), round(y1 + h)]
                objs.append((CLASSES[int(rng.integers(len(CLASSES)))], int(q), box))
            caps.append(cap(toks, objs))
        anns.append({"image_id": img, "captions": caps})
        if rng.random() < 0.12:
            continue                                                        # not in the submission
        gts = [(w, b) for c in caps for w, b in zip(c["process_clss"], c["process_bnd_box"])]
        ents = []
        for k in range(int(rng.integers(0, 9))):
            if gts and rng.random() < 0.65:
                w, b = gts[int(rng.integers(len(gts)))]
                u = rng.random()
                if u < 0.45:
                    box = list(b)
                elif u < 0.75:
                    d = (rng.random(4) - 0.5) * 40
                    box = [b[0] + d[0], b[1] + d[1], b[2] + d[2], b[3] + d[3]]
                else:
                    box = [b[0], b[1], b[0] + (b[2] - b[0]) * 0.4, b[3]]
            else:
                w = CLASSES[int(rng.integers(len(CLASSES)))]
                x1, y1 = rng.random(2) * 200
                box = [x1, y1, x1 + 5 + rng.random() * 150, y1 + 5 + rng.random() * 150]
            ents.append((w, 2 * k, box))
        results[str(img)] = sub(ents)
    return anns, [a["image_id"] for a in anns], results


def edge_set(rng):
    up, down = find_rounding_pairs(rng)
    edges = {}
    big, shifted = [0, 0, 9, 9], [20, 20, 29, 29]
    k = 0
    y = np.float32(4)
    while True:                                                             # the nearest hit above the exact 0.5
        y = np.nextafter(y, np.float32(np.inf)); k += 1
        if overlap([0, 0, 9, float(y)], big) > 0.5:
            break
    assert overlap([0, 0, 9, 4], big) == 0.5
    plain = [10.5, 20.25, 110.75, 220.5]
    # image 9000: one caption, every box case its own class
    boxes = [("c1", [0, 0, 9, 4], big, MISS, "iou_exactly_half"), ("c2", [0, 0, 9, float(y)], big, HIT, "nearest_hit"),
             ("c4", shifted, big, MISS, "disjoint"), ("c5", [9.25, 0, 18, 9], big, MISS, "fraction_of_a_pixel"),
             ("c6", up[0], up[1], HIT, "fp32_hit_fp64_miss"), ("c8", down[0], down[1], MISS, "fp32_miss_fp64_hit"),
             ("c10", big, [5, 5, 5, 5], MISS, "zero_area_gt"), ("c11", [5, 5, 5, 5], big, MISS, "zero_area_pred"),
             ("c12", [5, 5, 5, 5], [5, 5, 5, 5], MISS, "zero_area_both"), ("x1", plain, plain, HIT, "identical")]
    a0 = {"image_id": 9000, "captions": [cap([w for w, *_ in boxes] + ["t1"], [(w, q, gt) for q, (w, _, gt, _, _) in enumerate(boxes)])]}
    r0 = sub([(w, q, pr) for q, (w, pr, _, _, _) in enumerate(boxes)])
    for q, (w, pr, gt, code, name) in enumerate(boxes):
        assert (overlap(pr, gt) > 0.5) == (code == HIT), name
        edges[name] = {"image": 9000, "event": q, "code": code}
    edges["nearest_hit"]["ulps_above"] = k
    assert overlap(big, [5, 5, 5, 5]) == 0.0 and overlap([5, 5, 5, 5], big) == -1.0 and overlap([5, 5, 5, 5], [5, 5, 5, 5]) == -1.0
    assert overlap64(up[0], up[1]) <= 0.5 < overlap(up[0], up[1]) and overlap(down[0], down[1]) <= 0.5 < overlap64(down[0], down[1])
    # image 9001: a class predicted twice, a class annotated twice (the later word listed first)
    b2, b5 = [0, 0, 50, 50], [100, 100, 160, 170]
    a1 = {"image_id": 9001, "captions": [cap(["t1", "t2", "c1", "t3", "t4", "c1", "t6"], [("c1", 5, b5), ("c1", 2, b2)])]}
    r1 = sub([("c1", 0, b2), ("c1", 3, b5)])
    edges["predicted_twice_annotated_twice"] = {"image": 9001, "precision": [HIT, MISS], "recall": [MISS, HIT]}
    # image 9002: lemma exclusion and hallucination
    a2 = {"image_id": 9002, "captions": [cap(["t1", "c3", "t2", "c9ing", "", "c7"], [("c2", 5, plain)])]}
    r2 = sub([("c3s", 0, plain), ("c9", 1, plain), ("c4", 2, plain), ("c2", 3, plain), ("c7s", 4, plain)])
    edges["lemma"] = {"image": 9002, "precision": [SKIP, SKIP, HALLUCINATED, HIT, HALLUCINATED],
                      "note": "c3s excused by the token c3, c9 by c9ing; c4 by nothing; c7s NOT by the token c7, which is annotated"}
    # image 9003: a caption without objects; 9004: five captions; 9005: an empty predicted list; 9006: a 64-word sentence, every word grounded
    a3 = {"image_id": 9003, "captions": [cap(["t1", "t2", "c4"], [])]}
    r3 = sub([("c4", 0, plain), ("c5", 1, plain)])
    edges["caption_without_objects"] = {"image": 9003, "precision": [SKIP, HALLUCINATED], "recall": []}
    a4 = {"image_id": 9004, "captions": [cap(["t1", "c1", "t2"], [("c1", 1, b2)]), cap(["c2", "t3"], [("c2", 0, b5)]), cap(["t4"], []),
                                         cap(["c1", "c2", "t5s"], [("c1", 0, b5), ("c2", 1, b2)]), cap(["", "x1"], [("x1", 1, plain)])]}
    r4 = sub([("c1", 0, b2), ("c2", 1, b2)])
    edges["five_captions"], edges["one_caption"] = 9004, 9000
    a5 = {"image_id": 9005, "captions": [cap(["c1", "t1"], [("c1", 0, b2)])]}
    r5 = sub([])
    edges["empty_predicted_list"] = 9005
    cyc = [CLASSES[q % (len(CLASSES) - 1)] for q in range(64)]           # every class but x2
    a6 = {"image_id": 9006, "captions": [cap(["t1"] * 10, [("c1", 0, b2), ("x1", 3, b5), ("c12", 7, plain)]), cap(["c3"], [])]}
    r6 = sub([(w, q, b2 if q % 3 else b5) for q, w in enumerate(cyc)])
    edges["sixty_four_words"] = 9006
    # image 9100: in the split, absent from the submission, its only class occurs nowhere else
    a7 = {"image_id": 9100, "captions": [cap(["x2", "t1", "x2"], [("x2", 0, b2), ("x2", 2, b5)])]}
    edges["missing_image"] = {"image": 9100, "class": "x2"}
    # image 9999: annotated but outside the split; image 9998: submitted but not annotated
    a8 = {"image_id": 9999, "captions": [cap(["c1"], [("c1", 0, b2)])]}
    edges["outside_the_split"], edges["submitted_but_not_annotated"] = 9999, 9998
    anns = [a0, a1, a2, a3, a7, a4, a5, a6, a8]
    results = {"9000": r0, "9001": r1, "9002": r2, "9003": r3, "9004": r4, "9005": r5, "9006": r6, "9998": sub([("c1", 0, b2)]),
               "9999": sub([("c1", 0, b2)])}
    split_ids = [9000, 9001, 9002, 9003, 9100, 9004, 9005, 9006]
    return anns, split_ids, results, edges


def nan_set():
    b2, b5 = [0, 0, 50, 50], [100, 100, 160, 170]
    anns = [{"image_id": 9200, "captions": [cap(["c1", "t1"], [("c1", 0, b2)])]}, {"image_id": 9201, "captions": [cap(["t1", "c2"], [("c2", 1, b5)])]}]
    return anns, [9200, 9201], {"9200": sub([("c1", 0, b5)]), "9201": sub([("c2", 0, b2)])}


def grd_sets(arr, meta, words, tmp):
    """The `grd` golden material (grd_out.npz) against fabricated annotations of its images, one evaluator run per model and pick rule."""
    with open(os.path.join(HERE, "meta.json")) as f:
        g = json.load(f)["grd"]
    with np.load(os.path.join(HERE, "grd_out.npz")) as z:
        out = {k: z[k] for k in z.files}
    V = len(g["vocab"])
    lemma = {f"cls{i}": f"l{i}" for i in range(1, V + 1)}
    lemma.update(g["wd_to_lemma"])
    for name, imgs in g["cases"].items():
        mats = {c: {i["id"]: {"clss": [str(x) for x in out[f"{name}_{i['id']}_{c}_clss"]], "idx_in_sent": out[f"{name}_{i['id']}_{c}_idx_in_sent"].tolist(),
                              "bbox": out[f"{name}_{i['id']}_{c}_bbox"].tolist()} for i in imgs} for c in (0, 1)}
        anns = []
        for n_img, i in enumerate(imgs):
            first = {}
            for c in (0, 1):
                m = mats[c][i["id"]]
                for w, b in zip(m["clss"], m["bbox"]):              # the class's first well-formed box (the detector boxes are random corners)
                    if w not in first or (not (first[w][2] > first[w][0] and first[w][3] > first[w][1]) and b[2] > b[0] and b[3] > b[1]):
                        first[w] = b
            objs, toks = [], []
            for q, (w, b) in enumerate(first.items()):
                box = b if q % 3 != 2 else [b[0] + 40, b[1] + 40, b[2] + 90, b[3] + 90]
                objs.append((w, q, box))
                toks.append("w1")
            other = f"cls{2 + n_img}"
            excuse = [w.replace("cls", "w") for q, w in enumerate(first) if q % 2 == 0]
            anns.append({"image_id": i["id"], "captions": [cap(toks + ["w2", ""], objs),
                                                           cap(["w3"] + excuse, [(other, 0, [1, 2, 30, 40])])]})
        anns.append({"image_id": 5999, "captions": [cap(["w1", "w4"], [("cls1", 0, [0, 0, 10, 10])])]})
        split_ids = [a["image_id"] for a in anns]
        for c in (0, 1):
            results = {str(k): [v] for k, v in mats[c].items()}
            record(arr, meta, words, f"grd_{name}_{c}", tmp, anns, split_ids, results, lemma, store_sub=False, ann_tag=None if c == 0 else f"grd_{name}_0")
    meta["grd_lemma_rule"] = "cls<i> -> l<i>; the words of the grd case's wd_to_lemma; everything else is its own lemma"


def main():
    assert os.path.isdir(REF), "golden vectors can only be regenerated where the reference exists"
    arr, words = {}, Words()
    meta = {"det_id_to_det_wd": {str(k): v for k, v in DET.items()}, "extra_classes": EXTRA, "lemma": LEMMA, "classes": CLASSES,
            "codes": {"MISS": MISS, "HIT": HIT, "SKIP": SKIP, "HALLUCINATED": HALLUCINATED, "ABSENT": ABSENT}, "iou_thresh": 0.5, "sets": {}}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "stub"))
        with open(os.path.join(tmp, "stub", "stanfordcorenlp.py"), "w") as f:
            f.write(STUB)
        with open(os.path.join(tmp, "stub", "lemma.json"), "w") as f:
            json.dump({}, f)
        sys.path[:0] = [os.path.join(REF, "misc", "grounding"), os.path.join(tmp, "stub")]
        sys.dont_write_bytecode = True
        rng = np.random.default_rng(20241101)
        anns, split_ids, results = random_set(rng)
        ref, codes = record(arr, meta, words, "rnd", tmp, anns, split_ids, results, LEMMA)
        s = meta["sets"]["rnd"]
        assert min(s["precision_code_counts"][:4]) >= 5 and min(s["recall_code_counts"][:2] + s["recall_code_counts"][4:]) >= 5, s
        assert len(split_ids) - len(codes) >= 2                             # images of the split without a submission entry
        anns, split_ids, results, edges = edge_set(np.random.default_rng(7))
        ref, codes = record(arr, meta, words, "edge", tmp, anns, split_ids, results, LEMMA)
        by_img = {i: (pe, re_) for i, pe, re_ in codes}
        for name, e in edges.items():
            if isinstance(e, dict) and "event" in e:
                assert by_img[e["image"]][0][e["event"]][1] == e["code"] == by_img[e["image"]][1][e["event"]][1], name
            if isinstance(e, dict) and "precision" in e:
                assert [c for _, c in by_img[e["image"]][0]] == e["precision"], (name, by_img[e["image"]][0])
            if isinstance(e, dict) and "recall" in e:
                assert [c for _, c in by_img[e["image"]][1]] == e["recall"], (name, by_img[e["image"]][1])
        assert "x2" not in meta["sets"]["edge"]["vocab"] and ref["loc"]["recall"]["x2"] == [0, 0] == ref["all"]["recall"]["x2"]
        assert "x2" not in ref["all"]["prec"] and len(by_img[9006][0]) == 2 * 64 and by_img[9005][1] == [("c1", ABSENT)]
        meta["edges"] = edges
        anns, split_ids, results = nan_set()
        ref, _ = record(arr, meta, words, "nan", tmp, anns, split_ids, results, LEMMA)
        assert ref["all"]["numbers"][:2] == [0.0, 0.0] and all(np.isnan(ref[m]["numbers"][2]) for m in ("all", "loc"))
        grd_sets(arr, meta, words, tmp)
    meta["words"] = words.list
    with zipfile.ZipFile(os.path.join(HERE, "grounding_case.npz"), "w", zipfile.ZIP_DEFLATED) as z:   # np.savez stamps the time of day
        for k in sorted(arr):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    with open(os.path.join(HERE, "grounding_meta.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote grounding_case.npz (%d arrays, %d bytes) and grounding_meta.json (%d bytes)" % (
        len(arr), os.path.getsize(os.path.join(HERE, "grounding_case.npz")), os.path.getsize(os.path.join(HERE, "grounding_meta.json"))))
    for tag, s in meta["sets"].items():
        print(tag, "num_vocab", s["num_vocab"], "precision", s["precision_code_counts"], "recall", s["recall_code_counts"], arr[tag + "_numbers"])


if __name__ == "__main__":
    main()
