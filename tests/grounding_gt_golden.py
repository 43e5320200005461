"""The GT-sentence grounding fixture (tests/golden/make_golden_grounding_gt.py: written by running the reference's own evaluator) and the
forced-decode fixture (make_golden_forced.py: the reference model driven along given tokens) as the objects the tests need."""
import json
import os

import numpy as np

import grounding_golden as G

GOLDEN = G.GOLDEN


def load():
    with open(os.path.join(GOLDEN, "grounding_gt_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "grounding_gt_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def load_forced():
    with open(os.path.join(GOLDEN, "forced_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "forced_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def annotations(meta, arr, tag):
    return G.annotations(meta, arr, "edge" if tag == "bad5" else tag)


def results(arr, tag):
    """The GT-mode submission's 'results' dict: per image its lists of {'idx_in_sent', 'bbox'}."""
    lo, eo = arr[tag + "_sub_list_off"], arr[tag + "_sub_ent_off"]
    out = {}
    for i, img in enumerate(arr[tag + "_sub_ids"].tolist()):
        out[str(img)] = [{"idx_in_sent": arr[tag + "_sub_idx"][eo[q]:eo[q + 1]].tolist(), "bbox": arr[tag + "_sub_box"][eo[q]:eo[q + 1]].tolist()}
                         for q in range(lo[i], lo[i + 1])]
    return out


def references(meta, arr, tag, device=None):
    from subgc.grounding import GroundingReferences
    anns, split = annotations(meta, arr, tag)
    return GroundingReferences(anns, split, meta["det_id_to_det_wd"], G.WD_TO_LEMMA, G.LEMMA_DET, G.VOCAB, meta["lemma"], device=device)


def expected_entries(meta, arr, tag, refs):
    """The fixture's event codes as `GtGroundingScorer.unpack`-style entries ("ref", "events"), in reference order."""
    W, off = meta["words"], arr[tag + "_code_off"]
    out = []
    for i, img in enumerate(arr[tag + "_ent_ids"].tolist()):
        s = slice(off[i], off[i + 1])
        c = np.array([refs.class_id[W[x]] for x in arr[tag + "_code_cls"][s]], np.int32)
        out.append({"ref": refs.index[str(img)], "events": np.stack([c, arr[tag + "_code"][s].astype(np.int32)], 1).reshape(-1, 2)})
    return out


def same_events(got, want):
    assert [e["ref"] for e in got] == [e["ref"] for e in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g["events"], w["events"], err_msg=f"events of reference image {w['ref']}")


def accu_close(got, want, n_classes):
    """grd_accu within 4 * C * 2^-53 ABSOLUTE of the reference's: the C ratios are each rounded once, their sum (terms <= 1) is taken in
    two orders, one division."""
    tol = 4 * max(n_classes, 1) * 2.0 ** -53
    assert tol < 1e-13 and abs(got - want) <= tol, (got, want, tol)


def restate_submission(refs, res):
    """The numpy restatement over a whole submission, in reference order -> entries; raises like `score_submission`."""
    from subgc import grounding_gt as GT
    out = []
    for j, img in enumerate(refs.image_ids):
        s0, s1 = int(refs.cap_off[j]), int(refs.cap_off[j + 1])
        pred = res.get(img)
        if pred is not None and refs.obj_off[s1] > refs.obj_off[s0] and len(pred) != 5:
            raise Exception("Each image must have five caption predictions!")
        lists = [] if pred is None else [(e["idx_in_sent"], e["bbox"]) for e in pred[:s1 - s0]]
        codes = GT.restatement(lists, list(range(s0, s1)), [-1] * (s1 - s0) if pred is None else list(range(s1 - s0)), refs.obj_off, refs.obj_idx,
                               refs.obj_box)
        ev = [np.stack([refs.obj_cls[refs.obj_off[s]:refs.obj_off[s + 1]], c.astype(np.int32)], 1) for s, c in zip(range(s0, s1), codes)]
        out.append({"ref": j, "events": np.concatenate(ev + [np.zeros((0, 2), np.int32)]).astype(np.int32)})
    return out
