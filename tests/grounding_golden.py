"""The grounding-score fixture (tests/golden/make_golden_grounding.py: written by running the reference's own evaluator) as the objects
the tests need: annotations and submissions rebuilt from the arrays, the cooked references, and the expected per-image entries."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# a small model vocabulary for the synthetic sets: ids 1 .. 12 name the detection classes 1 .. 12 through a lemma, 13 .. 15 are bad
# endings ("with" also names class 12), 16 / 17 have a lemma that is no detection class, 18 is unknown to the lemmatiser
VOCAB = {str(i): f"w{i}" for i in range(1, 13)}
VOCAB.update({"13": "a", "14": "the", "15": "with", "16": "n16", "17": "n17", "18": "n18"})
WD_TO_LEMMA = {f"w{i}": f"l{i}" for i in range(1, 13)}
WD_TO_LEMMA.update({"a": "a", "the": "the", "with": "l12", "n16": "l16", "n17": "l17"})
LEMMA_DET = {f"l{i}": i for i in range(1, 13)}


def load():
    with open(os.path.join(GOLDEN, "grounding_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(GOLDEN, "grounding_case.npz")) as z:
        arr = {k: z[k] for k in z.files}
    return meta, arr


def grd_meta():
    with open(os.path.join(GOLDEN, "meta.json")) as f:
        return json.load(f)["grd"]


def annotations(meta, arr, tag):
    t, W = meta["sets"][tag]["annotations"], meta["words"]
    cap, tok, obj = arr[t + "_cap_off"], arr[t + "_tok_off"], arr[t + "_obj_off"]
    out = []
    for j, img in enumerate(arr[t + "_img_ids"].tolist()):
        caps = []
        for s in range(cap[j], cap[j + 1]):
            o = slice(obj[s], obj[s + 1])
            caps.append({"tokens": [W[x] for x in arr[t + "_tok"][tok[s]:tok[s + 1]]], "process_clss": [W[x] for x in arr[t + "_obj_cls"][o]],
                         "process_idx": arr[t + "_obj_idx"][o].tolist(), "process_bnd_box": arr[t + "_obj_box"][o].tolist()})
        out.append({"image_id": img, "captions": caps})
    return out, arr[t + "_split"].tolist()


def results(meta, arr, tag):
    """The submission's 'results' dict of a synthetic set (the grd sets' material is in grd_out.npz)."""
    W, off = meta["words"], arr[tag + "_sub_off"]
    out = {}
    for i, img in enumerate(arr[tag + "_sub_ids"].tolist()):
        o = slice(off[i], off[i + 1])
        out[str(img)] = [{"clss": [W[x] for x in arr[tag + "_sub_cls"][o]], "idx_in_sent": arr[tag + "_sub_idx"][o].tolist(),
                          "bbox": arr[tag + "_sub_box"][o].tolist()}]
    return out


def grd_results(tag):
    """grd_<model>_<consensus> -> the 'results' dict the reference's get_grounding_material wrote (grd_out.npz)."""
    _, name, c = tag.split("_")
    with np.load(os.path.join(GOLDEN, "grd_out.npz")) as z:
        return {str(i["id"]): [{"clss": [str(x) for x in z[f"{name}_{i['id']}_{c}_clss"]], "idx_in_sent": z[f"{name}_{i['id']}_{c}_idx_in_sent"].tolist(),
                                "bbox": z[f"{name}_{i['id']}_{c}_bbox"].tolist()}] for i in grd_meta()["cases"][name]}


def grd_lemma():
    g = grd_meta()
    lemma = {f"cls{i}": f"l{i}" for i in range(1, len(g["vocab"]) + 1)}
    lemma.update(g["wd_to_lemma"])
    return lemma


def references(meta, arr, tag, device=None):
    from subgc.grounding import GroundingReferences
    anns, split = annotations(meta, arr, tag)
    if tag.startswith("grd_"):
        g = grd_meta()
        return GroundingReferences(anns, split, g["det_id_to_det_wd"], g["wd_to_lemma"], g["lemma_det_id_dict"], g["vocab"], grd_lemma(), device=device)
    return GroundingReferences(anns, split, meta["det_id_to_det_wd"], WD_TO_LEMMA, LEMMA_DET, VOCAB, meta["lemma"], device=device)


def expected_entries(meta, arr, tag, refs):
    """The fixture's event codes as `GroundingScorer.unpack`-style entries (precision / recall only), in reference order."""
    W = meta["words"]
    po, ro = arr[tag + "_prec_off"], arr[tag + "_rec_off"]
    out = []
    for i, img in enumerate(arr[tag + "_ent_ids"].tolist()):
        p, r = slice(po[i], po[i + 1]), slice(ro[i], ro[i + 1])
        pc = np.array([refs.class_id[W[x]] for x in arr[tag + "_prec_cls"][p]], np.int32)
        rc = np.array([refs.class_id[W[x]] for x in arr[tag + "_rec_cls"][r]], np.int32)
        out.append({"ref": refs.index[str(img)], "precision": np.stack([pc, arr[tag + "_prec_code"][p].astype(np.int32)], 1).reshape(-1, 2),
                    "recall": np.stack([rc, arr[tag + "_rec_code"][r].astype(np.int32)], 1).reshape(-1, 2)})
    return out


def same_events(got, want):
    assert [e["ref"] for e in got] == [e["ref"] for e in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g["precision"], w["precision"], err_msg=f"precision events of reference image {w['ref']}")
        np.testing.assert_array_equal(g["recall"], w["recall"], err_msg=f"recall events of reference image {w['ref']}")


def numbers(summary):
    from subgc.grounding import NAMES
    return [summary[n] for n in NAMES]


def close(got, want, n_classes):
    """The six numbers within 4 * n_classes * 2^-53 relative (two orders of summing n ratios in [0, 1] plus the few operations of F1);
    a NaN must be met by a NaN, a 0.0 by a 0.0.  n_classes: the classes that can add a non-zero ratio, num_vocab (a class outside it is
    hallucinated or belongs to a missing image: it adds an exact 0)."""
    tol = 4 * max(n_classes, 1) * 2.0 ** -53
    assert tol < 1e-14
    for g, w in zip(got, want):
        if math.isnan(w):
            assert math.isnan(g), (got, want)
        elif w == 0.0:
            assert g == 0.0, (got, want)
        else:
            assert abs(g - w) <= tol * abs(w), (got, want)
