"""Set-controllability scores (Noun IoU, BLEU, ROUGE-L, CIDEr) of a `--sct 1` decode on the device: the fourth table of the paper.

The reference finishes a controllability run with misc/controllability/controllability_score.py: per (generated caption, ground-truth
caption of its region set) pair `NounIoU.score` (misc/controllability/noun_iou.py:19-47) makes one `torch.from_numpy` +
`F.cosine_similarity` call per (noun, noun) cell of a Python double loop, hands the matrix to a pure-Python Hungarian solver (`munkres`)
and forms I / (m + n - I); the COCO scorer stack then runs over the same groups on strings.  Here one launch of
`subgc_control_noun_iou` (include/subgc_controllability_hip.h) does the first part for a whole batch of token rows -- a wave per pair
fills the similarity matrix in LDS and solves the assignment -- and the existing accuracy launches (subgc.accuracy, one candidate per
group, `oracle_num` = 1) do the second on the same stream; everything comes back in one host copy.  Corpus numbers are formed on the host
(`summarize`), so they accumulate across batches and ranks.

`NounVectors` is the one-time cook (numpy allowed) of the unpickled `flickr_noun_glove.pkl`, `ControlReferences` that of
`sct_gt_captions.npy`; `ControlScorer.score` and the `controllability=` argument of `eval_glue.caption_images` are the per-batch path and
issue only C-ABI launches; `score_predictions` is the drop-in for controllability_score.py on a finished `ctl_captions_*.npy` list.

Out of scope: METEOR and SPICE (Java programs), PTB tokenisation (captions are split at spaces, as `prep_seq` splits them), and making
`flickr_noun_glove.pkl`, `order_list.npy` or `sct_gt_captions.npy`: the caller loads them.
"""
from __future__ import annotations

import numpy as np

from . import _scoring, accuracy as _accuracy
from ._lib import SubgcError, call_controllability
from ._scoring import csr as _csr

MAX_WORDS = 64           # SUBGC_CTL_MAX_WORDS: vector words of a caption, on either side
COS_EPS = 1e-8           # the clamp of the cosine's denominator
NAMES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "Noun_IoU")


class NounVectors:
    """vectors: the unpickled {word: 1-d array} of the pre-computed file (GloVe vectors of the Flickr30k nouns); ix_to_word: the model's
    vocabulary.  Cooks `vec` fp32 [n_noun, d] (rows in the dictionary's order), `norm` fp64 [n_noun] (Euclidean norms of the fp32 rows,
    computed once), `tok_noun` int32 (model word id -> row, -1 = the word has no vector) and `word_row` (word -> row: a ground-truth word
    need not be in the model's vocabulary).  `device="auto"`: the current GPU; `device=None`: the host tables only."""

    def __init__(self, vectors, ix_to_word, device="auto"):
        if len(vectors) < 1:
            raise ValueError("controllability: no word vectors")
        self.words = list(vectors)
        rows = [np.asarray(vectors[w]) for w in self.words]
        d = rows[0].size
        for w, v in zip(self.words, rows):
            if v.ndim != 1 or v.size != d or d < 1:
                raise ValueError(f"controllability: the vector of {w!r} has shape {v.shape}; every vector is 1-d with the {d} entries of the first")
            if not np.isfinite(v.astype(np.float64)).all():
                raise ValueError(f"controllability: the vector of {w!r} has non-finite entries")
        self.vec = np.ascontiguousarray(np.stack(rows).astype(np.float32))
        if not np.isfinite(self.vec).all():
            raise ValueError("controllability: a vector overflows fp32")
        self.d, self.n_noun = int(d), len(rows)
        self.norm = np.sqrt(np.sum(self.vec.astype(np.float64) ** 2, axis=1))
        self.word_row = {w: i for i, w in enumerate(self.words)}
        V = max((int(k) for k in ix_to_word), default=0)
        self.tok_noun = np.full(V + 1, -1, np.int32)
        for k, w in ix_to_word.items():
            self.tok_noun[int(k)] = self.word_row.get(w, -1)
        self.device = None
        if device is not None:
            self.to(_scoring.resolve_device(device))

    def to(self, device):
        import torch
        dev = torch.device(device)
        self.d_vec, self.d_norm = torch.from_numpy(self.vec).to(dev), torch.from_numpy(self.norm).to(dev)
        self.device = dev
        return self


class ControlReferences:
    """gt_groups: the list of `sct_gt_captions.npy` -- per region set (in `order_list` order) the list of its ground-truth captions, each
    a string.  Cooks the offset tables of subgc_control_noun_iou (`gcap_off`, `gn_off`, `gn`: every caption split at ' ' exactly as
    `prep_seq` splits it, the words that have a vector kept in sentence order with repeats) and an `AccuracyReferences` whose "images" are
    the groups (captions split at white space; the CIDEr document frequency is over the groups, as the script's is).  `tok_noun` extends
    the vectors' table over the ids the accuracy cook gives to reference-only words, so a finished caption list can name them too."""

    def __init__(self, gt_groups, nouns, ix_to_word, device="auto"):
        if len(gt_groups) < 1:
            raise ValueError("controllability: no ground-truth groups")
        cap_n, word_n, gn = [], [], []
        for g, caps in enumerate(gt_groups):
            if isinstance(caps, str):
                raise ValueError(f"controllability: group {g} is a string; a group is a list of caption strings")
            if len(caps) < 1:
                raise ValueError(f"controllability: group {g} has no ground-truth caption; the score divides by the group's size")
            cap_n.append(len(caps))
            for s, cap in enumerate(caps):
                rows = [nouns.word_row[w] for w in cap.split(" ") if w in nouns.word_row]
                if len(rows) > MAX_WORDS:
                    raise ValueError(f"controllability: caption {s} of group {g} has {len(rows)} words with a vector; the limit is {MAX_WORDS}")
                word_n.append(len(rows))
                gn += rows
        self.nouns = nouns
        self.n_groups, self.n_caps, self.n_gn = len(cap_n), int(sum(cap_n)), len(gn)
        self.gcap_off, self.gn_off, self.gn = _csr(cap_n), _csr(word_n), np.array(gn, np.int32)
        self.accuracy = _accuracy.AccuracyReferences([[cap.split() for cap in caps] for caps in gt_groups], ix_to_word, device=None)
        self.tok_noun = np.full(self.accuracy.n_ids + 1, -1, np.int32)
        for w, k in self.accuracy.word_to_ix.items():
            self.tok_noun[k] = nouns.word_row.get(w, -1)
        self.device = None
        if device is not None:
            self.to(_scoring.resolve_device(device))

    def to(self, device):
        """Upload the tables (the vectors too, if they are not there yet); done once."""
        import torch
        dev = torch.device(device)
        if self.nouns.device != dev:
            self.nouns.to(dev)
        self.accuracy.to(dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, a.dtype)).astype(np.int32)).to(dev)
        self.d_tok_noun, self.d_gcap_off, self.d_gn_off, self.d_gn = up(self.tok_noun), up(self.gcap_off), up(self.gn_off), up(self.gn)
        self.device = dev
        return self


class ControlScorer:
    """controllability_score.py:40-52 and :54-69 for a batch of token rows, one generated caption per region set."""

    def __init__(self, refs):
        self.refs = refs
        self.acc = _accuracy.AccuracyScorer(refs.accuracy, oracle_num=1)

    def check_index(self, group_index):
        idx = [int(x) for x in group_index]
        for r, g in enumerate(idx):
            if not -1 <= g < self.refs.n_groups:
                raise SubgcError(f"controllability: row {r} names group {g}; the references hold {self.refs.n_groups} groups (-1 = no group)")
        return idx

    def plan(self, group_index):
        """The host side of a batch: the pairs of every row.  -> {"rows", "P", "idx", "pair_off"}."""
        r = self.refs
        idx = np.array(self.check_index(group_index), np.int64)
        live = idx >= 0
        ncap = np.where(live, r.gcap_off[np.where(live, idx, 0) + 1] - r.gcap_off[np.where(live, idx, 0)], 0) if len(idx) else np.zeros(0, np.int64)
        pair_off = _csr(ncap)
        return {"rows": len(idx), "P": int(pair_off[-1]), "idx": idx, "pair_off": pair_off}

    def arena_words(self, plan):
        """int32 words of a batch's results: the accuracy records first (they hold fp64), then iou, pair_iou, pair_mn and assign."""
        rows, P = plan["rows"], plan["P"]
        return self.acc.arena_words(rows, rows) + rows + P + 2 * P + (MAX_WORDS // 4) * P

    def views(self, arena, plan):
        """(accuracy arena, iou fp32 [rows], pair_iou fp32 [P], pair_mn int32 [P, 2], assign int8 [P, 64]) views of an arena (torch or numpy)."""
        f32, i8 = (ns := _scoring.dtypes(arena)).float32, ns.int8
        rows, P = plan["rows"], plan["P"]
        o = self.acc.arena_words(rows, rows)
        acc = arena[:o]
        iou = arena[o:o + rows].view(f32); o += rows
        pair = arena[o:o + P].view(f32); o += P
        mn = arena[o:o + 2 * P].reshape(P, 2); o += 2 * P
        ass = arena[o:o + (MAX_WORDS // 4) * P].view(i8).reshape(P, MAX_WORDS)
        return acc, iou, pair, mn, ass

    def enqueue_noun_iou(self, seq, table, remove_bad_endings, arena, plan):
        """subgc_control_noun_iou on the current stream.  seq: device token rows [rows, T] (int32 / int64); table: device int32, row_group
        [rows] followed by pair_off [rows + 1] (or a longer tensor that starts with them)."""
        import torch
        from . import ops
        r, nv = self.refs, self.refs.nouns
        if r.device is None:
            raise SubgcError("controllability: the references are not on a device (ControlReferences(..., device=...) or .to(device))")
        t64, T = _scoring.token_rows("controllability", seq)
        rows = seq.size(0)
        if rows != plan["rows"]:
            raise SubgcError(f"controllability: {rows} token rows, the plan holds {plan['rows']}")
        if arena.numel() < self.arena_words(plan):
            raise SubgcError("controllability: the result arena is too short")
        _, iou, pair, mn, ass = self.views(arena, plan)
        bad = r.accuracy.corpus.d_bad if remove_bad_endings else None
        P, has = ops._ptr, plan["P"] > 0
        call_controllability("subgc_control_noun_iou", P(seq), t64, int(T), P(bad, torch.uint8), 0 if bad is None else bad.numel(),
                             int(rows), P(r.d_tok_noun, torch.int32), len(r.tok_noun), P(nv.d_vec, torch.float32), P(nv.d_norm, torch.float64), nv.n_noun,
                             nv.d, P(table[:rows], torch.int32), r.n_groups, P(table[rows:2 * rows + 1], torch.int32), plan["P"],
                             P(r.d_gcap_off, torch.int32), r.n_caps, P(r.d_gn_off, torch.int32), P(r.d_gn, torch.int32), r.n_gn,
                             P(iou) if rows else None, P(pair) if has else None, P(mn) if has else None, P(ass) if has else None, ops._stream())

    def unpack(self, host, plan):
        """The host copy of an arena -> per row a dict of plain numpy data: "group", "noun_iou" (np.float32: the group mean), "pair_iou"
        fp32 [k], "pair_mn" int32 [k, 2] (the m and n of every pair), "assign" int8 [k, 64] (per ground-truth word the predicted word
        matched to it, or -1) and "accuracy" (`AccuracyScorer.unpack`'s entry of the row against its group; None for a row without group)."""
        rows = plan["rows"]
        host = np.ascontiguousarray(host)
        acc, iou, pair, mn, ass = self.views(host, plan)
        a_entries = self.acc.unpack(acc, list(range(rows + 1))) if rows else []
        out = []
        for r in range(rows):
            a, b = int(plan["pair_off"][r]), int(plan["pair_off"][r + 1])
            g = int(plan["idx"][r])
            out.append({"group": g, "noun_iou": np.float32(iou[r]), "pair_iou": pair[a:b].copy(), "pair_mn": mn[a:b].copy(), "assign": ass[a:b].copy(),
                        "accuracy": a_entries[r] if g >= 0 else None})
        return out

    def score(self, seq, group_index, remove_bad_endings=0):
        """seq [rows, T]: device token rows, one generated caption each; group_index[r]: the row's group in the references (-1: none).
        -> the per-row list of `unpack`.  The Noun IoU launch and the accuracy launches on one stream, one host copy."""
        import torch
        from . import ops
        if not seq.is_cuda:
            raise SubgcError("subgc ops need device tensors (the HIP path has no CPU fallback)")
        if len(group_index) != seq.size(0):
            raise SubgcError(f"controllability: {seq.size(0)} token rows and {len(group_index)} group indices")
        plan = self.plan(group_index)
        rows = plan["rows"]
        if rows == 0:
            return []
        dev = seq.device
        seq = seq.contiguous()
        # row_group | pair_off | the accuracy launch's row boundaries (one row per "image") | its reference "image" of every row
        tab = ops.upload(plan["idx"].tolist() + plan["pair_off"].tolist() + list(range(rows + 1)) + np.maximum(plan["idx"], 0).tolist(), torch.int32, dev)
        arena = torch.empty(max(self.arena_words(plan), 2), device=dev, dtype=torch.int32)
        self.enqueue_noun_iou(seq, tab, remove_bad_endings, arena, plan)
        self.acc.enqueue(seq, tab[2 * rows + 1:3 * rows + 2], rows, tab[3 * rows + 2:4 * rows + 2], None, remove_bad_endings, self.views(arena, plan)[0])
        return self.unpack(arena.cpu().numpy(), plan)                        # the one copy


def summarize(entries):
    """Per-row entries (`ControlScorer.score`, or the `"controllability"` entries of `caption_images` flattened in `order_list` order) ->
    the script's corpus numbers: "Bleu_1" .. "Bleu_4", "ROUGE_L", "CIDEr" through `accuracy.summarize` (corpus BLEU of the summed
    material, the means of the per-row ROUGE-L / CIDEr) and "Noun_IoU": `np.mean` of the per-row values as an fp32 array in entry order
    (what the script's `np.mean(scores_iou)` is for a list of fp32 values).  "rows": how many entered; rows without a group are left out."""
    live = [e for e in entries if e["group"] >= 0]
    out = {"rows": len(live), "left_out": len(entries) - len(live)}
    if not live:
        return out
    a = _accuracy.summarize([e["accuracy"] for e in live])
    for k in NAMES[:6]:
        out[k] = a[k]
    out["Noun_IoU"] = np.mean(np.array([e["noun_iou"] for e in live], np.float32))
    return out


def order_captions(predictions, order_list):
    """controllability_score.py:20-33: the generated captions re-ordered as the ground-truth groups are -- image by image in `order_list`
    order, an image's captions in their own order.  -> (captions, image id of every caption)."""
    sen = {str(p["image_id"]): p["caption"] for p in predictions}
    caps, ids = [], []
    for img in order_list:
        if str(img) not in sen:
            raise ValueError(f"controllability: order_list names image {img!r}, which has no prediction")
        caps.extend(sen[str(img)])
        ids.extend([str(img)] * len(sen[str(img)]))
    return caps, ids


def score_predictions(predictions, order_list, refs, ix_to_word, remove_bad_endings=0, device="auto", verbose=True):
    """The drop-in for controllability_score.py on a `ctl_captions_*.npy`-style list ({'image_id', 'caption': [one string per region
    set]}).  refs: a ControlReferences over `sct_gt_captions.npy`, or that list itself together with `ix_to_word` and a NounVectors as
    `refs = (gt_groups, nouns)`.  Captions are split at white space (like `accuracy.encode_predictions`) and mapped through the references' id map (a word neither the model nor the
    references know is refused).  Prints the script's lines -- its 'Blue_1' spelling included; METEOR and SPICE are Java programs and
    are left out -- and returns (summarize(...), the per-row entries in `order_list` order)."""
    import torch
    if not isinstance(refs, ControlReferences):
        gt_groups, nouns = refs
        refs = ControlReferences(gt_groups, nouns, ix_to_word, device=None)
    caps, ids = order_captions(predictions, order_list)
    if len(caps) != refs.n_groups:
        raise ValueError(f"controllability: {len(caps)} generated captions, the references hold {refs.n_groups} groups")
    dev = _scoring.resolve_device(device)
    if refs.device is None:
        refs.to(dev)
    rows = []
    for c, img in zip(caps, ids):
        try:
            rows.append(refs.accuracy.encode(c))
        except SubgcError as e:
            raise SubgcError(f"{e} (a caption of image {img!r})") from None
    seq = _scoring.id_rows("controllability", rows, MAX_WORDS)
    entries = ControlScorer(refs).score(torch.from_numpy(seq).to(dev), list(range(len(rows))), remove_bad_endings=remove_bad_endings)
    s = summarize(entries)
    if verbose:
        print("totally {} images in the test set".format(len({str(p["image_id"]) for p in predictions})))
        print("Computing set contrallabity results.")
        for name, key in zip(("Blue_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"), NAMES[:6]):
            print(name, s[key])
        print("Noun IoU", s["Noun_IoU"])
    return s, entries
