"""Accuracy and oracle scores of a whole decode batch on the device (`test.py --only_sent_eval 1 --oracle_num N`: misc/eval_utils.py:176-189
-> misc/sentence_utils.py:56-125 `language_eval` and :28-53 `cal_bleu`; the scorers are misc/coco-caption/pycocoevalcap/bleu/bleu_scorer.py,
cider/cider_scorer.py and rouge/rouge.py).

The reference runs the COCO scorer stack once per caption position -- N corpus passes of Python dictionaries over strings -- then takes,
per image, the caption with the largest sentence BLEU of each order, re-sums the BLEU material of those picks and averages the largest
CIDEr and ROUGE-L.  Here the token rows of a decode batch are already on the device in caption order; after one cook launch
(`subgc_consensus_cook`, the tf-idf lists) two launches of include/subgc_metrics_hip.h take them to per-row integers and fp64 values
(`subgc_accuracy_rows`) and to per-image picks and maxima (`subgc_accuracy_oracle`).  Corpus numbers are formed on the host from the
per-image integers and fp64 values with the reference's own expressions (`summarize`), so they accumulate across batches and ranks.

`AccuracyReferences(ref_sentences, ix_to_word)` is the one-time setup (numpy / torch allowed): `ref_sentences[j]` = the reference captions
of evaluated image j, each a list of words (already tokenised).  Document frequencies are counted per image over exactly these images and
`ref_len = log(len(ref_sentences))`, as `CiderScorer.compute_doc_freq` does over the evaluated set -- score a split with the references
of the whole split, whatever the batching.  `AccuracyScorer.score` and the `accuracy=` argument of `eval_glue.caption_images` are the
per-batch path and issue only C-ABI launches.

Two splits, as in the reference: BLEU and CIDEr split at white space (an empty caption has no words), ROUGE-L at single spaces (an empty
caption is the one-word caption of the empty word, which equals only itself).

Out of scope: METEOR and SPICE (Java), PTB tokenisation, the COCO json plumbing and `all_scores_*.npy`.
"""
from __future__ import annotations

import math

import numpy as np

from . import _scoring
from ._lib import SubgcError, call_metrics
from ._scoring import MAX_IDS

MAX_T = 64               # words of a candidate row
MAX_REF_WORDS = 256      # words of a reference caption (SUBGC_ACC_MAX_REF_WORDS)
MAX_REFS = 32            # reference captions of an image (SUBGC_ACC_MAX_REFS)
ROW_INT, ROW_F64, IMG_INT, IMG_F64 = 10, 6, 56, 12      # the SUBGC_ACC_* record widths of subgc_metrics_hip.h
BETA2 = 1.2 ** 2         # rouge.py:46,73 `self.beta**2`
NAMES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "CIDEr", "ROUGE_L")


def bleu_table(words, woff, cap_off):
    """cook_refs' `maxcounts` (bleu_scorer.py:45-52) for every image: (boff int64 [n_img + 1], keys uint64, maxcount int32) -- image j's
    distinct n-gram keys in ascending order with the largest count over its captions."""
    from .consensus import ngram_keys
    n_img = len(cap_off) - 1
    keys, sent = ngram_keys(words, woff)
    if len(keys) == 0:
        return np.zeros(n_img + 1, np.int64), np.zeros(0, np.uint64), np.zeros(0, np.int32)
    img = np.repeat(np.arange(n_img), np.diff(cap_off))[sent]
    o = np.lexsort((sent, keys, img))
    keys, sent, img = keys[o], sent[o], img[o]
    new_run = np.ones(len(keys), bool)                                    # a run = one (image, key, caption): its length is the count
    new_run[1:] = (img[1:] != img[:-1]) | (keys[1:] != keys[:-1]) | (sent[1:] != sent[:-1])
    start = np.flatnonzero(new_run)
    count = np.diff(np.append(start, len(keys)))
    r_img, r_key = img[start], keys[start]
    new_key = np.ones(len(start), bool)
    new_key[1:] = (r_img[1:] != r_img[:-1]) | (r_key[1:] != r_key[:-1])
    first = np.flatnonzero(new_key)
    mx = np.maximum.reduceat(count, first)
    boff = np.concatenate([[0], np.cumsum(np.bincount(r_img[first], minlength=n_img))]).astype(np.int64)
    return boff, r_key[first].astype(np.uint64), mx.astype(np.int32)


class AccuracyReferences:
    """The reference captions of the evaluated images as the device needs them: the id map (model words keep the model's ids, other words
    get fresh ones), per image `log df` / `ref_len` and every caption cooked once (CIDEr), the per-image max-count n-gram table (BLEU) and
    the id rows (ROUGE-L).  `device="auto"`: the current GPU; `device=None`: the host tables only (`.to(device)` finishes the job)."""

    def __init__(self, ref_sentences, ix_to_word, device="auto"):
        from .consensus import ConsensusCorpus
        if len(ref_sentences) < 1:
            raise SubgcError("accuracy: no reference images")
        for j, caps in enumerate(ref_sentences):
            if len(caps) < 1:
                raise SubgcError(f"accuracy: image {j} has 0 reference captions; every evaluated image needs at least 1")
            if len(caps) > MAX_REFS:
                raise SubgcError(f"accuracy: image {j} has {len(caps)} reference captions; the limit is {MAX_REFS}")
            for cap in caps:
                if isinstance(cap, str):
                    raise SubgcError("accuracy: reference captions are lists of words (already tokenised), not strings")
                if len(cap) > MAX_REF_WORDS:
                    raise SubgcError(f"accuracy: a reference caption of {len(cap)} words (image {j}); the limit is {MAX_REF_WORDS}")
        model_words = set(ix_to_word.values())
        fresh = {w for caps in ref_sentences for cap in caps for w in cap} - model_words
        n_ids = max((int(k) for k in ix_to_word), default=0) + len(fresh)
        if n_ids > MAX_IDS:
            raise SubgcError(f"accuracy: the references need {n_ids} word ids, the 16-bit n-gram lanes hold {MAX_IDS} "
                             f"(model vocabulary {len(ix_to_word)} + {len(fresh)} reference-only words)")
        c = ConsensusCorpus(ref_sentences, ix_to_word, device=None)
        self.corpus = c
        self.ix_to_word, self.word_to_ix, self.n_ids = ix_to_word, c.word_to_ix, c.n_ids
        self.n_img, self.n_caps = c.n_img, c.n_caps
        self.words, self.woff, self.cap_off = c.words, c.woff, c.cap_off
        self.ukeys, self.ulogdf, self.ref_len, self.gauss, self.bad = c.ukeys, c.ulogdf, c.ref_len, c.gauss, c.bad
        self.boff, self.bkeys, self.bmax = bleu_table(self.words, self.woff, self.cap_off)
        self.device = None
        if device is not None:
            self.to(_scoring.resolve_device(device))

    def to(self, device):
        """Upload the tables and cook every reference caption (one launch); done once."""
        import torch
        dev = torch.device(device)
        self.corpus.to(dev)
        c = self.corpus
        self.d_words = c.d_words if len(self.words) else torch.zeros(1, dtype=torch.int32, device=dev)
        self.d_boff = torch.from_numpy(self.boff.astype(np.int32)).to(dev)
        self.d_bkeys = torch.from_numpy((self.bkeys if len(self.bkeys) else np.zeros(1, np.uint64)).view(np.int64)).to(dev)
        self.d_bmax = torch.from_numpy(self.bmax if len(self.bmax) else np.zeros(1, np.int32)).to(dev)
        self.device = dev
        return self

    def encode(self, words):
        """A caption (list of words, or a string split at white space) -> ids; a word neither the model nor the references know is refused."""
        if isinstance(words, str):
            words = words.split()
        try:
            return [self.word_to_ix[w] for w in words]
        except KeyError as e:
            raise SubgcError(f"accuracy: word {e.args[0]!r} is neither in the model's vocabulary nor in the references") from None


class AccuracyScorer:
    """`language_eval` for a decode batch.  oracle_num: the reference's `--oracle_num` (the oracle looks at each image's first oracle_num
    captions; 1 = the top-1 caption alone)."""

    def __init__(self, refs, oracle_num=20):
        if int(oracle_num) < 1:
            raise SubgcError(f"accuracy: oracle_num = {oracle_num}; at least 1 caption per image is scored")
        self.refs, self.oracle_num = refs, int(oracle_num)

    @staticmethod
    def arena_words(rows, I):
        """int32 words of a batch's results: the fp64 records first (8-byte aligned when the slice is), then the integer ones."""
        return 2 * (ROW_F64 * rows + IMG_F64 * I) + ROW_INT * rows + IMG_INT * I

    def check_index(self, image_index):
        return _scoring.check_index("accuracy", image_index, self.refs.n_img)

    def enqueue(self, seq, seg, I, d_index, first, remove_bad_endings, arena, oracle=True):
        """The cook launch and the two accuracy launches on the current stream (`oracle=False`: the row records alone, without the per-image
        launch -- the self-critical reward reads nothing else).  seq: device token rows [rows, T] (int32 / int64) in caption
        order; seg: device int32 row boundaries (>= I + 1 entries); d_index: device int32 [I], the reference image of every batch image;
        first: device int32 [I] image-local top-1 rows or None (row 0); arena: device int32 [arena_words(rows, I)], 8-byte aligned."""
        import torch
        from . import ops
        r = self.refs
        if r.device is None:
            raise SubgcError("accuracy: the references are not on a device (AccuracyReferences(..., device=...) or .to(device))")
        t64, T = _scoring.token_rows("accuracy", seq, MAX_T)
        rows = seq.size(0)
        if arena.numel() < self.arena_words(rows, I) or arena.data_ptr() % 8:
            raise SubgcError("accuracy: the result arena is too short or not 8-byte aligned")
        c = r.corpus
        bad = c.d_bad if remove_bad_endings else None
        row_d, row_i, img_d, img_i = self.views(arena, rows, I)
        ck, cw, cc, cl, cn = ops.consensus_cook(seq, c.d_ukeys, c.d_ulogdf, c.ref_len, bad=bad)
        rk, rw, rc, rl, rn = c.cooked
        P, s = ops._ptr, ops._stream()
        call_metrics("subgc_accuracy_rows", P(seq), t64, int(T), P(bad, torch.uint8), 0 if bad is None else bad.numel(),
                     int(rows), P(seg, torch.int32), int(I), P(d_index, torch.int32), r.n_img, P(ck, torch.int64), P(cw, torch.float64),
                     P(cc, torch.int32), P(cl, torch.int32), P(cn, torch.float64), P(c.d_cap_off, torch.int32), r.n_caps,
                     P(c.d_woff, torch.int32), P(r.d_words, torch.int32), len(r.words), P(rk, torch.int64), P(rw, torch.float64),
                     P(rc, torch.int32), P(rl, torch.int32), P(rn, torch.float64), P(r.d_boff, torch.int32), P(r.d_bkeys, torch.int64),
                     P(r.d_bmax, torch.int32), len(r.bkeys), P(c.d_gauss, torch.float64), c.d_gauss.numel(), BETA2, P(row_i), ROW_INT,
                     P(row_d), ROW_F64, s)
        if not oracle:
            return
        call_metrics("subgc_accuracy_oracle", P(row_i), ROW_INT, P(row_d), ROW_F64, int(rows), P(seg, torch.int32), int(I), self.oracle_num,
                     P(first, torch.int32), P(img_i), IMG_INT, P(img_d), IMG_F64, s)

    @staticmethod
    def views(arena, rows, I):
        """(row fp64 [rows, 6], row int32 [rows, 10], image fp64 [I, 12], image int32 [I, 56]) views of an arena (torch or numpy)."""
        f64 = _scoring.dtypes(arena).float64
        n_d = 2 * (ROW_F64 * rows + IMG_F64 * I)
        d = arena[:n_d].view(f64)
        i0 = n_d + ROW_INT * rows
        return (d[:ROW_F64 * rows].reshape(rows, ROW_F64), arena[n_d:i0].reshape(rows, ROW_INT), d[ROW_F64 * rows:].reshape(I, IMG_F64),
                arena[i0:i0 + IMG_INT * I].reshape(I, IMG_INT))

    def batch_pass(self, arg, batch, slots):
        """The accuracy pass of `eval_collect` (arg: its `accuracy=`): the images' reference indices go up with the batch; the top-1 row
        is `batch.c_first` (the consensus pass's first choice) when there is one, row 0 otherwise."""
        rows, I = batch.rows, batch.I
        index = self.check_index(arg["index"])
        if len(index) != I:
            raise SubgcError("eval_collect: accuracy needs one reference-image index per image")
        n = self.arena_words(rows, I)
        s_index, w, live = slots.ints(index), slots.words(n, align8=True), bool(I and rows)

        def enqueue():
            if live:
                self.enqueue(batch.seq_s, batch.seg, I, slots.seg[s_index], batch.c_first, arg.get("remove_bad_endings", 0), slots.arena[w])

        return enqueue, lambda host: {"a_words": host[w].copy() if live else np.zeros(n, np.int32)}

    def unpack(self, host, bounds):
        """The host copy of an arena -> per image a dict of plain numpy data:
        "n" rows, "oracle_num", "considered" = min(n, oracle_num); per row "material" int64 [n, 10] (testlen, reflen, guess[4], correct[4])
        and "values" fp64 [n, 6] (sentence BLEU-1 .. 4, CIDEr, ROUGE-L); "top1_row", "top1_material" [10], "top1_values" [6];
        "oracle_rows" [4] (first arg-max of each BLEU order), "oracle_material" [4, 10], "oracle_values" [6] (the six maxima)."""
        rows, I = int(bounds[-1]), len(bounds) - 1
        host = np.ascontiguousarray(host)
        row_d, row_i, img_d, img_i = self.views(host, rows, I)
        out = []
        for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
            e = {"n": int(b - a), "oracle_num": self.oracle_num, "considered": int(img_i[i, 0]),
                 "material": row_i[a:b].astype(np.int64), "values": row_d[a:b].copy(),
                 "top1_row": int(img_i[i, 1]), "top1_material": img_i[i, 2:12].astype(np.int64), "top1_values": img_d[i, :6].copy(),
                 "oracle_rows": img_i[i, 12:16].astype(np.int64), "oracle_material": img_i[i, 16:56].astype(np.int64).reshape(4, ROW_INT),
                 "oracle_values": img_d[i, 6:12].copy()}
            out.append(e)
        return out

    def score(self, seq, bounds, image_index, first=None, remove_bad_endings=0):
        """seq [rows, T]: device token rows, image i owning rows bounds[i] .. bounds[i+1]-1 in caption (sGPN-ranked) order;
        image_index[i]: its image in the references; first: optional per-image top-1 rows (default row 0).
        -> the per-image list of `unpack`.  Three launches, one host copy."""
        import torch
        from . import ops
        if not seq.is_cuda:
            raise SubgcError("subgc ops need device tensors (the HIP path has no CPU fallback)")
        rows, I = seq.size(0), len(bounds) - 1
        if int(bounds[-1]) != rows or len(image_index) != I or (first is not None and len(first) != I):
            raise SubgcError("accuracy: bounds / image_index / first do not cover the rows and images of seq")
        idx = self.check_index(image_index)
        bounds = [int(b) for b in bounds]
        words = self.arena_words(rows, I)
        if I == 0:
            return []
        dev = seq.device
        tab = ops.upload(bounds + idx + ([] if first is None else [int(f) for f in first]), torch.int32, dev)
        arena = torch.empty(max(words, 2), device=dev, dtype=torch.int32)
        self.enqueue(seq.contiguous(), tab, I, tab[I + 1:2 * I + 1], None if first is None else tab[2 * I + 1:], remove_bad_endings, arena)
        return self.unpack(arena.cpu().numpy(), bounds)                      # the one copy


def chunk_entries(arg, h, bounds):
    """`caption_images(accuracy=...)`: what every image's entry gains from `eval_collect`'s outputs `h` (None: a batch without rows, every image the entry of no captions)."""
    sc = arg["scorer"]
    if h is None:
        return [{"accuracy": sc.unpack(np.zeros(sc.arena_words(0, 1), np.int32), [0, 0])[0]} for _ in bounds[1:]]
    return [{"accuracy": e} for e in sc.unpack(h["a_words"], bounds)]


def corpus_bleu(material):
    """`cal_bleu`'s expressions (sentence_utils.py:43-52) over summed material [10]: python ints in, four python floats out."""
    testlen, reflen = int(material[0]), int(material[1])
    guess, correct = [int(x) for x in material[2:6]], [int(x) for x in material[6:10]]
    small = 1e-9; tiny = 1e-15; bleus = []; bleu = 1.
    for k in range(4):
        bleu *= float(correct[k] + tiny) / (guess[k] + small)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        for k in range(4):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus


def summarize(per_image):
    """The per-image entries of `AccuracyScorer.score` (or the `"accuracy"` entries of `caption_images`) -> the corpus numbers under the
    reference's names: "Bleu_1" .. "Bleu_4", "CIDEr", "ROUGE_L" of the top-1 captions (corpus BLEU of the summed material; np.mean of the
    per-image CIDEr / ROUGE-L) and "oracle": the same names over the oracle picks (`cal_bleu` of the material of each order's picks,
    sentence_utils.py:108-116; np.mean of the per-image maxima, :119-122).  "images": how many entered; an image without captions has
    nothing to score and is left out ("left_out" counts them)."""
    live = [e for e in per_image if e["n"] > 0]
    out = {"images": len(live), "left_out": len(per_image) - len(live), "oracle": {}}
    if not live:
        return out
    top = [sum(int(e["top1_material"][q]) for e in live) for q in range(ROW_INT)]
    for k, b in enumerate(corpus_bleu(top)):
        out[NAMES[k]] = b
    out["CIDEr"] = float(np.mean(np.array([e["top1_values"][4] for e in live])))
    out["ROUGE_L"] = float(np.mean(np.array([e["top1_values"][5] for e in live])))
    for k in range(4):
        tot = [sum(int(e["oracle_material"][k][q]) for e in live) for q in range(ROW_INT)]
        out["oracle"][NAMES[k]] = corpus_bleu(tot)[k]
    out["oracle"]["CIDEr"] = float(np.mean(np.array([e["oracle_values"][4] for e in live])))
    out["oracle"]["ROUGE_L"] = float(np.mean(np.array([e["oracle_values"][5] for e in live])))
    return out


def encode_predictions(predictions, refs):
    """A finished `predictions` list (eval_utils.py:132-141: per image 'caption' strings) -> (seq int64 [rows, T], bounds): every caption
    split at white space and mapped through the references' id map; a word outside it is refused."""
    rows, bounds = [], [0]
    for p in predictions:
        for c in p["caption"]:
            try:
                rows.append(refs.encode(c))
            except SubgcError as e:
                raise SubgcError(f"{e} (a caption of image {p.get('image_id')!r})") from None
        bounds.append(len(rows))
    return _scoring.id_rows("accuracy", rows, MAX_T), bounds


def score_predictions(predictions, refs, ix_to_word, oracle_num=1, remove_bad_endings=0, device="auto", verbose=True):
    """The drop-in for `--only_sent_eval 1 --oracle_num N` on a `captions_*.npy`-style list.  refs: {image_id: [reference captions, each a
    list of words]} covering every image of `predictions` (or an AccuracyReferences built over the predictions' images in their order).
    remove_bad_endings trims the candidates by `decode_sequence`'s rule (for captions written without it).
    Prints the lines the reference prints (eval.py:83 per metric; sentence_utils.py:116-122 for the oracle) and returns
    (summarize(...), the per-image entries)."""
    import torch
    if not isinstance(refs, AccuracyReferences):
        missing = [p["image_id"] for p in predictions if p["image_id"] not in refs]
        if missing:
            raise SubgcError(f"accuracy: no reference captions for image ids {missing[:5]}")
        refs = AccuracyReferences([refs[p["image_id"]] for p in predictions], ix_to_word, device=None)
    if refs.n_img != len(predictions):
        raise SubgcError(f"accuracy: {len(predictions)} images predicted, the references hold {refs.n_img}")
    dev = _scoring.resolve_device(device)
    if refs.device is None:
        refs.to(dev)
    seq, bounds = encode_predictions(predictions, refs)
    per_image = AccuracyScorer(refs, oracle_num).score(torch.from_numpy(seq).to(dev), bounds, list(range(len(predictions))),
                                                       remove_bad_endings=remove_bad_endings)
    s = summarize(per_image)
    if verbose and s["images"]:
        for name in NAMES:
            print("%s: %0.3f" % (name, s[name]))
        if oracle_num != 1:
            print("\n\nThe following is top-{}: ".format(oracle_num))
            for k in range(4):
                print("oracle {}: {}".format(NAMES[k], s["oracle"][NAMES[k]]))
            print("oracle cider: {}".format(s["oracle"]["CIDEr"]))
            print("oracle rouge: {}".format(s["oracle"]["ROUGE_L"]))
    return s, per_image
