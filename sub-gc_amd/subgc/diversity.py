"""Diversity scores of a whole decode batch on the device (misc/diversity/diversity_score.py:55-163; the sentence BLEU-4 of its
mBLEU-4 is misc/diversity/bleu_scorer.py:26-93,248-256).

The reference scores the captions `eval_split` wrote (`captions_*.npy`) with four Python loops over strings: Distinct Caption (metric 1),
Novel Caption (2), 1-gram / 2-gram diversity (3) and mBLEU-4 (4), each over a random draw of 20 / 100 of an image's captions and -- all
but the first -- over the best 5 of that draw by sGPN score.  Here the token rows, scores and row boundaries of a decode batch are
already on the device in that order; three launches (`subgc_diversity_select / _distinct / _best`) take them to integer counts and fp64
BLEU values, one workgroup per (image, draw).  Ratios and means are formed on the host in float64 from the integer counts (`summarize`),
so every number but mBLEU-4 equals the script's bit for bit; mBLEU-4 agrees to a few ulp.

The draws are an input of the device path.  The script seeds numpy once and runs the metrics in the order 4, 3, 2, 1 over the whole
file, so image i's draws depend on every image before it and on `--evaluate_mB4`: `reference_draws` reproduces exactly that stream (for
comparing against the script), `per_image_draws` gives draws that depend on (seed, image key, metric, top_n) alone, so that batching
and sharding cannot change a result -- `eval_glue.caption_images(diversity=...)` uses those.

Tie rule: `np.argsort` leaves the order of equal scores open.  On the device, among equal scores the row LATER in the draw comes first
(a stable ascending sort, reversed).

`NoveltyIndex(train_strings, ix_to_word)`: the training captions as the sorted id lists the device searches.  `train_strings` are the raw
captions (the script's `all_cap_dict[img_id]` entries of the training images); each becomes `lower().replace('.', '')` and is split at
single spaces, as the script's string comparison implies.  A caption holding ANY word outside the model's vocabulary -- including the
empty word a double or trailing space produces -- is dropped: it can never equal a generated caption, whose words all come from
`ix_to_word` joined by single spaces, so equality stays exact.  The empty string is kept as the zero-word caption.

An image with fewer than 2 captions has no mBLEU-4 (the reference asserts there, bleu.py:38): its `mbleu4_valid` is False and
`summarize` leaves it out of the mean and counts it.

Out of scope: PTB tokenisation (the model's captions are lower-case words joined by single spaces already) and the COCO metric scripts.
"""
from __future__ import annotations

import hashlib

import numpy as np

from ._lib import SubgcError
from ._scoring import MAX_IDS, bad_table, id_rows, resolve_device

MAX_DRAW = 1024          # rows of one draw
MAX_T = 64               # words of a token row
METRICS = (4, 3, 2, 1)   # the script's order
TOP_N = (20, 100)


def reference_draws(sub_nums, top_n=TOP_N, evaluate_mB4=False, seed=2019):
    """The script's own draws: {metric: [per image [per top_n: int64 array of caption indices]]}, from the legacy numpy stream seeded once
    (`np.random.seed(2019)`, diversity_score.py:8), metrics in the order 4 (only with evaluate_mB4), 3, 2, 1, images inside, top_n inside
    that (`np.random.choice(sub_num, min(top_k, sub_num), replace=False)`, :63, :92, :139, :157)."""
    rs = np.random.RandomState(seed)
    out = {}
    for metric in METRICS:
        if metric == 4 and not evaluate_mB4:
            continue
        out[metric] = [[rs.choice(int(n), min(int(k), int(n)), replace=False).astype(np.int64) for k in top_n] for n in sub_nums]
    return out


def per_image_draws(sub_nums, image_keys, top_n=TOP_N, seed=2019):
    """Draws of the same shape as `reference_draws` (all four metrics) that depend only on (seed, image key, metric, top_n) and the image's
    own caption count: the order of the list, the batch an image falls into and the rank that captions it cannot change them."""
    if len(sub_nums) != len(image_keys):
        raise SubgcError("diversity: one image key per image")
    out = {m: [] for m in METRICS}
    for n, key in zip(sub_nums, image_keys):
        for metric in METRICS:
            per = []
            for k in top_n:
                h = hashlib.sha256(repr((int(seed), key if isinstance(key, str) else int(key), int(metric), int(k))).encode()).digest()
                rs = np.random.RandomState(np.frombuffer(h, np.uint32))
                per.append(rs.choice(int(n), min(int(k), int(n)), replace=False).astype(np.int64) if int(n) > 0 else np.zeros(0, np.int64))
            out[metric].append(per)
    return out


def _inverse_vocab(ix_to_word):
    w2i = {}
    for k, w in ix_to_word.items():
        ix = int(k)
        if not 1 <= ix <= MAX_IDS:
            raise SubgcError(f"diversity: ix_to_word holds id {ix}; word ids are 1 .. {MAX_IDS} (0 ends a caption, n-gram lanes are 16 bits)")
        if w in w2i:
            raise SubgcError(f"diversity: ix_to_word maps both {w2i[w]} and {ix} to {w!r}: ids and words must correspond one to one")
        w2i[w] = ix
    return w2i


class NoveltyIndex:
    """The set of training captions (diversity_score.py:127-131) as distinct id lists in lexicographic order (a prefix first), CSR;
    see the module docstring for what is kept and dropped.  `.captions`: the kept id tuples, `.dropped`: how many strings were dropped.
    `device="auto"`: the current GPU; `device=None`: host tables only (`.to(device)` uploads later)."""

    def __init__(self, train_strings, ix_to_word, device="auto"):
        self.ix_to_word = ix_to_word
        self.word_to_ix = w2i = _inverse_vocab(ix_to_word)
        caps, dropped = set(), 0
        for s in train_strings:
            s = s.lower().replace(".", "")
            if s == "":
                caps.add(())
                continue
            try:
                caps.add(tuple(w2i[w] for w in s.split(" ")))
            except KeyError:
                dropped += 1
        self.captions, self.dropped = caps, dropped
        order = sorted(caps)
        self.n = len(order)
        self.off = np.concatenate([[0], np.cumsum([len(c) for c in order], dtype=np.int64)]).astype(np.int64)
        if self.off[-1] >= 1 << 31:
            raise SubgcError("diversity: the training captions hold 2^31 words or more")
        self.tok = np.asarray([w for c in order for w in c], np.int32)
        self.device = None
        if device is not None:
            self.to(resolve_device(device))

    def to(self, device):
        import torch
        dev = torch.device(device)
        self.d_off = torch.from_numpy(self.off.astype(np.int32)).to(dev)
        self.d_tok = torch.from_numpy(self.tok if len(self.tok) else np.zeros(1, np.int32)).to(dev)
        self.device = dev
        return self

    def __contains__(self, caption):
        """A GENERATED caption (words of the vocabulary joined by single spaces; '' = no words) -- the script's `sen_i in train_sents`."""
        if caption == "":
            return () in self.captions
        try:
            return tuple(self.word_to_ix[w] for w in caption.split(" ")) in self.captions
        except KeyError:
            return False


def _check_draws(draws, sizes):
    nt = None
    for metric, per in draws.items():
        if metric not in METRICS:
            raise SubgcError(f"diversity: draws of metric {metric!r}; the metrics are 1 (distinct), 2 (novel), 3 (n-grams), 4 (mBLEU-4)")
        if len(per) != len(sizes):
            raise SubgcError(f"diversity: metric {metric} has draws for {len(per)} images, the batch holds {len(sizes)}")
        for i, d in enumerate(per):
            if nt is None:
                nt = len(d)
            if len(d) != nt:
                raise SubgcError("diversity: every image and metric needs one draw per top_n")
            for x in d:
                if len(x) > MAX_DRAW:
                    raise SubgcError(f"diversity: a draw of {len(x)} rows (image {i}, metric {metric}); the limit is {MAX_DRAW}")
    return nt or 0


class DiversityScorer:
    """`diversity_score.py` for a decode batch.  novelty: a NoveltyIndex (None: no Novel Caption count); n_best: the script's best 5;
    ix_to_word: only needed for `remove_bad_endings` when there is no novelty index to take the vocabulary from."""

    def __init__(self, novelty=None, n_best=5, ix_to_word=None):
        if not 2 <= int(n_best) <= 16:
            raise SubgcError(f"diversity: n_best = {n_best}; 2 <= n_best <= 16")
        self.novelty, self.n_best = novelty, int(n_best)
        vocab = ix_to_word if ix_to_word is not None else (novelty.ix_to_word if novelty is not None else None)
        self.bad = None if vocab is None else bad_table(vocab)
        self._d_bad = None

    def plan(self, draws, sizes):
        """Host side of a batch: the sets (metric, image, top_n) of `draws` flattened into ONE int32 table
        [set_img | set_flags | set_off | draw] -> {"table", "n_sets", "n_draw", "max_draw", "index": [(metric, image, t)], "n_top", "I"}."""
        from .ops import DIV_WANT
        nt = _check_draws(draws, sizes)
        img, flags, lens, index, flat = [], [], [], [], []
        for metric in METRICS:
            if metric not in draws or (metric == 2 and self.novelty is None):
                continue
            for i, per in enumerate(draws[metric]):
                for t, d in enumerate(per):
                    img.append(i)
                    flags.append(DIV_WANT[metric])
                    lens.append(len(d))
                    index.append((metric, i, t))
                    flat.append(np.asarray(d, np.int64))
        S = len(img)
        off = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
        draw = np.concatenate(flat).astype(np.int64) if flat else np.zeros(0, np.int64)
        if len(draw) and (draw.min() < -(1 << 31) or draw.max() >= 1 << 31):
            raise SubgcError("diversity: a draw index does not fit 32 bits")
        table = np.concatenate([np.asarray(img, np.int64), np.asarray(flags, np.int64), off, draw]).astype(np.int32)
        return {"table": table, "n_sets": S, "n_draw": int(off[-1]), "max_draw": max(lens, default=0), "index": index, "n_top": nt, "I": len(sizes)}

    def enqueue(self, seq, score, seg, I, plan, remove_bad_endings, out_i, out_d):
        """The three launches on the current stream.  seq: device token rows [rows, T] (int32 / int64), score fp32 [rows], both in the
        images' ranked order; seg: device int32 row boundaries (>= I + 1 entries); out_i int32 [sets, DIV_COLS + n_best], out_d fp64
        [sets, n_best + 1]: device outputs."""
        import torch
        from . import ops
        S = plan["n_sets"]
        if S == 0:
            return
        if plan["I"] != I:
            raise SubgcError("diversity: the plan was made for another batch")
        if seq.size(1) > MAX_T:
            raise SubgcError(f"diversity: token rows of {seq.size(1)} words; the limit is {MAX_T}")
        dev = seq.device
        bad = None
        if remove_bad_endings:
            if self.bad is None:
                raise SubgcError("diversity: remove_bad_endings needs the vocabulary (DiversityScorer(..., ix_to_word=...) or a NoveltyIndex)")
            if self._d_bad is None or self._d_bad.device != dev:
                self._d_bad = torch.from_numpy(self.bad).to(dev)
            bad = self._d_bad
        nv = self.novelty
        if nv is not None and nv.device is None:
            raise SubgcError("diversity: the novelty index is not on a device (NoveltyIndex(..., device=...) or .to(device))")
        tab = ops.upload(plan["table"], torch.int32, dev)
        set_img, set_flags, set_off, draw = tab[:S], tab[S:2 * S], tab[2 * S:3 * S + 1], tab[3 * S + 1:]
        ops.diversity_select(score, seg, I, seq.size(0), set_img, set_off, draw, S, plan["n_draw"], plan["max_draw"], self.n_best, out_i)
        ops.diversity_distinct(seq, bad, seg, I, set_img, set_off, set_flags, draw, S, plan["n_draw"], plan["max_draw"], out_i)
        ops.diversity_best(seq, bad, seg, I, set_img, set_flags, S, self.n_best, None if nv is None else nv.d_off,
                           None if nv is None else nv.d_tok, 0 if nv is None else nv.n, out_i, out_d)

    def batch_pass(self, arg, batch, slots):
        """The diversity pass of `eval_collect` (arg: its `diversity=`): the sets' fp64 values, then their integer columns."""
        import torch
        from .ops import DIV_COLS
        plan, S, nb = arg["plan"], arg["plan"]["n_sets"], self.n_best
        w_d, w_i = slots.words(2 * S * (nb + 1), align8=True), slots.words(S * (DIV_COLS + nb))

        def enqueue():
            if S:
                self.enqueue(batch.seq_s, batch.score_s, batch.seg, batch.I, plan, arg.get("remove_bad_endings", 0),
                             slots.arena[w_i].view(S, DIV_COLS + nb), slots.arena[w_d].view(torch.float64).view(S, nb + 1))

        return enqueue, lambda host: {"d_f64": host[w_d].view(np.float64).reshape(S, nb + 1).copy(), "d_int": host[w_i].reshape(S, DIV_COLS + nb).copy()}

    def unpack(self, plan, h_int, h_f64, top_n=None):
        """Host results of a plan -> per image {"drawn", "distinct" (metric 1), "words", "unigrams", "bigrams" (3), "novel", "novel_of" (2:
        novel captions among `novel_of` selected ones), "bleu4" [n_top, n_best] (NaN past the selection), "mbleu4", "mbleu4_valid",
        "selected" [n_top, n_best] (4: the chosen caption indices, -1 past the count)}: int64 / float64 / bool arrays with one entry per
        top_n; a metric without draws leaves its keys out."""
        from .ops import DIV_COLS
        nt, nb = plan["n_top"], self.n_best
        out = [dict() if top_n is None else {"top_n": [int(k) for k in top_n]} for _ in range(plan["I"])]

        def slot(e, key, dtype, shape=()):
            if key not in e:
                e[key] = np.zeros((nt,) + shape, dtype)
            return e[key]

        for s, (metric, i, t) in enumerate(plan["index"]):
            e, r = out[i], h_int[s]
            if metric == 1:
                slot(e, "drawn", np.int64)[t] = r[0]
                slot(e, "distinct", np.int64)[t] = r[1]
            elif metric == 3:
                slot(e, "words", np.int64)[t] = r[3]
                slot(e, "unigrams", np.int64)[t] = r[4]
                slot(e, "bigrams", np.int64)[t] = r[5]
            elif metric == 2:
                slot(e, "novel", np.int64)[t] = r[6]
                slot(e, "novel_of", np.int64)[t] = r[2]
            else:
                n = int(r[2])
                b = slot(e, "bleu4", np.float64, (nb,))
                b[t] = np.nan
                b[t, :n] = h_f64[s, :n] if r[7] else np.nan
                slot(e, "mbleu4", np.float64)[t] = h_f64[s, nb] if r[7] else np.nan
                slot(e, "mbleu4_valid", bool)[t] = bool(r[7])
                slot(e, "selected", np.int64, (nb,))[t] = r[DIV_COLS:DIV_COLS + nb]
        return out

    def score(self, seq, bounds, score, draws, remove_bad_endings=0):
        """seq [rows, T]: device token rows, image i owning rows bounds[i] .. bounds[i+1]-1 in sGPN-ranked order; score [rows]: their
        fp32 sGPN scores; draws: {metric: [per image [per top_n: caption indices]]} (`reference_draws` / `per_image_draws`).
        -> the per-image list of `unpack`.  Three launches, one host copy."""
        import torch
        from . import ops
        if not seq.is_cuda or not score.is_cuda:
            raise SubgcError("subgc ops need device tensors (the HIP path has no CPU fallback)")
        rows, I = seq.size(0), len(bounds) - 1
        if bounds[-1] != rows or score.numel() != rows:
            raise SubgcError("diversity: bounds / score do not cover the rows of seq")
        sizes = [b - a for a, b in zip(bounds, bounds[1:])]
        plan = self.plan(draws, sizes)
        S, nb = plan["n_sets"], self.n_best
        if S == 0 or I == 0:
            return self.unpack(plan, np.zeros((0, ops.DIV_COLS + nb), np.int32), np.zeros((0, nb + 1)))
        dev = seq.device
        seg = ops.upload([int(b) for b in bounds], torch.int32, dev)
        n_f64 = 2 * S * (nb + 1)
        arena = torch.empty(n_f64 + S * (ops.DIV_COLS + nb), device=dev, dtype=torch.int32)
        out_d = arena[:n_f64].view(torch.float64).view(S, nb + 1)
        out_i = arena[n_f64:].view(S, ops.DIV_COLS + nb)
        self.enqueue(seq.contiguous(), score.contiguous().float() if score.dtype != torch.float32 else score.contiguous(), seg, I, plan,
                     remove_bad_endings, out_i, out_d)
        host = arena.cpu().numpy()                                          # the one copy
        return self.unpack(plan, host[n_f64:].reshape(S, ops.DIV_COLS + nb), host[:n_f64].view(np.float64).reshape(S, nb + 1))


def chunk_arg(arg, opt, ids, sizes):
    """`caption_images(diversity=opt)`: the chunk's argument with the plan of its draws, which are keyed by the image id
    (`per_image_draws`); "top_n" rides along for `chunk_entries`."""
    top_n = tuple(opt.get("top_n", TOP_N))
    return dict(arg, top_n=top_n, plan=opt["scorer"].plan(per_image_draws(sizes, ids, top_n, opt.get("seed", 2019)), sizes))


def chunk_entries(arg, h, bounds):
    """What every image's entry gains from `eval_collect`'s outputs `h` (None: a batch without rows, all counts zero)."""
    from .ops import DIV_COLS
    sc, S = arg["scorer"], arg["plan"]["n_sets"]
    d_int, d_f64 = (np.zeros((S, DIV_COLS + sc.n_best), np.int32), np.zeros((S, sc.n_best + 1))) if h is None else (h["d_int"], h["d_f64"])
    return [{"diversity": e} for e in sc.unpack(arg["plan"], d_int, d_f64, arg["top_n"])]


def summarize(per_image):
    """The per-image entries of `DiversityScorer.score` (or the `"diversity"` entries of `caption_images`) -> the numbers the script
    prints, each a list with one value per top_n: "mbleu4" (:81-82; the mean over the images with a valid value, "mbleu4_left_out" counts
    the others), "unigram" / "bigram" (:110-113), "novel" (:146-147, a sum), "distinct" (:162-163), and "printed": all of them in the
    script's print order.  Ratios are float64 divisions of the integer counts, means are np.mean over the images in list order -- the
    script's own expressions.  An image without captions has no ratio and is left out."""
    out = {}
    if not per_image:
        return out
    keys = set().union(*[set(e) for e in per_image])
    nt = max((len(np.atleast_1d(v)) for e in per_image for k, v in e.items() if k != "top_n"), default=0)
    printed = []
    if "mbleu4" in keys:
        out["mbleu4"], out["mbleu4_left_out"] = [], []
        for t in range(nt):
            vals = [e["mbleu4"][t] for e in per_image if e["mbleu4_valid"][t]]
            out["mbleu4"].append(float(np.mean(np.array(vals))) if vals else float("nan"))
            out["mbleu4_left_out"].append(len(per_image) - len(vals))
        printed += out["mbleu4"]
    if "words" in keys:
        out["unigram"], out["bigram"] = [], []
        for t in range(nt):
            live = [e for e in per_image if e["words"][t] > 0]
            out["unigram"].append(float(np.mean(np.array([int(e["unigrams"][t]) / float(int(e["words"][t])) for e in live]))) if live else float("nan"))
            out["bigram"].append(float(np.mean(np.array([int(e["bigrams"][t]) / float(int(e["words"][t])) for e in live]))) if live else float("nan"))
            printed += [out["unigram"][-1], out["bigram"][-1]]
    if "novel" in keys:
        out["novel"] = [int(sum(int(e["novel"][t]) for e in per_image)) for t in range(nt)]
        printed += out["novel"]
    if "drawn" in keys:
        out["distinct"] = []
        for t in range(nt):
            live = [e for e in per_image if e["drawn"][t] > 0]
            out["distinct"].append(float(np.mean(np.array([int(e["distinct"][t]) / float(int(e["drawn"][t])) for e in live]))) if live else float("nan"))
        printed += out["distinct"]
    out["printed"] = printed
    return out


def encode_predictions(predictions, ix_to_word):
    """A finished `predictions` list (eval_utils.py:132-141: 'caption' strings, 'subgraph_score') -> (seq int64 [rows, T], bounds, score
    fp32 [rows]) through the inverse vocabulary; a word outside it is refused."""
    w2i = _inverse_vocab(ix_to_word)
    rows, bounds, scores = [], [0], []
    for p in predictions:
        sc = np.asarray(p["subgraph_score"], np.float32).reshape(-1)
        if len(sc) != len(p["caption"]):
            raise SubgcError(f"diversity: image {p.get('image_id')!r} has {len(p['caption'])} captions and {len(sc)} scores")
        for c in p["caption"]:
            try:
                rows.append([w2i[w] for w in c.split(" ")] if c != "" else [])
            except KeyError as e:
                raise SubgcError(f"diversity: word {e.args[0]!r} of a caption of image {p.get('image_id')!r} is not in the vocabulary") from None
        scores.append(sc)
        bounds.append(len(rows))
    return id_rows("diversity", rows, MAX_T), bounds, (np.concatenate(scores) if scores else np.zeros(0, np.float32))


def score_predictions(predictions, ix_to_word, novelty=None, evaluate_mB4=False, top_n=TOP_N, seed=2019, n_best=5, device="auto"):
    """The drop-in for running diversity_score.py on a `captions_*.npy`: the `predictions` list re-encoded through the inverse vocabulary,
    the script's own draws (`reference_draws`), one scoring pass on the device.  -> (summarize(...), the per-image entries)."""
    import torch
    seq, bounds, score = encode_predictions(predictions, ix_to_word)
    dev = resolve_device(device)
    draws = reference_draws([b - a for a, b in zip(bounds, bounds[1:])], top_n, evaluate_mB4, seed)
    scorer = DiversityScorer(novelty, n_best, ix_to_word=ix_to_word)
    per_image = scorer.score(torch.from_numpy(seq).to(dev), bounds, torch.from_numpy(score).to(dev), draws)
    return summarize(per_image), per_image
