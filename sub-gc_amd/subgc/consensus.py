"""Consensus re-ranking, methods 'cider' and 'bleu', of a whole decode batch on the device
(misc/consensus_reranking/cr_mRNN_demo.py -> concensus_reranking_utils/consensus_reranking.py:122-179; the pair scores are
CiderScorer.compute_cider_sen_pair, external/coco_caption_patch_mRNN_cr/cider_scorer_compute_sentence.py:187-264, and
calculate_bleu_sentence, concensus_reranking_utils/bleu_score_util.py:15-61).

The reference re-ranks each image's candidate captions by the sum of their `m` largest similarities to the captions of the image's
`k` nearest training images -- a triple Python loop over string-keyed dictionaries, run on the captions `eval_split` wrote.  Here words
become 16-bit ids once on the host, an n-gram is one 64-bit key, and three launches (`subgc_consensus_cook / _score / _rank`, or
`subgc_consensus_bleu_cook / _bleu_score` and the same `_rank`) take the decode loop's token rows to a per-image order.
`ConsensusCorpus` is the one-time setup (numpy / torch allowed); `ConsensusReranker.rerank` / `BleuConsensusReranker.rerank` and the
`consensus=` argument of `eval_glue.caption_images` are the per-batch path and issue only C-ABI launches.  `make_reranker` picks the
class and the reference's defaults (conf_cr.py:43-48) by method name.

Tie rule: `np.argsort(-sim)` leaves the order of equal sums unspecified, and duplicate captions from different sub-graphs make exact
ties routine.  The device order is STABLE: among equal sums the lower candidate index comes first.

The neighbour lists are either the host lists the reference caches as `NNimg_list_*.npy` or a device int32 tensor -- the output of
`neighbours.ImageIndex.search` (`find_NNimg` on the device), which `caption_images(consensus={"index": ...})` runs in the same pass.

Out of scope: extracting the ResNet features the search runs over; PTB tokenisation and the COCO metric scripts.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import SubgcError
from ._scoring import MAX_IDS, bad_table, resolve_device
from .neighbours import WORKSPACE_BYTES

MAX_WORDS = 256          # words of one corpus caption (subgc_consensus_cook)
MAX_CAPS = 2048          # neighbour captions per image (subgc_consensus_score)
MAX_K = 256              # neighbour images per image
SIGMA = 6.0              # CiderScorer's default


def build_id_map(ref_sentences, ix_to_word):
    """-> (word -> id, number of ids).  Model words keep the model's id (the inverse of `ix_to_word`, so a literal 'UNK' in a caption
    is the model's UNK); words outside the vocabulary get fresh ids above it in order of first appearance: string equality and id
    equality coincide.  More than 65535 ids are refused."""
    word_to_ix = {}
    for k, w in ix_to_word.items():
        ix = int(k)
        if ix < 1:
            raise SubgcError(f"consensus: ix_to_word holds id {ix}; ids start at 1 (0 ends a caption)")
        if w in word_to_ix:
            raise SubgcError(f"consensus: ix_to_word maps both {word_to_ix[w]} and {ix} to {w!r}: ids and words must correspond one to one")
        word_to_ix[w] = ix
    nxt = max(word_to_ix.values(), default=0) + 1
    for caps in ref_sentences:
        for cap in caps:
            for w in cap:
                if w not in word_to_ix:
                    word_to_ix[w] = nxt
                    nxt += 1
    if nxt - 1 > MAX_IDS:
        raise SubgcError(f"consensus: the corpus needs {nxt - 1} word ids, the 16-bit n-gram lanes hold {MAX_IDS} "
                         f"(model vocabulary {len(ix_to_word)} + {nxt - 1 - len(ix_to_word)} corpus-only words)")
    return word_to_ix, nxt - 1


def ngram_keys(words, woff):
    """All n-grams (orders 1-4) of CSR sentences as uint64 keys (word j in bits 63-16j .. 48-16j) -> (keys, sentence index of each)."""
    words = np.asarray(words, np.uint64)
    woff = np.asarray(woff, np.int64)
    lens = np.diff(woff)
    sent = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(len(words))
    end = woff[sent + 1] if len(words) else pos
    pad = np.concatenate([words, np.zeros(3, np.uint64)])
    ks, ss = [], []
    for o in range(4):
        valid = pos + o < end
        key = pad[pos] << np.uint64(48)
        if o >= 1:
            key = key | (pad[pos + 1] << np.uint64(32))
        if o >= 2:
            key = key | (pad[pos + 2] << np.uint64(16))
        if o >= 3:
            key = key | pad[pos + 3]
        ks.append(key[valid])
        ss.append(sent[valid])
    return np.concatenate(ks), np.concatenate(ss)


def gauss_table(n=MAX_WORDS, sigma=SIGMA):
    """The length factor by |delta|, with the reference's own expression (cider_scorer_compute_sentence.py:239)."""
    return np.array([np.e ** (-(float(d) ** 2) / (2 * sigma ** 2)) for d in range(n)], np.float64)


class ConsensusCorpus:
    """The reference captions of the training images (`anno_list_ref[i]['sentences']`: per image a list of captions, each a list of
    words) as the device needs them: the id map, the sorted distinct n-gram keys with log(document frequency) -- counted per IMAGE,
    `compute_doc_freq` -- and every caption cooked once (`subgc_consensus_cook`).  `device="auto"`: the current GPU; `device=None`: the host
    tables only (id map, keys, log df: enough for tooling and CPU tests; `.to(device)` finishes the job later)."""

    def __init__(self, ref_sentences, ix_to_word, device="auto", sigma=SIGMA):
        self.ix_to_word = ix_to_word
        self.word_to_ix, self.n_ids = build_id_map(ref_sentences, ix_to_word)
        self.n_img = len(ref_sentences)
        if self.n_img < 1:
            raise SubgcError("consensus: an empty corpus")
        w2i = self.word_to_ix
        flat, lens, per_img = [], [], []
        for caps in ref_sentences:
            per_img.append(len(caps))
            for cap in caps:
                if len(cap) > MAX_WORDS:
                    raise SubgcError(f"consensus: a corpus caption of {len(cap)} words; the limit is {MAX_WORDS}")
                lens.append(len(cap))
                flat.extend(w2i[w] for w in cap)
        self.words = np.asarray(flat, np.int32)
        self.woff = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
        self.cap_off = np.concatenate([[0], np.cumsum(np.asarray(per_img, np.int64))]).astype(np.int64)
        self.n_caps = len(lens)
        self.max_words = max(lens, default=0)
        if self.woff[-1] >= 1 << 29:
            raise SubgcError("consensus: the corpus holds 2^29 words or more")
        keys, sent = ngram_keys(self.words, self.woff)
        img = np.repeat(np.arange(self.n_img), per_img)[sent] if len(sent) else sent
        o = np.lexsort((img, keys))
        keys, img = keys[o], img[o]
        fresh = np.ones(len(keys), bool)
        fresh[1:] = (keys[1:] != keys[:-1]) | (img[1:] != img[:-1])     # one count per (n-gram, image)
        self.ukeys, df = np.unique(keys[fresh], return_counts=True)
        self.ulogdf = np.log(np.maximum(1.0, df.astype(np.float64)))
        self.ref_len = float(np.log(float(self.n_img)))
        self.gauss = gauss_table(MAX_WORDS, sigma)
        self.bad = bad_table(ix_to_word)
        self.device = None
        self._bleu_cooked = None
        if device is not None:
            self.to(resolve_device(device))

    def to(self, device):
        """Upload the tables and cook every corpus caption (one launch); done once."""
        dev = torch.device(device)
        self.d_words = torch.from_numpy(self.words).to(dev)
        self.d_woff = torch.from_numpy(self.woff.astype(np.int32)).to(dev)
        self.d_cap_off = torch.from_numpy(self.cap_off.astype(np.int32)).to(dev)
        self.d_ukeys = torch.from_numpy(self.ukeys.view(np.int64)).to(dev)
        self.d_ulogdf = torch.from_numpy(self.ulogdf).to(dev)
        self.d_gauss = torch.from_numpy(self.gauss).to(dev)
        self.d_bad = torch.from_numpy(self.bad).to(dev)
        self.cooked = ops.consensus_cook(self.d_words, self.d_ukeys, self.d_ulogdf, self.ref_len, woff=self.d_woff, max_words=self.max_words)
        self._bleu_cooked = None
        self.device = dev
        return self

    def bleu_cooked(self):
        """Every corpus caption's n-gram key / count list for method 'bleu' (`subgc_consensus_bleu_cook`): one launch on first use, over
        the words and offsets `to` uploaded, then cached; the 'cider' tables are not touched."""
        if self.device is None:
            raise SubgcError("consensus: the corpus is not on a device (ConsensusCorpus(..., device=...) or .to(device))")
        if self._bleu_cooked is None:
            self._bleu_cooked = ops.consensus_bleu_cook(self.d_words, woff=self.d_woff, max_words=self.max_words)
        return self._bleu_cooked

    def encode(self, words):
        """A caption (list of words, or a string) -> ids; words the corpus never saw and the model does not know get id 0 -> refused."""
        if isinstance(words, str):
            words = words.split()
        try:
            return [self.word_to_ix[w] for w in words]
        except KeyError as e:
            raise SubgcError(f"consensus: word {e.args[0]!r} is neither in the model's vocabulary nor in the corpus") from None


class ConsensusReranker:
    """`consensus_rerank(method='cider')` for a decode batch: candidates = the (sGPN-ranked) token rows of each image, neighbours = the
    first `k` entries of the image's nearest-training-image list, score = sum of the `m` largest pair scores (defaults k_cider = 60,
    m_cider = 125 of cr_mRNN_demo.py)."""

    def __init__(self, corpus, k=60, m=125):
        if m < 1:
            raise SubgcError(f"consensus: m = {m}; at least one pair score is summed")
        if not 1 <= k <= MAX_K:
            raise SubgcError(f"consensus: k = {k}; 1 <= k <= {MAX_K} neighbour images")
        self.corpus, self.k, self.m = corpus, int(k), int(m)
        self._caps_bound = None

    def caps_bound(self):
        """The neighbour-caption capacity for lists that live on the device and cannot be read here: the sum of the k largest per-image
        caption counts of the corpus, an upper bound for every list; computed once.  A capacity only: the kernels score the captions
        that are there, so any value >= the true count gives the same bits."""
        if self._caps_bound is None:
            per_img = np.sort(np.diff(self.corpus.cap_off))
            self._caps_bound = int(per_img[-self.k:].sum())
        if self._caps_bound > MAX_CAPS:
            raise SubgcError(f"consensus: the {self.k} largest images of the corpus hold {self._caps_bound} captions; the limit is {MAX_CAPS} "
                             "neighbour captions per image, and lists on the device cannot be counted one by one")
        return self._caps_bound

    def device_neighbours(self, nn, I, device):
        """A device int32 [I, >= k] tensor of neighbour indices with unit inner stride (ImageIndex.search's `idx`) -> (it, caps_bound())."""
        if not nn.is_cuda or nn.device != device:
            raise SubgcError("consensus: a neighbour tensor lives on the device of the token rows; host lists go in as lists")
        if nn.dtype != torch.int32 or nn.dim() != 2 or nn.size(0) != I or nn.size(1) < self.k or (nn.size(1) > 1 and nn.stride(1) != 1):
            raise SubgcError(f"consensus: a neighbour tensor is int32 [{I}, >= k = {self.k}] with unit inner stride, got {nn.dtype} "
                             f"{tuple(nn.shape)} / {nn.stride()}")
        return nn, self.caps_bound()

    def neighbours(self, nn_lists):
        """-> (int32 [I, k] array of the first k neighbours, the largest neighbour-caption count of an image); host work, numpy."""
        k, c = self.k, self.corpus
        for j, l in enumerate(nn_lists):
            if len(l) < k:
                raise SubgcError(f"consensus: k = {k} is larger than the neighbour list of image {j} ({len(l)} entries)")
        nn = np.asarray([l[:k] for l in nn_lists], np.int64).reshape(len(nn_lists), k)             # one conversion for the batch
        cl = np.clip(nn, 0, c.n_img - 1)                                    # what the kernel reads for an index out of range
        caps = (c.cap_off[cl + 1] - c.cap_off[cl]).sum(1)
        max_caps = int(caps.max()) if len(caps) else 0
        if max_caps > MAX_CAPS:
            raise SubgcError(f"consensus: image {int(caps.argmax())} has {max_caps} neighbour captions; the limit is {MAX_CAPS} per image")
        return nn.astype(np.int32), max_caps

    def enqueue(self, seq, seg, I, max_rows, nn_lists, top_k, remove_bad_endings, sim, order, first=None, pair_out=None):
        """The three launches on the current stream.  seq: device token rows [rows, T] (int32 / int64) in candidate order; seg: device
        int32 row boundaries (>= I + 1 entries); sim fp64 [rows], order int32 [rows], first int32 [I]: device outputs.  nn_lists: per image
        a host list of neighbour indices, or ONE device int32 [I, >= k] tensor (`device_neighbours`), read where it lies."""
        c = self.corpus
        if c.device is None:
            raise SubgcError("consensus: the corpus is not on a device (ConsensusCorpus(..., device=...) or .to(device))")
        if len(nn_lists) != I:
            raise SubgcError("consensus: one neighbour list per image")
        T = seq.size(1)
        top_k = 0 if top_k is None else int(top_k)
        if top_k < 0:
            raise SubgcError("consensus: top_k >= 1 or None")
        if torch.is_tensor(nn_lists):
            d_nn, max_caps = self.device_neighbours(nn_lists, I, seq.device)
        else:
            nn, max_caps = self.neighbours(nn_lists)
            d_nn = torch.from_numpy(nn).to(seq.device)
        self._score(seq, T, seg, I, max_rows, top_k, d_nn, max_caps, remove_bad_endings, sim, pair_out)
        ops.consensus_rank(sim, seg, I, top_k, order, first)
        return max_caps

    def _score(self, seq, T, seg, I, max_rows, top_k, d_nn, max_caps, remove_bad_endings, sim, pair_out):
        """The method's two launches: cook the candidate rows, score them against the neighbour captions."""
        c = self.corpus
        cand = ops.consensus_cook(seq, c.d_ukeys, c.d_ulogdf, c.ref_len, bad=c.d_bad if remove_bad_endings else None)
        ops.consensus_score(cand, T, seg, I, max_rows, top_k, d_nn, self.k, c.d_cap_off, c.n_img, c.n_caps, c.d_woff, c.cooked, c.d_gauss,
                            self.m, max_caps, sim, pair_out)

    def batch_pass(self, arg, batch, slots):
        """The consensus pass of `eval_collect` (arg: its `consensus=`): fp64 sums | order | first choice in the batch's arena; publishes
        `batch.c_first`, the device int32 [I] first choices, for the accuracy and grounding passes."""
        rows, I = batch.rows, batch.I
        w_sim, w_order, w_first = slots.words(2 * rows, align8=True), slots.words(rows), slots.words(I)
        if ("nn" in arg) == ("index" in arg):
            raise SubgcError("consensus: exactly one of 'nn' (host neighbour lists) and 'index' (an ImageIndex, with 'features') is needed")
        if "nn" in arg:
            def enqueue():
                batch.c_first = slots.arena[w_first]
                if I and rows:
                    self.enqueue(batch.seq_s, batch.seg, I, batch.max_rows, arg["nn"], arg.get("top_k"), arg.get("remove_bad_endings", 0),
                                 slots.arena[w_sim].view(torch.float64), slots.arena[w_order], batch.c_first)

            return enqueue, lambda host: {"c_sim": host[w_sim].view(np.float64).copy(), "c_order": host[w_order].copy(), "c_first": host[w_first].copy()}
        # the search in the same pass: the batch's query rows go up now, `search` writes its int32 lists straight into the batch's arena
        # (so they ride in its one copy) and the score launch reads their first k columns there (nn_ld = k_search)
        index = arg["index"]
        k_search = index.check_k(arg.get("k_search", self.k))
        if k_search < self.k:
            raise SubgcError(f"consensus: k_search = {k_search} is smaller than the re-ranker's k = {self.k}")
        if len(arg["features"]) != I:
            raise SubgcError("consensus: one feature vector per image")
        self.caps_bound()
        w_nn = slots.words(I * k_search)
        d_q = index.queries(np.stack([np.asarray(f).reshape(-1) for f in arg["features"]])) if I else None

        def enqueue():
            batch.c_first = slots.arena[w_first]
            if I:
                d_nn = slots.arena[w_nn].view(I, k_search)
                index.search(d_q, k_search, arg.get("workspace_bytes", WORKSPACE_BYTES), idx=d_nn, want_dist=False)
                if rows:
                    self.enqueue(batch.seq_s, batch.seg, I, batch.max_rows, d_nn, arg.get("top_k"), arg.get("remove_bad_endings", 0),
                                 slots.arena[w_sim].view(torch.float64), slots.arena[w_order], batch.c_first)

        return enqueue, lambda host: {"c_sim": host[w_sim].view(np.float64).copy(), "c_order": host[w_order].copy(), "c_first": host[w_first].copy(),
                                      "c_nn": host[w_nn].reshape(I, k_search)[:, :self.k].copy()}

    def rerank(self, seq, bounds, nn_lists, top_k=None, remove_bad_endings=0, return_pairs=False):
        """seq [rows, T]: the decode batch's device token rows, image i owning rows bounds[i] .. bounds[i+1]-1 in sGPN-ranked order;
        top_k keeps each image's first top_k rows (cr_mRNN_demo.py --top_k; None: all).
        -> (order, sim): per image an int64 array (indices into the image's candidate list, best first; equal sums: lower index first)
        and the fp64 sums of its candidates; with return_pairs also the per-image [candidates, neighbour captions] pair scores."""
        if not seq.is_cuda:
            raise SubgcError("subgc ops need device tensors (the HIP path has no CPU fallback)")
        rows, I = seq.size(0), len(bounds) - 1
        if bounds[-1] != rows:
            raise SubgcError("consensus: bounds do not cover the rows of seq")
        dev = seq.device
        sizes = [b - a for a, b in zip(bounds, bounds[1:])]
        max_rows = max(sizes + [0])
        if rows == 0 or I == 0:
            return [np.zeros(0, np.int64) for _ in range(I)], [np.zeros(0, np.float64) for _ in range(I)]
        seg = ops.upload(list(bounds), torch.int32, dev)
        arena = torch.empty(3 * rows, device=dev, dtype=torch.int32)
        sim, order = arena[:2 * rows].view(torch.float64), arena[2 * rows:]
        pairs = None
        if return_pairs:
            mc = self.caps_bound() if torch.is_tensor(nn_lists) else self.neighbours(nn_lists)[1]
            pairs = torch.empty(rows, max(mc, 1), device=dev, dtype=torch.float64)
        self.enqueue(seq.contiguous(), seg, I, max_rows, nn_lists, top_k, remove_bad_endings, sim, order, None, pairs)
        host = arena.cpu().numpy()                                          # the one copy
        h_sim, h_order = host[:2 * rows].view(np.float64), host[2 * rows:]
        keep = [n if not top_k else min(n, int(top_k)) for n in sizes]
        out_o = [h_order[a:a + n].astype(np.int64) for a, n in zip(bounds, keep)]
        out_s = [h_sim[a:a + n].copy() for a, n in zip(bounds, keep)]
        if return_pairs:
            hp = pairs.cpu().numpy()
            return out_o, out_s, [hp[a:a + n] for a, n in zip(bounds, keep)]
        return out_o, out_s


class BleuConsensusReranker(ConsensusReranker):
    """`consensus_rerank(method='bleu')` for a decode batch: as ConsensusReranker -- same `neighbours`, `enqueue`, `rerank` and returns,
    so it serves as `consensus={"reranker": ...}` of `ops.eval_collect` / `eval_glue.caption_images` -- with the m-RNN sentence-level
    n-gram F-score (bleu_score_util.py:15-61) as the pair score: `subgc_consensus_bleu_cook / _bleu_score` of
    include/subgc_consensus_hip.h.  Defaults k_bleu = 60, m_bleu = 175, bleu_ngram = 4, fpr_bleu = 1.0 (conf_cr.py:45-48).  The corpus
    cooks its n-gram count lists on the first enqueue."""

    def __init__(self, corpus, k=60, m=175, ngram=4, fpr=1.0):
        super().__init__(corpus, k=k, m=m)
        if isinstance(ngram, bool) or int(ngram) != ngram or not 1 <= ngram <= 4:
            raise SubgcError(f"consensus: ngram = {ngram}; n-gram orders 1 .. 4")
        fpr = float(fpr)
        if not np.isfinite(fpr) or fpr < 0.0:
            raise SubgcError(f"consensus: fpr = {fpr}; a finite weight >= 0")
        self.ngram, self.fpr = int(ngram), fpr

    def _score(self, seq, T, seg, I, max_rows, top_k, d_nn, max_caps, remove_bad_endings, sim, pair_out):
        c = self.corpus
        cand = ops.consensus_bleu_cook(seq, bad=c.d_bad if remove_bad_endings else None)
        ops.consensus_bleu_score(cand, T, seg, I, max_rows, top_k, d_nn, self.k, c.d_cap_off, c.n_img, c.n_caps, c.d_woff, c.bleu_cooked(),
                                 self.ngram, self.fpr, self.m, max_caps, sim, pair_out)


def make_reranker(corpus, method="cider", **kw):
    """`consensus_rerank(method=...)` (consensus_reranking.py:122-143): the re-ranker of the method with the reference's defaults
    (conf_cr.py:43-48: cider k = 60, m = 125; bleu k = 60, m = 175, ngram = 4, fpr = 1.0); keywords override them."""
    if method == "cider":
        return ConsensusReranker(corpus, **kw)
    if method == "bleu":
        return BleuConsensusReranker(corpus, **kw)
    raise SubgcError(f"consensus: method = {method!r}; only support cider and bleu currently")      # consensus_reranking.py:123-124


def chunk_entries(arg, h, bounds):
    """`caption_images(consensus=...)`: what every image's entry gains from `eval_collect`'s outputs `h` (None: a batch without rows)."""
    # the search ran in the pass: every entry also carries the first k neighbour indices it used (a batch without rows launches nothing,
    # the search included: its entries carry an empty list)
    searched = "index" in arg
    if h is None:
        return [dict({"consensus_rerank_ind": np.zeros(0, np.int64), "consensus_sim": np.zeros(0, np.float64)},
                     **({"consensus_nn": np.zeros(0, np.int64)} if searched else {})) for _ in bounds[1:]]
    k = arg.get("top_k")
    keep = [(b - a) if not k else min(b - a, int(k)) for a, b in zip(bounds, bounds[1:])]
    out = [{"consensus_rerank_ind": h["c_order"][a:a + n].astype(np.int64), "consensus_sim": h["c_sim"][a:a + n].copy()} for a, n in zip(bounds, keep)]
    if searched:
        for j, e in enumerate(out):
            e["consensus_nn"] = h["c_nn"][j].astype(np.int64)
    return out


def _ngram_counters(ids):
    """Per order 1 .. 4 the dictionary n-gram (id tuple) -> count: `Counter(ngrams(sentence, o))`."""
    out = []
    for o in range(1, 5):
        d = {}
        for p in range(len(ids) - o + 1):
            g = tuple(ids[p:p + o])
            d[g] = d.get(g, 0) + 1
        out.append(d)
    return out


def _bleu_pair(tc, tl, rc, rl, n, fpr):
    if n > tl or n > rl:                                                     # bleu_score_util.py:27: n, not the order at hand
        return 0.0
    total = 0.0
    for o in range(n):
        acc = 0
        small, big = (tc[o], rc[o]) if len(tc[o]) <= len(rc[o]) else (rc[o], tc[o])
        for g, x in small.items():
            y = big.get(g)
            if y is not None:
                acc += min(x, y)
        f = 0.0
        if acc != 0:
            pre = float(acc) / float(tl - o)
            rec = float(acc) / float(rl - o)
            f = ((fpr + 1) * pre * rec) / (rec + fpr * pre)
        total = total + f                                                    # left to right, where the reference calls math.fsum
    return total / float(n)


def bleu_pair_restatement(t_ids, r_ids, n, fpr):
    """The device contract of one pair score (include/subgc_consensus_hip.h), restated with Python floats (IEEE fp64, one rounding per
    operation): calculate_bleu_sentence of bleu_score_util.py:15-61 on word ids, with the plain left-to-right sum of the n F-scores in
    place of math.fsum.  t_ids: the candidate's ids, r_ids: the neighbour caption's."""
    t_ids, r_ids = [int(x) for x in t_ids], [int(x) for x in r_ids]
    return _bleu_pair(_ngram_counters(t_ids), len(t_ids), _ngram_counters(r_ids), len(r_ids), int(n), float(fpr))


def bleu_rerank_restatement(cands, ref_ids, nn, k, m, n, fpr):
    """One image of consensus_reranking.py:152-172 with that pair score: candidates (id lists) against the captions (`ref_ids`: per
    corpus image a list of id lists) of its first k neighbours -> (pair scores [candidates, captions], sums of the m largest added in
    descending order as Python's sum adds the sorted list, the stable descending order of the sums: lower index first among equals)."""
    caps = []
    for j in range(k):
        caps += ref_ids[int(nn[j])]
    rc = [(_ngram_counters(r), len(r)) for r in caps]
    pairs = np.zeros((len(cands), len(caps)))
    sums = np.zeros(len(cands))
    seen = {}
    for a, c in enumerate(cands):
        key = tuple(int(x) for x in c)
        if key not in seen:                                                  # duplicate candidates are scored once
            tc = _ngram_counters(list(key))
            seen[key] = [_bleu_pair(tc, len(key), r, rl, int(n), float(fpr)) for r, rl in rc]
        pairs[a] = seen[key]
        sums[a] = sum(sorted(seen[key], reverse=True)[:m])
    return pairs, sums, np.argsort(-sums, kind="stable")


def save_rerank_ind(path, rerank_ind):
    """Write {image_id: order} in the format of the reference's `consensus_rerank_ind.npy` (consensus_reranking.py:174,179: a pickled
    dict of python lists, read back by misc/grd_utils.py:34 with `np.load(..., allow_pickle=True).tolist()`)."""
    np.save(path, {k: [int(x) for x in v] for k, v in rerank_ind.items()})


def load_rerank_ind(path):
    return np.load(path, allow_pickle=True, encoding="latin1").tolist()
