"""The model-facing part of the reference's evaluation loop (misc/eval_utils.py:98-146, misc/utils.py:59-81,
misc/grd_utils.py:36-58).

What `eval_split` does between the model call and the metric scripts: rank an image's captions by sGPN score,
map the kept sub-graphs back to their original indices, turn token rows into sentences, collect one
`predictions` entry per image and -- for the grounding experiments (`return_att_weight`) -- find for every word of
the chosen caption the graph node with the largest attention weight.  Here the model call is `sample_images`
(many images per decode batch); ranking, reordering and the grounding arg-max are ONE launch each over the whole
batch (`subgc_eval_rank_rows`, `subgc_grounding_argmax`) and everything the host needs arrives in ONE copy per
decode batch (`eval_collect`: a fixed sequence of passes over one int32 upload and one int32 result arena; every optional scorer has a
`batch_pass` beside its own code).  The text side of the grounding protocol (lemma -> detection class, box files:
`grounding_material`) is dictionary look-ups on the host; the COCO / GVD metric scripts are out of scope.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from ._lib import SubgcError, call

# misc/utils.py:16-17
BAD_ENDINGS = ("with", "in", "on", "of", "a", "at", "to", "for", "an", "this", "his", "her", "that", "the")


def decode_sequence(ix_to_word, seq, remove_bad_endings=None):
    """Token rows -> sentences (misc/utils.py:59-81): words up to the first 0; optionally strip dangling
    function words (`REMOVE_BAD_ENDINGS`, set by eval_utils.py:38-39)."""
    if remove_bad_endings is None:
        remove_bad_endings = int(os.getenv("REMOVE_BAD_ENDINGS", "0"))
    rows = seq.detach().cpu().tolist() if torch.is_tensor(seq) else [list(r) for r in seq]
    out = []
    for row in rows:
        words = []
        for ix in row:
            if ix <= 0:
                break
            words.append(ix_to_word[str(int(ix))])
        txt = " ".join(words)
        if remove_bad_endings:
            parts = txt.split(" ")
            cut = 0
            for j in range(len(parts)):
                if parts[-j - 1] not in BAD_ENDINGS:
                    cut = -j
                    break
            txt = " ".join(parts[0:len(parts) + cut])
        out.append(txt)
    return out


# One description per option of `caption_images`, the first four in eval_collect's pass order.  only_sct: defined only in sct mode (else:
# not there); att: needs return_att and the attention buffer; covers: its id-keyed dicts that must hold every image, lacks: what a gap in
# them is called; what + verbs: the subject of its refusals.  A chunk's list-keyed argument is the option with those dicts read at the
# chunk's ids, finished by the scorer module's `chunk_arg` where it says so (per-image draws, prepared boxes); what an image of a row-less
# batch gets and which entry keys are attached is the module's `chunk_entries`.  Controllability is scored per image
# (`_score_controllability`).
_OPTIONS = {
    "consensus": dict(only_sct=False, att=False, covers=("nn",), lacks="consensus['nn'] has no neighbour list", what="consensus re-ranking",
                      verbs=("is", "needs")),
    "diversity": dict(only_sct=False, att=False, covers=(), lacks="", what="diversity scores", verbs=("are", "need"), chunk_arg=True),
    "accuracy": dict(only_sct=False, att=False, covers=("index",), lacks="accuracy['index'] names no reference image", what="accuracy scores",
                     verbs=("are", "need")),
    "grounding": dict(only_sct=False, att=True, covers=("index", "boxes"), lacks="grounding['index'] / ['boxes'] name no reference image or no boxes",
                      what="grounding scores", verbs=("are", "need"), chunk_arg=True),
    "controllability": dict(only_sct=True, att=False, covers=("index",), lacks="controllability['index'] names no first group",
                            what="controllability scores", verbs=("are", "need")),
}
# `consensus=` with an ImageIndex in place of the host lists: the same option, covered by the feature dict instead
_CONSENSUS_SEARCH = dict(_OPTIONS["consensus"], covers=("features",), lacks="consensus['features'] has no feature vector")
_NOT_IN_SCT = "not defined in sct (controllability) mode: its captions keep the input order and are not ranked"
_ONLY_SCT = "defined only in sct (controllability) mode (eval_kwargs['sct'] = 1): they need one caption per input region set, in input order"


def rank_subgraphs(model, seqq, subgraph_score, keep_nms_ind, sct_mode=False):
    """eval_utils.py:105-121 -> (seq, subgraph_score, sorted_subgraph_ind, sort_ind)."""
    if sct_mode:                                                          # controllability: input order, first half only
        valid = subgraph_score.size(0) // 2
        return seqq[:valid], subgraph_score[:valid], keep_nms_ind[:valid], keep_nms_ind[:valid].long()
    if model.gpn:
        sorted_score, sort_ind = ops.rank_desc(subgraph_score.float())
        return seqq[sort_ind.to(seqq.device)], sorted_score, keep_nms_ind[sort_ind], sort_ind
    sort_ind = torch.arange(subgraph_score.size(0), device=keep_nms_ind.device).type_as(keep_nms_ind)
    return seqq, subgraph_score, keep_nms_ind, sort_ind


class Slots:
    """Two-phase reservation for `eval_collect`: `ints` / `words` hand out slices while the passes are set up; then `seg` is the single upload
    of `values` and `arena` the single int32 result tensor of `n_words` they index; the same slices index the arena's one host copy."""

    def __init__(self, values):
        self.values, self.n_words = values, 0

    def ints(self, values):
        a = len(self.values)
        self.values += values
        return slice(a, len(self.values))

    def words(self, n, align8=False):
        a = (self.n_words + 1) & ~1 if align8 else self.n_words        # an fp64 slot starts 8-byte aligned
        self.n_words = a + n
        return slice(a, self.n_words)


def eval_collect(score, keep, seq, bounds, identity=False, AL=None, idx=None, pick=None, consensus=None, diversity=None, accuracy=None,
                 grounding=None):
    """The eval loop's per-image work for a whole decode batch (misc/eval_utils.py:105-121; grounding: misc/grd_utils.py:36-47):
    one ranking launch (subgc_eval_rank_rows), one grounding launch when `AL` (the decode loop's attention buffer [T1, rows, N]) and
    `idx` (the kept sub-graphs' node lists [rows, N]) are given, and ONE device -> host copy of everything.
    score [rows] fp32, keep [rows] int64, seq [rows, T] int64, bounds: python list of the I + 1 row boundaries of the images,
    pick: optional per-image subg_index list (default 0 = the best-ranked caption).
    consensus: optional {"reranker": ConsensusReranker, "nn": per-image neighbour index lists, "top_k": int or None, "remove_bad_endings": 0 / 1}
    (or, in place of "nn", "index": a neighbours.ImageIndex and "features": per-image feature vectors -> the search runs first, + c_nn):
    the ranked token rows are re-ranked on the device in the same pass (subgc_consensus_cook / _score / _rank) and, unless `pick` is
    given, the grounding launch takes each image's pick from the re-ranker's first choice ON THE DEVICE; its outputs ride in the same copy.
    -> dict of host numpy arrays: order / score / keep (int64) / seq (int64) [rows...], and with grounding att2 / node [I, T1], n_words [I];
    with consensus c_order (int32 [rows]: image i's order in its first n_i' = min(n_i, top_k) slots), c_sim (fp64 [rows]), c_first [I].
    diversity: optional {"scorer": DiversityScorer, "plan": its `plan(draws, sizes)`, "remove_bad_endings": 0 / 1}: the ranked rows and scores
    are scored on the device in the same pass (subgc_diversity_select / _distinct / _best) -> d_int (int32 [sets, DIV_COLS + n_best]) and
    d_f64 (fp64 [sets, n_best + 1]) in the same copy; `scorer.unpack(plan, d_int, d_f64)` makes the per-image entries.
    accuracy: optional {"scorer": AccuracyScorer, "index": per-image reference-image indices, "remove_bad_endings": 0 / 1}: the ranked rows
    are scored against their references on the device in the same pass (subgc_consensus_cook, subgc_accuracy_rows / _oracle of
    subgc_metrics_hip.h); the top-1 row is the re-ranker's first choice, read from device memory, when `consensus` is given, row 0
    otherwise -> a_words (int32: the scorer's result arena) in the same copy; `scorer.unpack(a_words, bounds)` makes the per-image entries.
    With accuracy=None the arena, the launches and the outputs are what they are without it.
    grounding: optional {"scorer": GroundingScorer, "index": per-image reference-image indices, "boxes": per image its fp32 boxes [N_i, 4]
    in image scale (`grounding.prepare_boxes`), "remove_bad_endings": 0 / 1}; needs AL / idx.  Behind the grounding arg-max the chosen
    captions become {'clss','idx_in_sent','bbox'} lists and precision / recall event codes on the device (subgc_grounding_material /
    _score of subgc_grounding_hip.h); the boxes go up with the batch -> g_words (int32: the scorer's result arena) in the same copy and
    g_plan; `scorer.unpack(g_words, g_plan)` makes the per-image entries.  With grounding=None nothing changes."""
    P, stream, dev = ops._ptr, ops._stream(), score.device
    rows, T = seq.shape
    I = len(bounds) - 1
    if bounds[-1] != rows or score.numel() != rows or keep.numel() != rows:
        raise SubgcError("eval_collect: bounds / score / keep do not cover the rows of seq")
    ground = AL is not None
    T1 = AL.size(0) if ground else 0
    # what the passes read: the batch's sizes now, `seg` / `seq_s` / `score_s` (the upload and the ranked rows) once they exist, and what
    # earlier passes publish: `c_first`, then `pick` / `node` / `n_words` of the grounding arg-max
    b = SimpleNamespace(I=I, rows=rows, T=T, T1=T1, bounds=bounds, ground=ground, max_rows=max([y - x for x, y in zip(bounds, bounds[1:])] + [0]),
                        c_first=None)
    slots = Slots(list(bounds))                                         # the bounds lead the upload: the kernels' `seg`
    s_pick = slots.ints([0] * I if pick is None else [int(p) for p in pick])
    w_order, w_score, w_keep, w_seq = slots.words(rows), slots.words(rows), slots.words(rows), slots.words(rows * T)
    if ground:
        w_att2, w_node, w_nw = slots.words(I * T1), slots.words(I * T1), slots.words(I)
    # the passes, in launch order: each validates and reserves now, launches and reads back below
    passes = [(name, *arg["reranker" if name == "consensus" else "scorer"].batch_pass(arg, b, slots))
              for name, arg in (("consensus", consensus), ("diversity", diversity), ("accuracy", accuracy), ("grounding", grounding))
              if arg is not None]
    b.seg = slots.seg = ops.upload(slots.values, torch.int32, dev)
    arena = slots.arena = torch.empty(max(slots.n_words, 1), device=dev, dtype=torch.int32)
    order, keep_s = arena[w_order], arena[w_keep]
    b.score_s, b.seq_s = arena[w_score].view(torch.float32), arena[w_seq].view(rows, T)
    # the rows as both launches read them, held until the last is enqueued; a batch without rows has no storage, and the arg-max, which
    # then reads none, refuses a null pointer
    seq_c = seq.contiguous()
    p_seq = P(seq_c, torch.int64) if rows else arena.data_ptr()
    if I and rows:
        call("subgc_eval_rank_rows", P(score.contiguous(), torch.float32), P(keep.contiguous(), torch.int64), p_seq,
             T, P(b.seg), I, b.max_rows, int(bool(identity)), P(order), P(b.score_s), P(keep_s), P(b.seq_s), stream)
    for name, enqueue, _ in passes:
        if name != "grounding":
            enqueue()
    if ground:
        att2, b.node, b.n_words = arena[w_att2], arena[w_node], arena[w_nw]
        if AL.stride(2) != 1 or idx.stride(1) != 1:
            raise SubgcError("eval_collect: AL / idx need unit inner strides")
        if I:
            # the caption the entry describes: an explicit pick, else the re-ranker's first choice, else 0
            b.pick = b.seg[s_pick] if pick is not None else (b.c_first if (b.c_first is not None and rows) else None)
            call("subgc_grounding_argmax", P(AL, torch.float32), AL.stride(0), AL.stride(1), AL.size(2), T1, p_seq, T,
                 P(idx, torch.int64), idx.stride(0), P(b.seg), P(order) if (rows and not identity) else None, P(b.pick), I, P(att2),
                 P(b.node), P(b.n_words), stream)
    for name, enqueue, _ in passes:
        if name == "grounding":
            enqueue()
    host = arena.cpu().numpy()                                          # the one copy (synchronises the stream)
    out = {"order": host[w_order].astype(np.int64), "score": host[w_score].view(np.float32).copy(), "keep": host[w_keep].astype(np.int64),
           "seq": host[w_seq].reshape(rows, T).astype(np.int64)}
    if ground:
        out.update(att2=host[w_att2].reshape(I, T1).copy(), node=host[w_node].reshape(I, T1).copy(), n_words=host[w_nw].copy())
    for _, _, results in passes:
        out.update(results(host))
    return out


@torch.no_grad()
def caption_images(model, images, infos, ix_to_word, eval_kwargs=None, group=256, shard=False, grd_pick=None, consensus=None, diversity=None, accuracy=None,
                   grounding=None, controllability=None):
    """The testing branch of eval_split for a list of loader items: returns the `predictions` list
    (eval_utils.py:132-141): {'image_id', 'caption': [...], 'subgraph_score', 'sorted_subgraph_ind'} per image.

    Single-process by default, like the reference's eval (one process, eval_utils.py:98-104): safe to call on rank 0 only
    while the other ranks of a data-parallel job wait elsewhere.
    `shard=True` makes the call COLLECTIVE: EVERY rank of the default process group must call it with the SAME
    `images` / `infos` lists; images go round-robin across the ranks, every rank captions its share, the predictions are
    gathered once at the end and every rank returns the full list.  The image ids are exchanged first and a mismatch (a caller
    that already split its list per rank, or ranks evaluating different splits) raises on every rank instead of merging
    results of different lists by index.

    `eval_kwargs["return_att"] = 1` (the grounding experiments, eval_utils.py:98-101,143-146): every entry also gets
    `"grounding"`: {'subg_index', 'sort_ind', 'att2_ind', 'node_ind'} -- for the caption ranked `subg_index` (0 = best by sGPN score;
    `grd_pick[i]` = the consensus re-ranker's choice for image i, grd_utils.py:31-35) the arg-max attention column of every word
    position and the full-graph node id (= box row) it stands for (grd_utils.py:36-47; `grounding_material` finishes the entry).
    With `beam_size > 1` (which the reference refuses for grounding, eval_utils.py:45) the entry describes the BEAM caption: the decode
    hands over the attention of every row's winning beam (sampling.decode; subgc_beam_att_hip.h) in the same [T + 1, rows, N] layout,
    so `grounding=`, `consensus=`, `accuracy=`, `diversity=`, `group_size > 1` and `shard=True` work as they do for a greedy decode.

    `consensus={"reranker": ConsensusReranker, "nn": {image_id: [nearest training-image indices]}, "top_k": 4}` (default None: off)
    re-ranks every image's sGPN-sorted captions -- its best `top_k`, None = all -- by CIDEr consensus (or, with a
    `BleuConsensusReranker`, by the m-RNN sentence BLEU: `consensus.make_reranker(corpus, method)`) on the device, in the decode
    batch's own pass (subgc.consensus; cr_mRNN_demo.py -> consensus_rerank).  Every entry gains `"consensus_rerank_ind"` (indices into
    its `caption` list, best first, equal sums in ascending index: what the reference's consensus_rerank_ind.npy holds) and
    `"consensus_sim"` (the fp64 sums of those captions).  With `return_att` the grounding entry is the re-ranker's FIRST choice, picked on
    the device in the same pass -- no second evaluation run; an explicit `grd_pick` still wins.  `remove_bad_endings` trims the
    candidates exactly as it trims the strings.  Not available in `sct` mode.
    `consensus={"reranker": ..., "index": neighbours.ImageIndex, "features": {image_id: [D] feature vector}, "top_k": 4}` takes the place of
    `"nn"` (exactly one of the two): the nearest-image search (`find_NNimg`) runs on the decode stream ahead of the consensus launches --
    the batch's query rows go up with the batch, the re-ranker reads the device lists where they lie, there is no host list -- and every
    entry additionally gains `"consensus_nn"`: the first `reranker.k` neighbour indices of its image, from the batch's one copy.
    Optional `"k_search"` (default `reranker.k`, at most 1024) and `"workspace_bytes"` as in `ImageIndex.search`.

    `diversity={"scorer": DiversityScorer, "top_n": (20, 100), "seed": 2019}` (default None: off) scores every image's captions the way
    misc/diversity/diversity_score.py does -- distinct captions of a random draw, n-gram diversity, novel captions and mBLEU-4 of the
    draw's best five by sGPN score -- on the device, in the decode batch's own pass and its one copy (subgc.diversity).  Every entry gains
    `"diversity"`: plain integer counts and fp64 values with one entry per `top_n` (`DiversityScorer.unpack`); `diversity.summarize` of
    those entries gives the numbers the script prints.  The draws come from `per_image_draws`, keyed by the image id, so `group`, the
    order of the list and `shard=True` cannot change an image's result (the script's own stream runs over the whole file;
    `diversity.score_predictions` reproduces that one).  Works together with `consensus=`; not available in `sct` mode.

    `accuracy={"scorer": AccuracyScorer, "index": {image_id: index of the image in the scorer's references}}` (default None: off) scores
    every caption against the image's reference captions the way `test.py --only_sent_eval 1 --oracle_num N` does (sentence BLEU-1..4
    with their material, CIDEr, ROUGE-L; the oracle picks over the first `oracle_num` captions) on the device, in the decode batch's own
    pass and its one copy (subgc.accuracy).  Every entry gains `"accuracy"` (`AccuracyScorer.unpack`); `accuracy.summarize` of those
    entries gives the corpus numbers, so they accumulate across batches and ranks.  The top-1 caption is caption 0, or with `consensus=`
    the re-ranker's first choice, taken on the device.  Works together with `consensus=` and `diversity=`; not available in `sct` mode.

    `grounding={"scorer": GroundingScorer, "index": {image_id: index of the image in the scorer's references}, "boxes": {image_id: the
    detector's boxes [N, 4]}, "img_wh": {image_id: (w, h)} or None}` (default None: off; needs `return_att`) finishes the grounding
    experiment on the device, in the decode batch's own pass and its one copy (subgc.grounding): the sentence `"grounding"` describes --
    `grd_pick`, else the re-ranker's first choice with `consensus=`, else caption 0 -- becomes the {'clss','idx_in_sent','bbox'} list of
    misc/grd_utils.py:49-60 and is scored against the image's annotated captions the way misc/grounding/grounding_score.py does.  The
    boxes are prepared as grd_utils.py:27 and the JSON round trip leave them (`boxes * max(w, h) / 592` in the array's own dtype, rounded
    once to fp32; `img_wh` None: used as given) and go up with the batch.  Every entry gains `"grounding_score"`
    (`GroundingScorer.unpack`: the list and the precision / recall event codes); `grounding.summarize` of those entries gives F1_all /
    F1_loc and their parts, so they accumulate across batches and ranks.  `"grounding"` itself gains and loses nothing.  Not available in
    `sct` mode.

    `controllability={"scorer": ControlScorer, "index": {image_id: index of the image's first group in the scorer's references}}` (default
    None: off; available ONLY in `sct` mode) scores the set-controllability run the way misc/controllability/controllability_score.py
    does (subgc.controllability): an image's kept rows (the first half, in input order) are the generated captions of its consecutive
    groups, index .. index + rows - 1.  The decode stays per image; the kept rows of a chunk are scored together in one
    `ControlScorer.score` call -- the Noun IoU launch, the accuracy launches, one host copy -- and every entry gains `"controllability"`: the
    per-row entries of its rows (Noun IoU with its pairs and assignments, BLEU material, CIDEr, ROUGE-L against the row's group);
    `controllability.summarize` of those entries, flattened in `order_list` order, gives the script's numbers.  `index` holds the first
    group of EVERY image of the references: an image's number of groups is the distance to the next first group (the last image's: to
    the number of groups), and an image whose kept rows differ from it in number is an error that names the image id.

    Decode rules (subgc.decode_rules; greedy / sampling decode only, `beam_size > 1` with one of the first three raises):
    `eval_kwargs["block_trigrams"]` (with `"trigram_alpha"`, default 2.0), `["block_bad_endings"]` (the ids of BAD_ENDINGS are taken from
    `ix_to_word` unless `["bad_ending_ids"]` gives them), `["suppress_unk"]` and `["decoding_constraint"]` shape the captions in the token
    loop.  With a rule active every entry gains `"rule_stats"`: int32 [captions, 4], per caption (in the entry's caption order) the steps
    on which a trigram penalty / the repeat ban / the bad-ending ban was applied and on which the first arg-max moved
    (`decode_rules.STAT_NAMES`).  `remove_bad_endings` is untouched by them: it trims the finished strings.
    Under beam search the two rules that have a beam meaning come in through `eval_kwargs["beam_rules"]`, a dict with the keys
    `block_trigrams`, `trigram_alpha`, `block_bad_endings` and `bad_ending_ids` (filled from `ix_to_word` the same way;
    `DecodeRules.from_beam_options`): every state row is ruled before the top-k reads it, and `"rule_stats"` holds
    `decode_rules.sequence_events` of every caption's winning beam (columns 1 and 3 are 0 and -1 there)."""
    import torch.distributed as dist
    from . import parallel
    eval_kwargs = dict(eval_kwargs or {})
    if eval_kwargs.get("block_bad_endings", 0) and eval_kwargs.get("bad_ending_ids") is None:
        from .decode_rules import bad_ending_ids
        eval_kwargs["bad_ending_ids"] = bad_ending_ids(ix_to_word)
    br = eval_kwargs.get("beam_rules")
    if isinstance(br, dict) and br.get("block_bad_endings", 0) and br.get("bad_ending_ids") is None:
        from .decode_rules import bad_ending_ids
        eval_kwargs["beam_rules"] = dict(br, bad_ending_ids=bad_ending_ids(ix_to_word))
    world = dist.get_world_size() if dist.is_initialized() else 1
    if shard and world > 1:
        ids = [info["id"] for info in infos]
        if len(ids) != len(images):
            raise ValueError("caption_images: one `infos` entry per image")
        seen = [None] * world
        dist.all_gather_object(seen, ids)
        if any(s != ids for s in seen):
            raise ValueError("caption_images(shard=True) is collective: every rank must pass the same image list "
                             f"(rank {dist.get_rank()} has {len(ids)} images, the ranks hold {[len(s) for s in seen]})")
        mine, idx = parallel.shard_images(images, dist.get_rank(), world)
        local = caption_images(model, mine, [infos[i] for i in idx], ix_to_word, eval_kwargs, group, shard=False,
                               grd_pick=None if grd_pick is None else [grd_pick[i] for i in idx], consensus=consensus, diversity=diversity, accuracy=accuracy,
                               grounding=grounding, controllability=controllability)
        return parallel.gather_by_index(local, idx, len(images))
    from . import accuracy as accuracy_m, consensus as consensus_m, diversity as diversity_m, grounding as grounding_m
    sct_mode = eval_kwargs.get("sct", 0) == 1
    rbe = eval_kwargs.get("remove_bad_endings", 0)
    return_att = eval_kwargs.get("return_att", 0) == 1
    if grd_pick is not None and len(grd_pick) != len(images):
        raise ValueError("caption_images: one grd_pick entry per image")
    given = {"consensus": consensus, "diversity": diversity, "accuracy": accuracy, "grounding": grounding, "controllability": controllability}
    mods = {"consensus": consensus_m, "diversity": diversity_m, "accuracy": accuracy_m, "grounding": grounding_m}
    if consensus is not None and ("nn" in consensus) == ("index" in consensus):
        raise ValueError("caption_images: consensus re-ranking needs exactly one of consensus['nn'] (host neighbour lists) and "
                         "consensus['index'] (a neighbours.ImageIndex, with consensus['features'])")
    live = [(name, _CONSENSUS_SEARCH if name == "consensus" and "index" in given[name] else d, given[name])
            for name, d in _OPTIONS.items() if given[name] is not None]
    for name, d, opt in live:
        if sct_mode != d["only_sct"]:
            raise ValueError(f"caption_images: {d['what']} {d['verbs'][0]} " + (_ONLY_SCT if d["only_sct"] else _NOT_IN_SCT))
        if d["att"] and not return_att:
            raise ValueError(f"caption_images: {d['what']} {d['verbs'][1]} eval_kwargs['return_att'] = 1 (the attention arg-max of every word)")
        missing = [info["id"] for info in infos if any(info["id"] not in opt[k] for k in d["covers"])]
        if missing:
            raise ValueError(f"caption_images: {d['lacks']} for image ids {missing[:5]}")
    batch_opts = [(name, d, opt, mods[name]) for name, d, opt in live if name in mods]      # those that ride in the decode batch's pass
    if controllability is not None:
        c_scorer = controllability["scorer"]
        firsts = sorted(set(int(v) for v in controllability["index"].values())) + [c_scorer.refs.n_groups]
        c_count = {a: b - a for a, b in zip(firsts, firsts[1:])}
    was_training = model.training
    model.eval()
    predictions = []
    # a decode batch holds up to group x gpn_max_subg sub-graph rows (x beam): keep it near 8 k rows -- 256 images at the
    # Karpathy setting (10 sub-graphs), 8 at the MRNN setting (up to 1000), where one image already fills the chip
    group = max(1, min(group, 8192 // max(1, int(getattr(model, "gpn_max_subg", 1)) * max(1, int(eval_kwargs.get("beam_size", 1))))))
    try:
        for i in range(0, len(images), group):
            chunk, chunk_infos = images[i:i + group], infos[i:i + group]
            hold = {"skip_att": True}
            results = model.sample_images(chunk, opt=eval_kwargs) if sct_mode else _sample_batch(model, chunk, eval_kwargs, hold)
            for _, d, _, _ in batch_opts:
                if "bounds" not in hold or (d["att"] and hold.get("AL") is None):
                    raise ValueError(f"caption_images: {d['what']} {d['verbs'][1]} a model whose sample_images exposes the decode batch"
                                     f"{' and its attention buffer' if d['att'] else ''} (batch_out)")
            if "bounds" not in hold:
                # per image: controllability mode (input order, first half, no ranking; rare) and models whose sample_images does not
                # expose the batch tensors
                kept = []
                for info, r in zip(chunk_infos, results):
                    seq, score, sorted_ind, _ = rank_subgraphs(model, r[0], r[2], r[3], sct_mode)
                    predictions.append({"image_id": info["id"], "caption": decode_sequence(ix_to_word, seq, rbe),
                                        "subgraph_score": score.cpu().numpy(), "sorted_subgraph_ind": sorted_ind.cpu().numpy()})
                    kept.append(seq)
                if controllability is not None:
                    _score_controllability(c_scorer, controllability["index"], c_count, chunk_infos, kept, predictions[len(predictions) - len(kept):], rbe)
                continue
            bounds = hold["bounds"]
            ids, sizes = [info["id"] for info in chunk_infos], [b - a for a, b in zip(bounds, bounds[1:])]
            args = {}
            for name, d, opt, mod in batch_opts:                        # id-keyed dicts -> the chunk's lists; then what only the scorer knows
                args[name] = dict(opt, remove_bad_endings=rbe, **{k: [opt[k][x] for x in ids] for k in d["covers"]})
                if d.get("chunk_arg"):
                    args[name] = mod.chunk_arg(args[name], opt, ids, sizes)
            if hold["rows"] == 0:
                gained = [mod.chunk_entries(args[name], None, bounds) for name, _, _, mod in batch_opts]
                for j, k in enumerate(ids):
                    predictions.append({"image_id": k, "caption": [], "subgraph_score": np.zeros(0, np.float32),
                                        "sorted_subgraph_ind": np.zeros(0, np.int64)})
                    for per_image in gained:
                        predictions[-1].update(per_image[j])
                continue
            ground = return_att and hold.get("AL") is not None
            pick = None if grd_pick is None else grd_pick[i:i + group]
            # eval_utils.py:105-115 for every image of the batch + grd_utils.py:36-47: two launches, one host copy
            h = eval_collect(hold["score"], hold["keep"], hold["seq"], bounds, identity=not model.gpn,
                             AL=hold["AL"] if ground else None, idx=hold["idx"] if ground else None, pick=pick if ground else None, **args)
            gained = [mod.chunk_entries(args[name], h, bounds) for name, _, _, mod in batch_opts]
            rule_stats = hold["rule_stats"].cpu().numpy() if hold.get("rule_stats") is not None else None
            for j, (k, a, b) in enumerate(zip(ids, bounds, bounds[1:])):
                entry = {"image_id": k, "caption": decode_sequence(ix_to_word, h["seq"][a:b], rbe),
                         "subgraph_score": h["score"][a:b], "sorted_subgraph_ind": h["keep"][a:b]}
                if ground:
                    w = int(h["n_words"][j])
                    sub = int(pick[j]) if pick is not None else (int(h["c_first"][j]) if consensus is not None else 0)
                    entry["grounding"] = {"subg_index": sub, "sort_ind": h["order"][a:b],
                                          "att2_ind": h["att2"][j, :w].astype(np.int64), "node_ind": h["node"][j, :w].astype(np.int64)}
                if rule_stats is not None:                              # the decode rows' counters, in the entry's caption order
                    entry["rule_stats"] = rule_stats[a:b][h["order"][a:b]]
                for per_image in gained:
                    entry.update(per_image[j])
                predictions.append(entry)
    finally:
        model.train(was_training)
    return predictions


def _score_controllability(scorer, index, count, infos, kept, entries, rbe):
    """The kept rows of a chunk of `sct` images (one [rows_i, T_i] tensor each) -> one `ControlScorer.score` call; entry i gains
    `"controllability"`: the per-row entries of its rows."""
    groups = []
    for info, seq in zip(infos, kept):
        first = int(index[info["id"]])
        if seq.size(0) != count.get(first, -1):
            raise ValueError(f"caption_images: image {info['id']!r} has {seq.size(0)} kept rows and {count.get(first, 0)} ground-truth groups "
                             f"(first group {first}); controllability scores need one caption per region set")
        groups += list(range(first, first + seq.size(0)))
    T = max(int(seq.size(1)) for seq in kept)
    rows = torch.cat([seq if seq.size(1) == T else torch.nn.functional.pad(seq, (0, T - seq.size(1))) for seq in kept])
    scored = scorer.score(rows, groups, remove_bad_endings=rbe) if groups else []
    a = 0
    for e, seq in zip(entries, kept):
        e["controllability"] = scored[a:a + seq.size(0)]
        a += seq.size(0)


def _sample_batch(model, chunk, eval_kwargs, hold):
    try:
        return model.sample_images(chunk, opt=eval_kwargs, batch_out=hold)
    except TypeError as e:                                              # a stand-in model without the batch view (tests)
        if "batch_out" not in str(e):
            raise
        hold.clear()
        return model.sample_images(chunk, opt=eval_kwargs)


def control_images(model, raw, region_sets, set_off, img_wh, infos, ix_to_word, eval_kwargs=None, controllability=None, obj_num=None, rel_num=None,
                   mode="greedy", gt=None, group=256):
    """Controlled captioning from region boxes in one device pass: `control_input.assemble_sct_batch` (what the reference's
    `dataloaders/dataloader_test_sct.py` `__getitem__` does per image on the host) and then the unchanged `caption_images` in `sct` mode on the
    assembled items -- one caption per region set, in input order, scored with `controllability=` as `caption_images` describes.
    raw / region_sets / set_off / img_wh / mode / gt: see `assemble_sct_batch`; obj_num / rel_num default to raw's own sizes (objects + 1
    dummy node, 65 relation rows).  `eval_kwargs["sct"]` is set to 1.  Every entry additionally carries `"match"`: {'idx' [sets, R] int32,
    'iou' [sets, R] fp32}, per region of each of the image's sets the matched detection box (-1: none) and its IoU."""
    from .control_input import assemble_sct_batch
    obj_num = int(raw["object_fmap"].size(1)) + 1 if obj_num is None else obj_num
    rel_num = 65 if rel_num is None else rel_num
    if len(infos) != raw["object_fmap"].size(0):
        raise ValueError("control_images: one `infos` entry per image")
    if not getattr(model, "sct", False):
        raise ValueError("control_images: the model must be built with sct = 1 (every candidate sub-graph is decoded, no NMS)")
    items, table = assemble_sct_batch(dict(raw, image_ids=[info["id"] for info in infos]), region_sets, set_off, img_wh, obj_num, rel_num, mode=mode, gt=gt)
    preds = caption_images(model, items, infos, ix_to_word, dict(eval_kwargs or {}, sct=1), group=group, controllability=controllability)
    seg = [int(v) for v in (set_off.tolist() if hasattr(set_off, "tolist") else set_off)]
    for p, a, b in zip(preds, seg, seg[1:]):
        p["match"] = {"idx": table["idx"][a:b], "iou": table["iou"][a:b]}
    return preds


def proposal_key(image_id):
    """The sampler key of an image id: a non-negative integer id below 2^43 is its own key; any other id (a file name, say) is keyed by the
    CRC-32 of its `str`.  A function of the id alone, so `group`, the order of the list and the rank cannot change an image's draw."""
    if isinstance(image_id, (int, np.integer)) and not isinstance(image_id, bool) and 0 <= int(image_id) < 1 << 43:
        return int(image_id)
    import zlib
    return zlib.crc32(str(image_id).encode("utf-8"))


def caption_scene_graphs(model, raw, infos, ix_to_word, proposals, eval_kwargs=None, **scorers):
    """Captions from raw scene graphs in one device pass, without the reference's sub-graph files: `proposals` (a
    `subgc.proposals.ProposalSampler`) draws every image's candidate sub-graphs from `raw` (see `ProposalSampler.sample`; the key of an
    image is `proposal_key` of its id) and the unchanged `caption_images` runs on the sampler's items -- sGPN scores, NMS, the decode
    and every scorer.  `scorers`: `caption_images`' own keywords (group, shard, grd_pick, consensus, diversity, accuracy, grounding),
    passed through untouched, as are decode rules and beam search in `eval_kwargs`; with `shard=True` every rank draws the same
    candidates (the draw is cheap and keyed by the image) and captions its share.  Every entry gains `"proposal"`: {'seed_mask',
    'node_mask'} (uint64 each), the seed nodes and the final nodes of its captions' sub-graphs in the entry's caption order -- what
    misc/grd_utils.py:41-42 reads from the mask file.  A model built with sct = 1 is refused: region sets are `control_images`' job."""
    if getattr(model, "sct", False) or dict(eval_kwargs or {}).get("sct", 0) == 1:
        raise ValueError("caption_scene_graphs: sampled candidates are ranked and pruned by the sGPN; a model or a call with sct = 1 decodes "
                         "caller-given region sets (control_images)")
    if len(infos) != raw["object_fmap"].size(0):
        raise ValueError("caption_scene_graphs: one `infos` entry per image")
    drawn = proposals.sample(raw, keys=[proposal_key(info["id"]) for info in infos])
    preds = caption_images(model, drawn.items, infos, ix_to_word, eval_kwargs, **scorers)
    t = drawn.table
    for p, a in zip(preds, t["off"]):
        rows = int(a) + np.asarray(p["sorted_subgraph_ind"], np.int64)
        p["proposal"] = {"seed_mask": t["seed_mask"][rows], "node_mask": t["node_mask"][rows]}
    return preds


def grounding_material(entry, boxes, wd_to_lemma, lemma_det_id_dict, det_id_to_det_wd, img_wh=None):
    """misc/grd_utils.py:36-58 for one `predictions` entry of `caption_images(..., return_att=1)`: the sentence ranked
    `entry["grounding"]["subg_index"]`, its words -> lemma -> detection class; for every word that names one, the box of the node
    that word attended to most.  `boxes` [N_nodes, 4]: the scene-graph detector's boxes of the image (`img_wh` = (w, h): rescaled by
    max(w, h) / 592 like :27-28; None: used as given).  -> {'clss', 'idx_in_sent', 'bbox'} (what the reference appends to
    grd_output[image_id]).  Words are taken from the sentence (after remove_bad_endings, if that was on): arg-max positions beyond
    the sentence are simply not used, like the `[:len(grd_wd)]` slice."""
    g = entry["grounding"]
    boxes = np.asarray(boxes)
    if img_wh is not None:
        boxes = boxes * max(img_wh) / 592
    words = entry["caption"][g["subg_index"]].split()
    out = {"clss": [], "idx_in_sent": [], "bbox": []}
    for j, wd in enumerate(words[:len(g["node_ind"])]):
        if wd not in wd_to_lemma:
            continue
        lemma = wd_to_lemma[wd]
        if lemma in lemma_det_id_dict:
            out["bbox"].append(boxes[int(g["node_ind"][j])].tolist())
            out["clss"].append(det_id_to_det_wd[lemma_det_id_dict[lemma]])
            out["idx_in_sent"].append(j)
    return out


@torch.no_grad()
def ground_gt_images(model, images, infos, gt, group=64):
    """Grounding on GROUND-TRUTH sentences (misc/grounding/eval_grd_flickr30k_entities.py:63-109, the evaluator's `--eval_mode GT`) for a
    list of loader items: every reference caption of an image is decoded teacher-forced on the sub-graph the caller pairs it with --
    candidate j of the image carries caption j (the loaders' entries 0-4 are the sentences' own sub-graphs; a Full-GC model repeats the
    full graph) -- and the word at every annotated `process_idx` is grounded to the node it attended to most.
    gt = {"scorer": GtGroundingScorer, "index": {image_id: index of the image in the scorer's references}, "rows": GtCaptionRows or
    {image_id: int token rows [captions, Tf]}, "boxes": {image_id: the detector's boxes [N, 4]}, "img_wh": {image_id: (w, h)} or None
    (boxes used as given; else rescaled like grd_utils.py:27)}.
    Per batch of `group` images: one forced decode (subgc.forced), `subgc_grounding_argmax` with one row per "image",
    `subgc_gt_grounding_material`, `subgc_gt_grounding_score`, and ONE host copy.  -> one entry per image: {"image_id", "gt_grounding":
    `GtGroundingScorer.unpack`'s entry (the {'idx_in_sent','bbox'} list of every caption and one event code per annotated object),
    "caption_ll": {"ll" fp64, "n_tok" int32, "perplexity" fp64} per caption}; `grounding_gt.summarize` of the "gt_grounding" entries gives
    grd_accu, `grounding_gt.to_submission` the dict the reference evaluator reads.  Not sharded."""
    from . import forced
    from .grounding import prepare_boxes
    scorer, wh = gt["scorer"], gt.get("img_wh")
    if len(infos) != len(images):
        raise ValueError("ground_gt_images: one `infos` entry per image")
    missing = [info["id"] for info in infos if info["id"] not in gt["index"] or info["id"] not in gt["boxes"]]
    if missing:
        raise ValueError(f"ground_gt_images: gt['index'] / ['boxes'] name no reference image or no boxes for image ids {missing[:5]}")
    scorer._need_device()
    out = []
    for i0 in range(0, len(images), max(1, int(group))):
        chunk, ids = images[i0:i0 + group], [info["id"] for info in infos[i0:i0 + group]]
        tokens = [np.asarray(gt["rows"][k]) for k in ids]
        plan = scorer.plan([gt["index"][k] for k in ids], [len(t) for t in tokens])
        boxes = [prepare_boxes(gt["boxes"][k], None if wh is None else wh[k]) for k in ids]
        hold = forced.forced_decode(model, chunk, tokens, return_att=True)
        rows, I = hold["rows"], len(chunk)
        if rows == 0:
            for k, e in zip(ids, scorer.unpack(np.zeros(scorer.arena_words(plan), np.int32), plan)):
                out.append({"image_id": k, "gt_grounding": e, "caption_ll": {"ll": np.zeros(0), "n_tok": np.zeros(0, np.int32), "perplexity": np.zeros(0)}})
            continue
        Tf, dev, bounds = hold["Tf"], hold["seq"].device, hold["bounds"]
        n_box = sum(len(b) for b in boxes)
        row_img = np.repeat(np.arange(I), np.diff(bounds))
        box_off = np.concatenate([[0], np.cumsum([len(b) for b in boxes])])
        n_t = len(plan["table"])
        tables = ops.upload(np.concatenate([plan["table"], row_img, box_off, np.arange(rows + 1)]).astype(np.int32), torch.int32, dev)
        seg = tables[n_t + rows + I + 1:]
        d_box = ops.upload(np.concatenate(boxes).ravel() if n_box else np.zeros(4, np.float32), torch.float32, dev)
        # one int32 arena: ll (fp64) | n_tok | att2 | node | n_words | the scorer's lists and codes
        g_words = scorer.arena_words(plan)
        arena = torch.empty(3 * rows + 2 * rows * Tf + rows + g_words, device=dev, dtype=torch.int32)
        o = 2 * rows
        ll = arena[:o].view(torch.float64)
        n_tok = arena[o:o + rows]; o += rows
        att2 = arena[o:o + rows * Tf]; o += rows * Tf
        node = arena[o:o + rows * Tf]; o += rows * Tf
        nw = arena[o:o + rows]; o += rows
        ops.copy_(ll, hold["ll"]); ops.copy_(n_tok, hold["n_tok"])
        AL, idx = hold["AL"], hold["idx"]
        if AL.stride(2) != 1 or idx.stride(1) != 1:
            raise SubgcError("ground_gt_images: AL / idx need unit inner strides")
        call("subgc_grounding_argmax", ops._ptr(AL, torch.float32), AL.stride(0), AL.stride(1), AL.size(2), Tf, ops._ptr(hold["seq"], torch.int64), Tf,
             ops._ptr(idx, torch.int64), idx.stride(0), ops._ptr(seg, torch.int32), None, None, rows, ops._ptr(att2), ops._ptr(node), ops._ptr(nw),
             ops._stream())
        scorer.enqueue(node, Tf, nw, tables, I, d_box, n_box, arena[o:o + g_words], plan)
        host = arena.cpu().numpy()                                        # the one copy (synchronises the stream)
        h_ll, h_tok = host[:2 * rows].view(np.float64).copy(), host[2 * rows:3 * rows].copy()
        entries = scorer.unpack(host[o:o + g_words], plan)
        for k, e, a, b in zip(ids, entries, bounds, bounds[1:]):
            out.append({"image_id": k, "gt_grounding": e,
                        "caption_ll": {"ll": h_ll[a:b], "n_tok": h_tok[a:b], "perplexity": forced.perplexity(h_ll[a:b], h_tok[a:b])}})
    return out
