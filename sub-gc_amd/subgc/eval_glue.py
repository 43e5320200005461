"""The model-facing part of the reference's evaluation loop (misc/eval_utils.py:98-146, misc/utils.py:59-81,
misc/grd_utils.py:36-58).

What `eval_split` does between the model call and the metric scripts: rank an image's captions by sGPN score,
map the kept sub-graphs back to their original indices, turn token rows into sentences, collect one
`predictions` entry per image and -- for the grounding experiments (`return_att_weight`) -- find for every word of
the chosen caption the graph node with the largest attention weight.  Here the model call is `sample_images`
(many images per decode batch); ranking, reordering and the grounding arg-max are ONE launch each over the whole
batch (`subgc_eval_rank_rows`, `subgc_grounding_argmax`) and everything the host needs arrives in ONE copy per
decode batch (`ops.eval_collect`).  The text side of the grounding protocol (lemma -> detection class, box files:
`grounding_material`) is dictionary look-ups on the host; the COCO / GVD metric scripts are out of scope.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops

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
    the number of groups), and an image whose kept rows differ from it in number is an error that names the image id."""
    import torch.distributed as dist
    from . import parallel
    eval_kwargs = dict(eval_kwargs or {})
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
    sct_mode = eval_kwargs.get("sct", 0) == 1
    rbe = eval_kwargs.get("remove_bad_endings", 0)
    return_att = eval_kwargs.get("return_att", 0) == 1
    if grd_pick is not None and len(grd_pick) != len(images):
        raise ValueError("caption_images: one grd_pick entry per image")
    if consensus is not None:
        if sct_mode:
            raise ValueError("caption_images: consensus re-ranking is not defined in sct (controllability) mode: its captions keep the "
                             "input order and are not ranked")
        missing = [info["id"] for info in infos if info["id"] not in consensus["nn"]]
        if missing:
            raise ValueError(f"caption_images: consensus['nn'] has no neighbour list for image ids {missing[:5]}")
    if diversity is not None:
        if sct_mode:
            raise ValueError("caption_images: diversity scores are not defined in sct (controllability) mode: its captions keep the input "
                             "order and are not ranked")
        from .diversity import TOP_N, per_image_draws
        d_scorer, d_top_n, d_seed = diversity["scorer"], tuple(diversity.get("top_n", TOP_N)), diversity.get("seed", 2019)
    if accuracy is not None:
        if sct_mode:
            raise ValueError("caption_images: accuracy scores are not defined in sct (controllability) mode: its captions keep the input "
                             "order and are not ranked")
        missing = [info["id"] for info in infos if info["id"] not in accuracy["index"]]
        if missing:
            raise ValueError(f"caption_images: accuracy['index'] names no reference image for image ids {missing[:5]}")
        a_scorer = accuracy["scorer"]
    if grounding is not None:
        if sct_mode:
            raise ValueError("caption_images: grounding scores are not defined in sct (controllability) mode: its captions keep the input "
                             "order and are not ranked")
        if not return_att:
            raise ValueError("caption_images: grounding scores need eval_kwargs['return_att'] = 1 (the attention arg-max of every word)")
        missing = [info["id"] for info in infos if info["id"] not in grounding["index"] or info["id"] not in grounding["boxes"]]
        if missing:
            raise ValueError(f"caption_images: grounding['index'] / ['boxes'] name no reference image or no boxes for image ids {missing[:5]}")
        from .grounding import prepare_boxes
        g_scorer, g_wh = grounding["scorer"], grounding.get("img_wh")
    if controllability is not None:
        if not sct_mode:
            raise ValueError("caption_images: controllability scores are defined only in sct (controllability) mode (eval_kwargs['sct'] = 1): "
                             "they need one caption per input region set, in input order")
        missing = [info["id"] for info in infos if info["id"] not in controllability["index"]]
        if missing:
            raise ValueError(f"caption_images: controllability['index'] names no first group for image ids {missing[:5]}")
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
            if "bounds" not in hold and consensus is not None:
                raise ValueError("caption_images: consensus re-ranking needs a model whose sample_images exposes the decode batch (batch_out)")
            if "bounds" not in hold and diversity is not None:
                raise ValueError("caption_images: diversity scores need a model whose sample_images exposes the decode batch (batch_out)")
            if "bounds" not in hold and accuracy is not None:
                raise ValueError("caption_images: accuracy scores need a model whose sample_images exposes the decode batch (batch_out)")
            if grounding is not None and ("bounds" not in hold or hold.get("AL") is None):
                raise ValueError("caption_images: grounding scores need a model whose sample_images exposes the decode batch and its attention "
                                 "buffer (batch_out)")
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
            div = None
            if diversity is not None:
                sizes = [b - a for a, b in zip(bounds, bounds[1:])]
                d_plan = d_scorer.plan(per_image_draws(sizes, [info["id"] for info in chunk_infos], d_top_n, d_seed), sizes)
                div = {"scorer": d_scorer, "plan": d_plan, "remove_bad_endings": rbe}
            if hold["rows"] == 0:
                d_none = None if div is None else d_scorer.unpack(d_plan, np.zeros((d_plan["n_sets"], ops.DIV_COLS + d_scorer.n_best), np.int32),
                                                                  np.zeros((d_plan["n_sets"], d_scorer.n_best + 1)), d_top_n)
                for j, info in enumerate(chunk_infos):
                    predictions.append({"image_id": info["id"], "caption": [], "subgraph_score": np.zeros(0, np.float32),
                                        "sorted_subgraph_ind": np.zeros(0, np.int64)})
                    if consensus is not None:
                        predictions[-1].update(consensus_rerank_ind=np.zeros(0, np.int64), consensus_sim=np.zeros(0, np.float64))
                    if div is not None:
                        predictions[-1]["diversity"] = d_none[j]
                    if accuracy is not None:
                        predictions[-1]["accuracy"] = a_scorer.unpack(np.zeros(a_scorer.arena_words(0, 1), np.int32), [0, 0])[0]
                    if grounding is not None:
                        predictions[-1]["grounding_score"] = g_scorer.empty_entry(g_scorer.check_index([grounding["index"][info["id"]]])[0])
                continue
            ground = return_att and hold.get("AL") is not None
            pick = None if grd_pick is None else grd_pick[i:i + group]
            # eval_utils.py:105-115 for every image of the batch + grd_utils.py:36-47: two launches, one host copy
            h = ops.eval_collect(hold["score"], hold["keep"], hold["seq"], bounds, identity=not model.gpn,
                                 AL=hold["AL"] if ground else None, idx=hold["idx"] if ground else None, pick=pick if ground else None,
                                 consensus=None if consensus is None else {
                                     "reranker": consensus["reranker"], "nn": [consensus["nn"][info["id"]] for info in chunk_infos],
                                     "top_k": consensus.get("top_k"), "remove_bad_endings": rbe}, diversity=div,
                                 accuracy=None if accuracy is None else {
                                     "scorer": a_scorer, "index": [accuracy["index"][info["id"]] for info in chunk_infos], "remove_bad_endings": rbe},
                                 grounding=None if grounding is None else {
                                     "scorer": g_scorer, "index": [grounding["index"][info["id"]] for info in chunk_infos], "remove_bad_endings": rbe,
                                     "boxes": [prepare_boxes(grounding["boxes"][info["id"]], None if g_wh is None else g_wh[info["id"]])
                                               for info in chunk_infos]})
            g_entries = None if grounding is None else g_scorer.unpack(h["g_words"], h["g_plan"])
            a_entries = None if accuracy is None else a_scorer.unpack(h["a_words"], bounds)
            d_entries = None if div is None else d_scorer.unpack(d_plan, h["d_int"], h["d_f64"], d_top_n)
            ctk = None if consensus is None else consensus.get("top_k")
            for j, (info, a, b) in enumerate(zip(chunk_infos, bounds, bounds[1:])):
                entry = {"image_id": info["id"], "caption": decode_sequence(ix_to_word, h["seq"][a:b], rbe),
                         "subgraph_score": h["score"][a:b], "sorted_subgraph_ind": h["keep"][a:b]}
                if consensus is not None:
                    nc = (b - a) if not ctk else min(b - a, int(ctk))
                    entry["consensus_rerank_ind"] = h["c_order"][a:a + nc].astype(np.int64)
                    entry["consensus_sim"] = h["c_sim"][a:a + nc].copy()
                if div is not None:
                    entry["diversity"] = d_entries[j]
                if accuracy is not None:
                    entry["accuracy"] = a_entries[j]
                if ground:
                    w = int(h["n_words"][j])
                    sub = int(pick[j]) if pick is not None else (int(h["c_first"][j]) if consensus is not None else 0)
                    entry["grounding"] = {"subg_index": sub, "sort_ind": h["order"][a:b],
                                          "att2_ind": h["att2"][j, :w].astype(np.int64), "node_ind": h["node"][j, :w].astype(np.int64)}
                    if grounding is not None:
                        entry["grounding_score"] = g_entries[j]
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
    from ._lib import SubgcError, call
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
