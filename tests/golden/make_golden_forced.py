#!/usr/bin/env python
"""Write the forced-decode fixture by DRIVING THE REFERENCE MODEL's own modules along given token rows where the reference lies (never
copied): forced_case.npz + forced_meta.json.  Data only: the token rows, the per-step log-probabilities of the forced tokens, the per-step
attention rows, the node lists, the arg-max nodes and LanguageModelCriterion's masked mean.

    python tests/golden/make_golden_forced.py        (then make_golden_grounding_gt.py, whose `model` set reads this file)

The tiny golden options and weights of make_golden.py (subgc_beam / fullgc_train; drop_prob_lm = 0, eval mode).  Per image the reference's
`feat_fusion`, `gcn_backbone`, the sGPN test branch (`gpn_layer` with `use_nms` off on the instance: every candidate in input order) or the
Full-GC read-out of AttModel.py:261-271, `_prepare_feature`, and then `get_logprobs_state(return_att=True)` step by step: step j is fed
word j - 1 (<bos> at 0; 0 behind the end token, like `it * unfinished`) and scores word j.  One sub-GC case of 3 images x 5 candidates
(the first five of the image's 2 M) and one Full-GC case of 2 images x 5 captions (the image's row repeated).

The script fails unless at every compared (row, live step) the two largest attention weights differ by more than 1e-4 relative, so the
arg-max node the tests compare is well defined; the seeds below pass."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                               # noqa: E402
from subgc import synthetic                                            # noqa: E402

TF = MG.TINY["seq_length"] + 1                                         # GtCaptionRows' width: a full-length caption's end token is scored
GAP = 1e-4


def token_rows(rng, n, V):
    """n rows of TF columns: words 1 .. V, then zeros; lengths vary, the last row is full-length (its end token sits in the last column)."""
    tok = np.zeros((n, TF), np.int64)
    for r in range(n):
        L = TF - 1 if r == n - 1 else int(rng.integers(2, TF - 2))
        tok[r, :L] = rng.integers(1, V + 1, L)
    return tok


def drive(model, batch, tok, gpn, n_rows):
    """-> (lp [n, TF], alpha [n, TF, N], idx [n, N], logprobs [n, TF, V + 1]) along tok, by the reference's own modules."""
    (fc_feats, att_feats, att_masks, _t, obj_dist, _b, rel_ind, _f, pred_dist, gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind,
     gpn_pool_mtx) = synthetic.sample_args({k: v.clone() for k, v in batch.items()})
    att_feats, pred_fmap = model.feat_fusion(obj_dist, att_feats, pred_dist)
    b, N, K, L = att_feats.size(0), att_feats.size(1), rel_ind.size(1), model.GCN_dim
    att_feats, x_pred = model.gcn_backbone(b, N, K, L, att_feats, obj_dist, pred_fmap, rel_ind)
    b = att_feats.size(0)
    if gpn:
        model.gpn_layer.use_nms = False                                # every candidate, input order
        _, _, att_feats, fc_feats, att_masks, keep = model.gpn_layer(b, N, K, L, gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind, gpn_pool_mtx, att_feats,
                                                                     x_pred, fc_feats, att_masks)
        assert keep.tolist() == list(range(keep.numel())) and keep.numel() >= n_rows
        att_feats, fc_feats, att_masks = att_feats[:n_rows], fc_feats[:n_rows], att_masks[:n_rows]
        idx = gpn_obj_ind[0].contiguous().view(-1, N)[:n_rows]
    else:
        att_feats = att_feats[0:1]
        fc_feats = model.read_out_proj(torch.mean(att_feats, 1))
        att_masks = att_masks[0:1, 0, 0]
        att_masks[:, :36].fill_(1.0)
        att_feats, fc_feats, att_masks = att_feats.expand(n_rows, -1, -1), fc_feats.expand(n_rows, -1), att_masks.expand(n_rows, -1)
        idx = torch.arange(N).view(1, N).expand(n_rows, N)
    state = model.init_hidden(n_rows)
    p_fc, p_att, pp_att, p_masks = model._prepare_feature(fc_feats.contiguous(), att_feats.contiguous(), att_masks.contiguous())
    t_tok = torch.from_numpy(tok)
    lps, alphas = [], []
    for t in range(TF):
        it = torch.zeros(n_rows, dtype=torch.long) if t == 0 else t_tok[:, t - 1]
        logprobs, state, att = model.get_logprobs_state(it, p_fc, p_att, pp_att, p_masks, state, return_att=True)
        lps.append(logprobs)
        a = torch.zeros(n_rows, N)
        a[:, :att.size(1)] = att
        alphas.append(a)
    logprobs = torch.stack(lps, 1)
    return logprobs.gather(2, t_tok.unsqueeze(2)).squeeze(2), torch.stack(alphas, 1), idx, logprobs


def main():
    assert os.path.isdir(MG.REF), "golden vectors can only be regenerated where the reference exists"
    MG.enter_scratch()
    from misc.utils import LanguageModelCriterion
    from models.AttModel import TopDownModel
    with np.load(os.path.join(HERE, "subgc_beam_weights.npz")) as z:
        w = {k: z[k].copy() for k in z.files}
    with np.load(os.path.join(HERE, "fullgc_train_weights.npz")) as z:
        wf = {k: z[k].copy() for k in z.files}
    t = dict(test_LSTM=1, gpn_nms_thres=0.75, gpn_max_subg=10)
    fo = dict(use_gpn=0, noun_fuse=0, pred_emb_type=2, gcn_layers=4, gcn_residual=1, gcn_bn=1)
    cases = [("subgc", MG.ref_opt(**t), w, True, [(3, None, 920), (4, 14, 921), (6, 10, 922)]),
             ("fullgc", MG.ref_opt(**fo), wf, False, [(2, None, 930), (3, None, 931)])]
    V, n_rows = MG.TINY["vocab_size"], 5
    rng = np.random.default_rng(1117)
    arr, meta = {}, {"Tf": TF, "gap": GAP, "cases": {}}
    crit = LanguageModelCriterion()
    for name, opt, weights, gpn, imgs in cases:
        torch.manual_seed(3)
        model = TopDownModel(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
        model.eval()
        toks, lps, alphas, idxs, nodes, full, boxes = [], [], [], [], [], [], []
        for M, pool, seed in imgs:
            batch = synthetic.make_test_batch(M, D=opt.att_feat_size, seed=seed, fc_size=opt.att_feat_size, node_pool=pool)
            tok = token_rows(rng, n_rows, V)
            with torch.no_grad():
                lp, alpha, idx, logprobs = drive(model, batch, tok, gpn, n_rows)
            live = np.concatenate([np.ones((n_rows, 1), bool), np.cumprod(tok[:, :-1] > 0, 1).astype(bool)], 1)
            words = np.cumprod(tok > 0, 1).astype(bool)                 # the positions the arg-max is compared at
            a = alpha.numpy()
            top2 = np.sort(a, 2)[:, :, -2:]
            gap = (top2[:, :, 1] - top2[:, :, 0]) / top2[:, :, 1]
            assert (gap[words] > GAP).all(), (name, seed, "attention arg-max is not well separated", float(gap[words].min()))
            node = np.where(words, np.take_along_axis(idx.numpy(), a.argmax(2), 1), -1)
            toks.append(tok); lps.append(np.where(live, lp.numpy(), 0).astype(np.float32)); alphas.append(a.astype(np.float32))
            idxs.append(idx.numpy().astype(np.int64)); nodes.append(node.astype(np.int32)); full.append(logprobs)
            xy, wh_ = rng.random((a.shape[2], 2)) * 300, 5 + rng.random((a.shape[2], 2)) * 200
            boxes.append(np.concatenate([xy, xy + wh_], 1))
        tok_all = np.concatenate(toks)
        live = np.concatenate([np.ones((len(tok_all), 1), bool), np.cumprod(tok_all[:, :-1] > 0, 1).astype(bool)], 1)
        with torch.no_grad():
            mean = crit(torch.cat(full), torch.from_numpy(tok_all), torch.from_numpy(live.astype(np.float32)))
        arr[name + "_tokens"], arr[name + "_lp"], arr[name + "_att"] = tok_all, np.concatenate(lps), np.concatenate(alphas)
        arr[name + "_idx"], arr[name + "_node"] = np.concatenate(idxs), np.concatenate(nodes)
        arr[name + "_bounds"] = np.arange(len(imgs) + 1, dtype=np.int64) * n_rows
        arr[name + "_masked_mean"] = np.asarray([float(mean)], np.float64)
        arr[name + "_boxes"] = np.concatenate(boxes)
        arr[name + "_box_off"] = np.concatenate([[0], np.cumsum([len(b) for b in boxes])]).astype(np.int64)
        meta["cases"][name] = dict(images=[dict(M=M, pool=pool, seed=seed) for M, pool, seed in imgs], rows_per_image=n_rows,
                                   weights="subgc_beam" if gpn else "fullgc_train", opt={k: v for k, v in vars(opt).items() if "path" not in k},
                                   live_steps=int(live.sum()))
        print(name, "rows", len(tok_all), "live steps", int(live.sum()), "masked mean", float(mean))
    np.savez_compressed(os.path.join(HERE, "forced_case.npz"), **arr)
    with open(os.path.join(HERE, "forced_meta.json"), "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote forced_case.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "forced_case.npz")))


if __name__ == "__main__":
    main()
