"""`LossWrapper`: model + language-model criterion, the module `train.py` wraps in DataParallel.

Same call signature and return dict as reference `models/loss_wrapper.py:14-27`; the criterion
(`misc/utils.py:115-124`) runs as the masked-NLL HIP kernels.  With `opt.label_smoothing > 0` the criterion is `LabelSmoothing`
(`misc/utils.py:126-156`), as in the upstream project's LossWrapper; the reference's own LossWrapper never reads the option.
"""
from __future__ import annotations

import torch

from .. import functions as F_
from .. import ops


class LanguageModelCriterion(torch.nn.Module):
    def forward(self, input, target, mask):
        target = target[:, : input.size(1)]
        mask = mask[:, : input.size(1)]
        return F_.MaskedNLLFn.apply(input, target, mask)


class LabelSmoothing(torch.nn.Module):
    """misc/utils.py:126-156, the reference's constructor signature (`size` and `padding_idx` are unused there as well): the masked KL
    divergence against the smoothed target distribution, in closed form on the device (include/subgc_criterion_hip.h)."""

    def __init__(self, size=0, padding_idx=0, smoothing=0.0):
        super().__init__()
        self.smoothing = ops.check_smoothing(smoothing)
        self.confidence = 1.0 - self.smoothing

    def forward(self, input, target, mask):
        target = target[:, : input.size(1)]
        mask = mask[:, : input.size(1)]
        return F_.SmoothedNLLFn.apply(input, target, mask, self.smoothing)


class RewardCriterion(torch.nn.Module):
    """misc/utils.py:89-109, the reference's signature: `input` [S, T] the log-probabilities gathered at `seq`, `reward` [S, T] (any per-token
    reward), `gpn_loss` [S] optional.  Runs as subgc_reward_nll_fwd / _bwd (include/subgc_selfcritical_hip.h); `reward` gets no gradient."""

    def forward(self, input, seq, reward, gpn_loss=None):
        return F_.RewardNLLFn.apply(input, seq, reward, gpn_loss)


class LossWrapper(torch.nn.Module):
    def __init__(self, model, opt, sc_reward=None, sc_samples=None):
        """`sc_reward`: a subgc.selfcritical.SelfCriticalReward; with it `forward(..., sc_flag=True)` is a self-critical step.
        `sc_samples` (default: `opt.train_sample_n`, else 1): the samples per caption row of such a step.  1: the rollout with its greedy
        baseline and the replay, every launch as before; 2 .. 16: one decoder pass over n samples per row, each sample's baseline the
        mean score of the others (subgc/selfcritical.py); anything else raises ValueError."""
        super().__init__()
        from ..selfcritical import check_samples
        self.sc_reward = sc_reward
        self.sc_samples = check_samples(getattr(opt, "train_sample_n", 1) if sc_samples is None else sc_samples)
        self.opt = opt
        self.model = model
        # `opt` may be None (the benchmark and the tools) or lack the attribute: LanguageModelCriterion, every launch as before
        self.label_smoothing = ops.check_smoothing(getattr(opt, "label_smoothing", 0) or 0)
        if self.label_smoothing > 0:
            self.crit = LabelSmoothing(smoothing=self.label_smoothing)
        else:
            self.crit = LanguageModelCriterion()

    def forward(self, fc_feats, att_feats, labels, masks, att_masks, gts, gt_indices, trip_pred, obj_dist, obj_box, rel_ind,
                pred_fmap, pred_dist, gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind, gpn_pool_mtx, sc_flag=False):
        """`sc_flag` (the upstream name): a self-critical step -- the language loss is RewardCriterion on a rollout of the model's own,
        `gt_indices` are the images' positions in the RewardReferences, `gts` is not read, `label_smoothing` does not apply, and the
        result carries the mean reward as well.  False or absent: every launch as before."""
        if sc_flag:
            return self._forward_sc(fc_feats, att_feats, labels, att_masks, gt_indices, trip_pred, obj_dist, obj_box, rel_ind, pred_fmap,
                                    pred_dist, gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind, gpn_pool_mtx)
        T = labels.size(1) - 1
        fused = (labels[:, 1:], masks[:, 1:T + 1]) if getattr(self.model, "supports_fused_crit", False) else None
        kw = {"fused_crit": fused, "need_outputs": False} if fused is not None else {}
        if fused is not None and self.label_smoothing > 0:
            kw["label_smoothing"] = self.label_smoothing
        lang_output, gpn_loss, subgraph_score = self.model(fc_feats, att_feats, labels, att_masks, trip_pred, obj_dist, obj_box,
                                                           rel_ind, pred_fmap, pred_dist, gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind,
                                                           gpn_pool_mtx, **kw)
        if fused is not None:
            lang_loss = self.model.fused_lang_loss          # criterion evaluated inside the decoder Function
        else:
            lang_loss = self.crit(lang_output, labels[:, 1:], masks[:, 1:]) if lang_output is not None else None
        return {"gpn_loss": gpn_loss, "lang_loss": lang_loss}

    def _forward_sc(self, fc_feats, att_feats, labels, att_masks, gt_indices, trip_pred, obj_dist, obj_box, rel_ind, pred_fmap, pred_dist,
                    gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind, gpn_pool_mtx):
        if self.sc_reward is None:
            raise ops.SubgcError("LossWrapper: sc_flag=True needs a reward: build subgc.selfcritical.RewardReferences from the training captions "
                                 "and pass LossWrapper(model, opt, sc_reward=subgc.selfcritical.SelfCriticalReward(refs, cider_weight, bleu_weight))")
        if not getattr(self.model, "supports_fused_crit", False):
            raise ops.SubgcError("LossWrapper: a self-critical step needs a model whose _forward takes `self_critical` (AttModel)")
        if torch.is_tensor(gt_indices) and gt_indices.is_cuda:
            d_index = gt_indices.to(torch.int32)             # already on the device: debug bounds mode checks it (subgc_accuracy_rows)
        else:
            idx = self.sc_reward.check_index(gt_indices.tolist() if torch.is_tensor(gt_indices) else gt_indices)
            d_index = ops.upload(idx, torch.int32, att_feats.device)
        _, gpn_loss, _ = self.model(fc_feats, att_feats, labels, att_masks, trip_pred, obj_dist, obj_box, rel_ind, pred_fmap, pred_dist,
                                    gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind, gpn_pool_mtx, need_outputs=False,
                                    self_critical=(self.sc_reward, d_index) if self.sc_samples == 1 else (self.sc_reward, d_index, self.sc_samples))
        return {"gpn_loss": gpn_loss, "lang_loss": self.model.fused_lang_loss, "reward": self.model.sc_stats["reward"]}
