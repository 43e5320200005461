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


class LossWrapper(torch.nn.Module):
    def __init__(self, model, opt):
        super().__init__()
        self.opt = opt
        self.model = model
        # `opt` may be None (the benchmark and the tools) or lack the attribute: LanguageModelCriterion, every launch as before
        self.label_smoothing = ops.check_smoothing(getattr(opt, "label_smoothing", 0) or 0)
        if self.label_smoothing > 0:
            self.crit = LabelSmoothing(smoothing=self.label_smoothing)
        else:
            self.crit = LanguageModelCriterion()

    def forward(self, fc_feats, att_feats, labels, masks, att_masks, gts, gt_indices, trip_pred, obj_dist, obj_box, rel_ind,
                pred_fmap, pred_dist, gpn_obj_ind, gpn_pred_ind, gpn_nrel_ind, gpn_pool_mtx):
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
