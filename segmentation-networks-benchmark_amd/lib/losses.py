"""Segmentation losses on the fused HIP loss kernels -- drop-in for the reference's ``lib.losses``
(the reference's lib/losses.py).

Binary losses (losses.py:7-101, segnb.seglosses): class names, constructor signatures and numerics follow the reference,
including its quirks:
  * ``BCEWithSigmoidLoss`` applies the sigmoid twice (logsigmoid, then BCE-with-logits; losses.py:51-53)
  * Jaccard / Dice sums run over the WHOLE batch tensor, not per image (losses.py:13-14,23-24,39-40)
  * ``FocalLossBinary(size_average=False)`` is a SUM (torch_train.py:92)
Each forward is two kernel launches (global sums + finalize), backward one; nothing syncs the host.

Multi-class losses (losses.py:105-232, segnb.mcloss): logits [N,C,H,W], target [N,H,W] class indices, 1 <= C <= 256.  Each
forward is one launch on one device (two under data parallel), backward one.  Kept quirks of the reference:
  * ``FocalLossMulti(size_average=True)`` is the mean over ALL N*H*W pixels, ignored ones included; ``reduce`` is ignored
  * ``JaccardLossMulti``: smooth 100, the mask is ``target != ignore_index``, a class absent from the masked targets adds 0
  * the combinations divide by ``1 + jaccard_weight`` (the weight appears only in the denominator)
Deviations:
  * the legacy ``size_average`` / ``reduce`` arguments are stored on the instance (torch 2.x ``_Loss`` no longer does, and
    the reference's multi-class losses fail there with AttributeError)
  * ``NLLLAndJaccardLossMulti`` names an undefined ``NLLLoss`` in the reference (NameError); here it is
    ``torch.nn.NLLLoss(weight, ignore_index)``
  * a label outside [0, C) that is not ignore_index raises in the reference; here it adds nothing to the focal / NLL terms,
    stays inside the Jaccard mask without belonging to a class, and is counted (``mc_loss.last_fin[5]``)
  * the combinations take the fused mode-0 pass (softmax of the raw logits) where the reference applies log_softmax and then
    exp: equal up to rounding
"""
from torch.nn.modules.loss import _Loss

import torch
from torch import nn

from segnb.mcloss import make_cfg, mc_loss
from segnb.seglosses import make_spec, seg_loss, seg_loss_map


class DiceLoss(_Loss):
    def __init__(self):
        super(DiceLoss, self).__init__()
        self._spec = make_spec(w_dice=1.0)

    def forward(self, output, target):
        return seg_loss(output, target, self._spec)


class JaccardLoss(_Loss):
    def __init__(self):
        super(JaccardLoss, self).__init__()
        self._spec = make_spec(w_jaccard=1.0)

    def forward(self, output, target):
        return seg_loss(output, target, self._spec)


class SmoothJaccardLoss(_Loss):
    def __init__(self, smooth=100):
        super(SmoothJaccardLoss, self).__init__()
        self.smooth = smooth

    def forward(self, output, target):
        return seg_loss(output, target, make_spec(w_sjaccard=1.0, smooth=self.smooth))


class BCEWithSigmoidLoss(_Loss):
    def __init__(self, size_average=True, reduce=True):
        super(BCEWithSigmoidLoss, self).__init__()
        self.size_average, self.reduce = size_average, reduce

    def forward(self, outputs, targets):
        # the legacy (size_average, reduce) pair of F.binary_cross_entropy_with_logits (losses.py:53):
        # reduce=False -> per-pixel map; else mean (size_average) or sum
        if not self.reduce:
            return seg_loss_map(outputs, targets, 0)
        return seg_loss(outputs, targets, make_spec(w_bce=1.0, bce_sum=0 if self.size_average else 1))


class BCEWithLogitsLossAndSmoothJaccard(_Loss):
    """(bce_weight * BCE + jaccard_weight * SmoothJaccard) / (bce_weight + jaccard_weight), arXiv:1706.06169"""

    def __init__(self, bce_weight=1, jaccard_weight=0.5):
        super(BCEWithLogitsLossAndSmoothJaccard, self).__init__()
        self.bce_loss = BCEWithSigmoidLoss()
        self.jac_loss = SmoothJaccardLoss()
        self.bce_weight = bce_weight
        self.jaccard_weight = jaccard_weight

    def forward(self, outputs, targets):
        spec = make_spec(w_bce=self.bce_weight, w_sjaccard=self.jaccard_weight, smooth=self.jac_loss.smooth,
                         norm=self.bce_weight + self.jaccard_weight)
        return seg_loss(outputs, targets, spec)


class BCEAndDiceLoss(_Loss):
    """(bce_weight * BCE + dice_weight * Dice) / (bce_weight + dice_weight).  Build-defined: BASELINE.json
    config 2 names "BCE+Dice"; the reference ships both terms (losses.py:7,46) but no wired combination."""

    def __init__(self, bce_weight=1, dice_weight=1):
        super(BCEAndDiceLoss, self).__init__()
        self.bce_weight, self.dice_weight = bce_weight, dice_weight

    def forward(self, outputs, targets):
        spec = make_spec(w_bce=self.bce_weight, w_dice=self.dice_weight, norm=self.bce_weight + self.dice_weight)
        return seg_loss(outputs, targets, spec)


class FocalLossBinary(_Loss):
    def __init__(self, gamma=2, size_average=True, reduce=True):
        super(FocalLossBinary, self).__init__()
        self.gamma = gamma
        self.size_average, self.reduce = size_average, reduce

    def forward(self, outputs, targets):
        # `reduce` is accepted and ignored, as in the reference (losses.py:97-101 always reduces)
        return seg_loss(outputs, targets, make_spec(w_focal=1.0, focal_mean=1 if self.size_average else 0,
                                                    focal_gamma=self.gamma))


class FocalLossMulti(_Loss):
    """-(1 - pt)^gamma log pt of the target class; ``outputs`` are logits, or log-probabilities with from_logits=True."""

    def __init__(self, gamma=2, size_average=True, reduce=True, ignore_index=-100, from_logits=False):
        super(FocalLossMulti, self).__init__()
        self.size_average, self.reduce = size_average, reduce
        self.gamma = gamma
        self.ignore_index = ignore_index
        self.from_logits = from_logits

    def forward(self, outputs, targets):
        return mc_loss(outputs, targets, make_cfg(mode=1 if self.from_logits else 0, ignore_index=self.ignore_index,
                                                  gamma=self.gamma, w_focal=1.0, focal_mean=1 if self.size_average else 0))


class JaccardLossMulti(_Loss):
    """Per-class smooth Jaccard (smooth = 100), weighted by ``weight / weight.sum()``; reduce=False returns the [C] vector."""

    def __init__(self, ignore_index=-100, from_logits=False, weight=None, reduce=True):
        super(JaccardLossMulti, self).__init__()
        self.reduce = reduce
        self.ignore_index = ignore_index
        self.from_logits = from_logits
        self.class_weights = None if weight is None else weight / weight.sum()

    def forward(self, outputs, targets):
        return mc_loss(outputs, targets, make_cfg(mode=1 if self.from_logits else 0, ignore_index=self.ignore_index,
                                                  w_jaccard=1.0, reduce=1 if self.reduce else 0),
                       jac_weight=self.class_weights)


class FocalAndJaccardLossMulti(_Loss):
    """(focal + jaccard) / (1 + jaccard_weight) on log_softmax(outputs), as the reference."""

    def __init__(self, jaccard_weight=1, class_weights=None, ignore_index=-1):
        super(FocalAndJaccardLossMulti, self).__init__()
        nll_weight = None if class_weights is None else torch.from_numpy(class_weights).float()
        self.focal_loss = FocalLossMulti(ignore_index=ignore_index, from_logits=True)
        self.jaccard_loss = JaccardLossMulti(ignore_index=ignore_index, from_logits=True, weight=nll_weight)
        self.jaccard_weight = jaccard_weight

    def forward(self, outputs, targets):
        f, j = self.focal_loss, self.jaccard_loss
        return mc_loss(outputs, targets, make_cfg(mode=0, ignore_index=f.ignore_index, gamma=f.gamma, w_focal=1.0, w_jaccard=1.0,
                                                  norm=1 + self.jaccard_weight, focal_mean=1 if f.size_average else 0),
                       jac_weight=j.class_weights)


class NLLLAndJaccardLossMulti(_Loss):
    """(NLL + jaccard) / (1 + jaccard_weight) on log_softmax(outputs); NLL = nn.NLLLoss(weight, ignore_index)."""

    def __init__(self, jaccard_weight=1, class_weights=None, ignore_index=-1):
        super(NLLLAndJaccardLossMulti, self).__init__()
        nll_weight = None if class_weights is None else torch.from_numpy(class_weights).float()
        self.nll_loss = nn.NLLLoss(weight=nll_weight, ignore_index=ignore_index)
        self.jaccard_loss = JaccardLossMulti(ignore_index=ignore_index, from_logits=True, weight=nll_weight)
        self.jaccard_weight = jaccard_weight

    def forward(self, outputs, targets):
        return mc_loss(outputs, targets, make_cfg(mode=0, ignore_index=self.nll_loss.ignore_index, w_nll=1.0, w_jaccard=1.0,
                                                  norm=1 + self.jaccard_weight),
                       nll_weight=self.nll_loss.weight, jac_weight=self.jaccard_loss.class_weights)
