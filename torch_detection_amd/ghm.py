"""Gradient-harmonised losses of the dense anchor heads: GHM-C and GHM-R (Li et al., "Gradient Harmonized Single-stage
Detector", AAAI 2019), as mmdetection v1's ``GHMC`` / ``GHMR`` configure them (HIP kernels of csrc/ghm.hip; DESIGN.md
§4v has the exact arithmetic, tests/ghm_ref.py restates it).

They consume what ``anchor_target_all`` returns, as it is, and the head outputs in place.  Forward is four launches for
all levels and both losses, backward one; nothing synchronises with the host, so a training step can be captured in a
graph (a replay advances the running averages, like an optimizer's momentum); sums are fp64 in an order fixed by the
shapes, so two runs agree bit for bit.
"""
import torch
from torch import nn

from . import _lib
from . import ghm_ops as _g
from ._args import integer, number

__all__ = ["GHMHeadLossFunction", "ghm_head_loss", "GHMC", "GHMR"]


class GHMHeadLossFunction(torch.autograd.Function):
    """One autograd node for all levels and both losses: ``apply(meta, L, labels, label_weights, bbox_targets,
    bbox_weights, acc_cls, acc_reg, *cls_scores, *bbox_preds)``, ``meta`` = (num_classes, bins_cls, bins_reg,
    momentum_cls, momentum_reg, mu, scope).  The forward advances ``acc_cls`` / ``acc_reg`` in place and keeps the
    beta / tot table for the backward, which recomputes neither the counts nor the averages.  Targets get no gradient."""

    @staticmethod
    def forward(ctx, meta, L, labels, label_weights, bbox_targets, bbox_weights, acc_cls, acc_reg, *heads):
        targets = (labels, label_weights, bbox_targets, bbox_weights)
        losses, table = _g.ghm_head_loss_fwd(heads[:L], heads[L:], *targets, acc_cls, acc_reg, *meta)
        ctx.save_for_backward(*targets, table, *heads)
        ctx.meta, ctx.L = meta, L
        return losses

    @staticmethod
    def backward(ctx, g):
        targets, table, heads = ctx.saved_tensors[:4], ctx.saved_tensors[4], ctx.saved_tensors[5:]
        L = ctx.L
        g = g.to(torch.float32).contiguous()
        dcls, dreg = _g.ghm_head_loss_bwd(heads[:L], heads[L:], *targets, g, table, *ctx.meta)
        return (None,) * 8 + tuple(dcls) + tuple(dreg)


def ghm_head_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, acc_cls, acc_reg,
                  num_classes, bins_cls=30, bins_reg=10, momentum_cls=0.75, momentum_reg=0.7, mu=0.02, scope='level'):
    """GHM-C classification loss and GHM-R box loss of a dense anchor head over all levels.  Head outputs and targets
    are :func:`anchor_head_loss`'s.  A class element is valid iff its anchor's ``label_weights > 0``, a box element iff
    its ``bbox_weights > 0``; an invalid element is never evaluated.  ``acc_cls`` (bins_cls,) / ``acc_reg`` (bins_reg,)
    float32 CUDA tensors hold the running averages of the bin counts and are advanced in place by every call (``None``
    allowed when that momentum is 0).  ``scope='level'``: every level has a histogram of its own and advances the
    averages in turn, as mmdetection v1 does; ``'batch'``: one histogram over all levels.  Returns ``losses`` (2,) float32
    = [loss_cls, loss_bbox], each the sum over rows of ``sum(beta * l) / tot``; no ``loss_weight`` is applied."""
    cls_scores, bbox_preds = list(cls_scores), list(bbox_preds)
    if len(cls_scores) != len(bbox_preds):
        raise ValueError("%d cls_scores but %d bbox_preds" % (len(cls_scores), len(bbox_preds)))
    meta = (int(num_classes), bins_cls, bins_reg, momentum_cls, momentum_reg, mu, scope)
    return GHMHeadLossFunction.apply(meta, len(cls_scores), labels, label_weights, bbox_targets, bbox_weights, acc_cls,
                                     acc_reg, *cls_scores, *bbox_preds)


class _GHM(nn.Module):
    """Configuration and the running average ``acc_sum`` of one GHM loss.  As in mmdetection the average is no part of
    the state dict (a non-persistent buffer); it exists only with ``momentum > 0``.  The arithmetic is
    :func:`ghm_head_loss`'s: a head that holds a ``GHMC`` / ``GHMR`` pair calls it with both configurations."""

    def __init__(self, bins, momentum, loss_weight):
        super().__init__()
        self.bins = integer(bins, "bins", 1, _lib.GHM_MAX_BINS)
        self.momentum = _g._momentum(momentum, "momentum")
        self.loss_weight = number(loss_weight, "loss_weight")
        self.register_buffer("acc_sum", torch.zeros(self.bins) if self.momentum > 0 else None, persistent=False)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("%s holds a configuration: the loss of both terms is ghm_head_loss, which a head "
                                  "calls with its GHMC / GHMR pair" % type(self).__name__)


class GHMC(_GHM):
    """``GHMC(bins=10, momentum=0, use_sigmoid=True, loss_weight=1.0)``: mmdetection's constructor."""

    def __init__(self, bins=10, momentum=0, use_sigmoid=True, loss_weight=1.0):
        if not use_sigmoid:
            raise NotImplementedError("GHMC: only the sigmoid form exists (use_sigmoid=True)")
        super().__init__(bins, momentum, loss_weight)
        self.use_sigmoid = True


class GHMR(_GHM):
    """``GHMR(mu=0.02, bins=10, momentum=0, loss_weight=1.0)``: mmdetection's constructor."""

    def __init__(self, mu=0.02, bins=10, momentum=0, loss_weight=1.0):
        super().__init__(bins, momentum, loss_weight)
        self.mu = number(mu, "mu", positive=True)
