"""Losses of the dense anchor heads (RPN, RetinaNet) and of the RoI box head, with their gradients (HIP kernels of
csrc/loss.hip; DESIGN.md §4e has the exact arithmetic, tests/loss_ref.py restates it).

They consume what ``anchor_target`` / ``sample_rois`` return, as it is: no permuted copies of the head outputs, no
``(N, 4C)`` expanded targets, no host synchronisation for the divisor.  Forward is two launches for all levels and both
losses, backward one; sums are fp64 in an order fixed by the shapes, so two runs agree bit for bit, eager or replayed
from a graph.  An element whose weight is exactly 0 is never evaluated (loss 0, gradient 0, whatever its logit).
"""
import torch

from . import libra_ops as _b
from . import loss_ops as _l

__all__ = ["AnchorHeadLossFunction", "BBoxHeadLossFunction", "BalancedBBoxHeadLossFunction", "anchor_head_loss",
           "rpn_loss", "bbox_head_loss"]


def _avg_tensors(avg_factor):
    """(what goes through ``apply`` as tensors, how to put it together again)."""
    if torch.is_tensor(avg_factor):
        return (avg_factor,), lambda ts: ts[0]
    if isinstance(avg_factor, (tuple, list)):
        return tuple(avg_factor), lambda ts: tuple(ts)
    return (), lambda ts: avg_factor


class AnchorHeadLossFunction(torch.autograd.Function):
    """One autograd node for all levels and both losses: ``apply(meta, avg_number, n_avg, L, labels, label_weights,
    bbox_targets, bbox_weights, *avg_tensors, *cls_scores, *bbox_preds)``.  Targets get no gradient."""

    @staticmethod
    def forward(ctx, meta, avg_number, n_avg, L, labels, label_weights, bbox_targets, bbox_weights, *rest):
        avg_ts, heads = rest[:n_avg], rest[n_avg:]
        avg_factor = avg_number if n_avg == 0 else tuple(avg_ts)
        targets = (labels, label_weights, bbox_targets, bbox_weights)
        losses, avg = _l.anchor_head_loss_fwd(heads[:L], heads[L:], *targets, avg_factor, *meta)
        ctx.save_for_backward(*targets, *heads)
        ctx.meta, ctx.L, ctx.n_avg, ctx.avg = meta, L, n_avg, avg
        return losses

    @staticmethod
    def backward(ctx, g):
        targets, heads = ctx.saved_tensors[:4], ctx.saved_tensors[4:]
        L = ctx.L
        g = g.to(torch.float32).contiguous()
        dcls, dreg = _l.anchor_head_loss_bwd(heads[:L], heads[L:], *targets, g, ctx.avg, *ctx.meta)
        return (None,) * (8 + ctx.n_avg) + tuple(dcls) + tuple(dreg)


class BBoxHeadLossFunction(torch.autograd.Function):
    """``apply(beta, avg_number, n_avg, labels, label_weights, bbox_targets, bbox_weights, *avg_tensors, cls_score,
    bbox_pred)``."""

    @staticmethod
    def forward(ctx, beta, avg_number, n_avg, labels, label_weights, bbox_targets, bbox_weights, *rest):
        avg_ts, (cls_score, bbox_pred) = rest[:n_avg], rest[n_avg:]
        avg_factor = avg_number if n_avg == 0 else tuple(avg_ts)
        targets = (labels, label_weights, bbox_targets, bbox_weights)
        losses, avg = _l.bbox_head_loss_fwd(cls_score, bbox_pred, *targets, avg_factor, beta)
        ctx.save_for_backward(*targets, cls_score, bbox_pred)
        ctx.beta, ctx.n_avg, ctx.avg = beta, n_avg, avg
        return losses

    @staticmethod
    def backward(ctx, g):
        targets, (cls_score, bbox_pred) = ctx.saved_tensors[:4], ctx.saved_tensors[4:]
        g = g.to(torch.float32).contiguous()
        dcls, dreg = _l.bbox_head_loss_bwd(cls_score, bbox_pred, *targets, g, ctx.avg, ctx.beta)
        return (None,) * (7 + ctx.n_avg) + (dcls, dreg)


class BalancedBBoxHeadLossFunction(torch.autograd.Function):
    """:class:`BBoxHeadLossFunction` with balanced L1 as the box term: ``apply((beta, alpha, gamma), avg_number, n_avg,
    labels, label_weights, bbox_targets, bbox_weights, *avg_tensors, cls_score, bbox_pred)``."""

    @staticmethod
    def forward(ctx, meta, avg_number, n_avg, labels, label_weights, bbox_targets, bbox_weights, *rest):
        avg_ts, (cls_score, bbox_pred) = rest[:n_avg], rest[n_avg:]
        avg_factor = avg_number if n_avg == 0 else tuple(avg_ts)
        targets = (labels, label_weights, bbox_targets, bbox_weights)
        losses, avg = _b.bbox_head_loss_balanced_fwd(cls_score, bbox_pred, *targets, avg_factor, *meta)
        ctx.save_for_backward(*targets, cls_score, bbox_pred)
        ctx.meta, ctx.n_avg, ctx.avg = meta, n_avg, avg
        return losses

    @staticmethod
    def backward(ctx, g):
        targets, (cls_score, bbox_pred) = ctx.saved_tensors[:4], ctx.saved_tensors[4:]
        g = g.to(torch.float32).contiguous()
        dcls, dreg = _b.bbox_head_loss_balanced_bwd(cls_score, bbox_pred, *targets, g, ctx.avg, *ctx.meta)
        return (None,) * (7 + ctx.n_avg) + (dcls, dreg)


def anchor_head_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor,
                     num_classes=1, beta=1.0 / 9.0, gamma=None, alpha=0.25):
    """Sigmoid classification loss (binary cross entropy, or focal with ``gamma`` / ``alpha``) and smooth-L1 box loss of
    a dense anchor head over all levels.  ``cls_scores[l]``: (B, A*C, H_l, W_l), class channel ``a*C + c``;
    ``bbox_preds[l]``: (B, 4A, H_l, W_l), box channel ``4a + j``; float32 / bfloat16 / float16, NCHW-contiguous or
    channels_last (levels may differ).  The targets are ``anchor_target``'s (B, N) / (B, N, 4) tensors, N level-major
    with anchor ``(h*W + w)*A + a`` within a level; label 0 is background, label k in 1..C is class channel k-1.
    ``avg_factor``: a positive number, a CUDA int32 tensor, or a tuple of up to two (``(num_pos, num_neg)``): the
    divisor is their integer sum, at least 1, taken on the device.  Returns ``losses`` (2,) float32 =
    [loss_cls, loss_bbox]; its backward gives every head output a gradient of its own shape, dtype and strides."""
    cls_scores, bbox_preds = list(cls_scores), list(bbox_preds)
    if len(cls_scores) != len(bbox_preds):
        raise ValueError("%d cls_scores but %d bbox_preds" % (len(cls_scores), len(bbox_preds)))
    avg_ts, _ = _avg_tensors(avg_factor)
    meta = (int(num_classes), beta, gamma, alpha)
    return AnchorHeadLossFunction.apply(meta, avg_factor if not avg_ts else None, len(avg_ts), len(cls_scores), labels,
                                        label_weights, bbox_targets, bbox_weights, *avg_ts, *cls_scores, *bbox_preds)


def rpn_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor, beta=1.0 / 9.0):
    """:func:`anchor_head_loss` of an RPN head: one class, binary cross entropy."""
    return anchor_head_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor,
                            num_classes=1, beta=beta, gamma=None)


def bbox_head_loss(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, avg_factor=None, beta=1.0,
                   reg_loss='smooth_l1', reg_alpha=0.5, reg_gamma=1.5):
    """Softmax cross entropy and the box loss of the RoI head on ``sample_rois``' rows.  ``cls_score``: (R, C),
    class 0 background; ``bbox_pred``: (R, 4C) (row r regresses columns ``4*labels[r] ..``, every other column gets
    gradient 0) or (R, 4); targets stay (R, 4).  ``avg_factor``: as for :func:`anchor_head_loss`, or None for the number
    of rows with ``label_weights > 0`` (counted on the device, at least 1).  Padding rows (weight 0) are never read.
    ``reg_loss``: ``'smooth_l1'`` with knee ``beta``, or ``'balanced_l1'`` (Libra R-CNN) with knee ``beta`` and the shape
    parameters ``reg_alpha`` / ``reg_gamma``, which smooth L1 does not look at."""
    avg_ts, _ = _avg_tensors(avg_factor)
    if reg_loss == 'balanced_l1':
        return BalancedBBoxHeadLossFunction.apply((beta, reg_alpha, reg_gamma), avg_factor if not avg_ts else None,
                                                  len(avg_ts), labels, label_weights, bbox_targets, bbox_weights, *avg_ts,
                                                  cls_score, bbox_pred)
    if reg_loss != 'smooth_l1':
        raise ValueError("reg_loss must be 'smooth_l1' or 'balanced_l1', got %r" % (reg_loss,))
    return BBoxHeadLossFunction.apply(beta, avg_factor if not avg_ts else None, len(avg_ts), labels, label_weights,
                                      bbox_targets, bbox_weights, *avg_ts, cls_score, bbox_pred)
