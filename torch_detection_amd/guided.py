"""Guided Anchoring (Wang et al., CVPR 2019) head operations: location targets, shape targets, the location + shape
loss and the guided anchors (HIP kernels of csrc/guided.hip; DESIGN.md §4w has the specification, tests/ga_ref.py
restates it).  Names and semantics follow mmdetection v1's ``GuidedAnchorHead``.

The pyramid is given as ``featmap_sizes`` = [(H_l, W_l)] and integer ``strides``; locations are level-major,
``(y*W_l + x)`` within a level, ``Nloc = sum H_l*W_l``.  Boxes are float32 inclusive '+1' xyxy; ground truths come
padded as in ``target.py``: ``gt_bboxes`` (B, G, 4) with ``gt_counts`` (B,) int32.  Nothing synchronises with the host,
so every function can be captured in a graph; outputs have fixed shapes and are a pure function of the inputs, bit for
bit from run to run.
"""
import torch

from . import guided_ops as _g

__all__ = ["GALossFunction", "ga_loc_target", "ga_shape_target", "ga_loss", "guided_anchors", "ga_rpn_proposals"]

ANCHORING_MEANS = (0.0, 0.0, 0.0, 0.0)
ANCHORING_STDS = (0.07, 0.07, 0.14, 0.14)


def ga_loc_target(featmap_sizes, strides, anchor_scale, gt_bboxes, gt_counts, center_ratio=0.2, ignore_ratio=0.5):
    """Location targets of a Guided Anchoring head (mmdetection v1's ``ga_loc_target`` for a whole batch), one launch.

    A ground truth lies on level ``#{k in 1..L-1 : area >= t_k}``, ``area`` the float32 product of its '+1' sides and
    ``t_k = m^2 2^(2k-1)``, ``m = anchor_scale * strides[0]`` — mmdetection's ``floor(log2(sqrt(w h)) - log2(m) + 0.5)``
    clamped to the level range, stated on areas so that it is exact.  On that level it paints its centre region
    (``center_ratio``: target 1, weight 1) over its ignore region (``ignore_ratio``: weight 0); on the level above and
    the level below its ignore region makes unpainted locations weight 0.  A region of ratio ``rho`` is ``x1 =
    rint(c*g.x1 + r*g.x2)``, ``x2 = rint(r*g.x1 + c*g.x2)`` (the same for y) with ``g = gt / stride``,
    ``r = (1 - rho)/2``, ``c = 1 - r``, float32, rounding half to even, clamped to the map.  Ground truths are applied
    in ascending index: a later box's ignore region erases an earlier box's weight 1 but not its target 1.

    Returns ``loc_targets`` (B, Nloc) int64 in {0, 1}, ``loc_weights`` (B, Nloc) float32 in {0, 0.1, 1} and
    ``loc_avg_factor = B * Nloc / 200`` (a Python float).  Limits: 1..8 levels, B 1..64, G <= 256, Nloc <= 2^20."""
    return _g.ga_loc_target(featmap_sizes, strides, anchor_scale, gt_bboxes, gt_counts, center_ratio, ignore_ratio)


def ga_shape_target(approxs, squares, valid_flags, gt_bboxes, gt_counts, img_shapes, pos_iou_thr=0.7, neg_iou_thr=0.3,
                    min_pos_iou=0.3, num=256, pos_fraction=0.5, neg_pos_ub=-1, allowed_border=0, keys=None, seed=0,
                    gt_max_assign_all=True, sampling=True):
    """Shape targets of a Guided Anchoring head (mmdetection v1's ``ga_shape_target`` with ``ApproxMaxIoUAssigner``).

    ``approxs``: (Nloc, A, 4) float32, the ``A <= 16`` approximating anchors of every location (``anchor_pyramid``'s
    rows of a generator with ``A`` base anchors, viewed); ``squares``: (Nloc, 4), the location's square anchor;
    ``valid_flags``: uint8 (Nloc*A,) or (B, Nloc*A), or None; ``img_shapes``: CUDA int32 (B, 2) of (h, w).  A location
    takes part if one of its approxs is flagged valid and, with ``allowed_border >= 0``, inside the image by
    :func:`anchor_target`'s rule.  Its overlap with a ground truth is the maximum IoU over all ``A`` approxs; on those
    overlaps the assignment is :func:`assign_max_iou`'s and the sampling :func:`sample_assigned`'s (``sampling=False``:
    every positive and every negative).  The (9 Nloc) x G IoU matrix never exists in memory.

    Returns ``bbox_anchors`` (B, Nloc, 4) (the square), ``bbox_gts`` (B, Nloc, 4) (the assigned ground truth) and
    ``bbox_weights`` (B, Nloc, 4) (1), all float32, set on sampled positives and 0 elsewhere; ``num_pos``, ``num_neg``
    (B,) int32; ``assigned_gt_inds`` (B, Nloc) int32 and ``max_overlaps`` (B, Nloc) float32.  Five launches, six with
    ``gt_max_assign_all=False``."""
    return _g.ga_shape_target(approxs, squares, valid_flags, gt_bboxes, gt_counts, img_shapes, pos_iou_thr,
                              neg_iou_thr, min_pos_iou, gt_max_assign_all, num, pos_fraction, neg_pos_ub,
                              allowed_border, keys, seed, sampling)


def guided_anchors(shape_preds, squares, loc_preds=None, loc_filter_thr=None, anchoring_means=ANCHORING_MEANS,
                   anchoring_stds=ANCHORING_STDS):
    """The learned anchors of a whole pyramid and batch in one launch (``GuidedAnchorHead.get_anchors``).

    ``shape_preds[l]``: (B, 2, H_l, W_l) = (dw, dh), float32 / bfloat16 / float16, NCHW-contiguous or channels_last;
    ``squares``: (Nloc, 4) float32.  ``anchors`` (B, Nloc, 4) float32 is :func:`delta2bbox` of the square with deltas
    ``(0, 0, dw, dh)``, the anchoring means / stds and ``wh_ratio_clip=1e-6``.  ``loc_mask`` (B, Nloc) uint8 is all
    ones, or with ``loc_preds[l]`` (B, 1, H_l, W_l) and ``loc_filter_thr`` in (0, 1) it is ``logit >=
    float32(log(thr / (1 - thr)))`` — the comparison of mmdetection's ``sigmoid(logit) >= thr`` made on the logit.
    Both outputs feed :func:`anchor_target` / :func:`anchor_target_all`, which take (B, N, 4) anchors."""
    return _g.guided_anchors(shape_preds, squares, loc_preds, loc_filter_thr, anchoring_means, anchoring_stds)


class GALossFunction(torch.autograd.Function):
    """One autograd node for all levels and both losses: ``apply(meta, L, avg, loc_targets, loc_weights, bbox_anchors,
    bbox_gts, bbox_weights, *loc_preds, *shape_preds)`` with ``meta = (loc_avg_factor, gamma, alpha, beta, eps, means,
    stds)`` and ``avg`` the shape divisor.  Targets get no gradient."""

    @staticmethod
    def forward(ctx, meta, L, avg, loc_targets, loc_weights, bbox_anchors, bbox_gts, bbox_weights, *heads):
        losses, norm = _g.ga_loss_fwd(heads[:L], heads[L:], loc_targets, loc_weights, bbox_anchors, bbox_gts,
                                      bbox_weights, meta[0], avg, *meta[1:])
        ctx.save_for_backward(loc_targets, loc_weights, bbox_anchors, bbox_gts, bbox_weights, *heads)
        ctx.meta, ctx.L, ctx.norm = meta, L, norm
        return losses

    @staticmethod
    def backward(ctx, g):
        targets, heads = ctx.saved_tensors[:5], ctx.saved_tensors[5:]
        L = ctx.L
        g = g.to(torch.float32).contiguous()
        dloc, dshape = _g.ga_loss_bwd(heads[:L], heads[L:], *targets, g, ctx.norm, *ctx.meta[1:])
        return (None,) * 8 + tuple(dloc) + tuple(dshape)


def ga_loss(loc_preds, shape_preds, loc_targets, loc_weights, bbox_anchors, bbox_gts, bbox_weights, loc_avg_factor,
            shape_avg_factor, gamma=2.0, alpha=0.25, beta=0.2, eps=1e-3, anchoring_means=ANCHORING_MEANS,
            anchoring_stds=ANCHORING_STDS):
    """Location and shape loss of a Guided Anchoring head over all levels (``GuidedAnchorHead.loss_loc_single`` /
    ``loss_shape_single``).

    ``loc_preds[l]``: (B, 1, H_l, W_l) logits, ``shape_preds[l]``: (B, 2, H_l, W_l) = (dw, dh); float32 / bfloat16 /
    float16 (one dtype per call), NCHW-contiguous or channels_last (levels may differ), read in place.  Targets are
    :func:`ga_loc_target`'s and :func:`ga_shape_target`'s.  ``shape_avg_factor``: as :func:`anchor_head_loss`'s
    ``avg_factor`` (a number, CUDA int32 tensors, or a tuple of two).

    ``loss_loc`` is the sigmoid focal loss of the location map with the float weights, summed and divided by
    ``loc_avg_factor``; a location of weight 0 is never evaluated.  ``loss_shape`` is mmdetection's
    ``bounded_iou_loss`` (``beta``, ``eps``) between ``delta2bbox(bbox_anchors, (0, 0, dw, dh), means, stds,
    wh_ratio_clip=1e-6)`` and ``bbox_gts`` on the rows with ``bbox_weights[..., 0] > 0``, every term weighted, summed
    and divided by the factor; only the ``dw`` / ``dh`` terms reach ``shape_preds``, the ``dx`` / ``dy`` terms add to
    the value.  Other rows never have their ``shape_preds`` read and get gradient exactly 0.

    Returns ``losses`` (2,) float32 = [loss_loc, loss_shape]; its backward gives every head output a gradient of its
    own shape, dtype and strides.  Forward is two launches, backward one; sums are fp64 in an order fixed by the
    shapes."""
    loc_preds, shape_preds = list(loc_preds), list(shape_preds)
    if len(loc_preds) != len(shape_preds):
        raise ValueError("%d loc_preds, %d shape_preds" % (len(loc_preds), len(shape_preds)))
    meta = (loc_avg_factor, gamma, alpha, beta, eps, tuple(anchoring_means), tuple(anchoring_stds))
    return GALossFunction.apply(meta, len(loc_preds), shape_avg_factor, loc_targets, loc_weights, bbox_anchors, bbox_gts,
                                bbox_weights, *loc_preds, *shape_preds)


def ga_rpn_proposals(cls_scores, bbox_preds, anchors, loc_mask, img_shapes, nms_pre=2000, nms_post=2000, max_num=2000,
                     nms_thr=0.7, min_bbox_size=0, target_means=(0, 0, 0, 0), target_stds=(1, 1, 1, 1)):
    """RPN proposals from guided anchors (mmdetection v1's ``GARPNHead.get_bboxes`` for a whole batch) in four launches.

    ``cls_scores[l]``: (B, 1, H_l, W_l) logits, ``bbox_preds[l]``: (B, 4, H_l, W_l) deltas — one anchor per location, as
    GA-RPN has — float32 or bfloat16, any strides; ``anchors`` (B, Nloc, 4) float32 and ``loc_mask`` (B, Nloc) uint8 as
    :func:`guided_anchors` returns them; ``img_shapes``: CUDA int32 (B, 2) of (h, w).  This is :func:`rpn_proposals`'
    pipeline — per-level top-``nms_pre`` by logit, decode, clip, ``min_bbox_size``, NMS, the first ``nms_post``
    survivors, then the ``max_num`` best of the image — with the anchors of the image and with masked-out locations
    absent: a level sends the ``min(nms_pre, locations in)`` highest of its locations that are in.  Returns the same
    three outputs with the same padding rules: ``proposals`` (B, max_num, 5), ``anchor_idx`` (B, max_num) int64
    (location of the pyramid; -1 on unused rows) and ``counts`` (B,) int32, 0 for an image whose mask is empty.  With
    anchors shared by the images and a mask of ones the outputs equal :func:`rpn_proposals`' bit for bit.  No host
    synchronisation; limits are :func:`rpn_proposals`' (``nms_pre``, or a level's locations when it is 0, at most 4096;
    ``max_num`` at most 8192).  ``nms_across_levels`` is not supported."""
    return _g.ga_rpn_proposals(cls_scores, bbox_preds, anchors, loc_mask, img_shapes, nms_pre, nms_post, max_num,
                               nms_thr, min_bbox_size, target_means, target_stds)
