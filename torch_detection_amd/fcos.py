"""FCOS (anchor-free, centre-ness) dense head operations: the point generator, training targets, the loss and test-time
detections (HIP kernels of csrc/fcos.hip; DESIGN.md §4n has the specification, tests/fcos_ref.py restates it).

The pyramid is given as ``featmap_sizes`` = [(H_l, W_l)] and integer ``strides``; point ``i = h*W_l + w`` of level ``l``
sits at ``(x, y) = (w*s + s//2, h*s + s//2)`` and points are level-major, ``N = sum H_l*W_l``.  Nothing synchronises with
the host, so every function can be captured in a graph; outputs have fixed shapes and are a pure function of the
inputs, bit for bit from run to run.
"""
import torch

from . import fcos_ops as _f

__all__ = ["FcosLossFunction", "fcos_points", "fcos_target", "fcos_loss", "fcos_detections", "fcos_detections_plan"]

fcos_detections_plan = _f.fcos_detections_plan


def fcos_points(featmap_sizes, strides, device=None):
    """The pyramid's points as an (N, 4) float32 tensor of rows ``(x, y, stride, level)`` on ``device`` (default: the
    current CUDA device).  One launch; the other FCOS operations recompute the points and do not need this tensor."""
    return _f.fcos_points(featmap_sizes, strides, device)


def fcos_target(featmap_sizes, strides, regress_ranges, gt_bboxes, gt_labels, gt_counts, center_sample_radius=None):
    """Training targets of an FCOS head (mmdetection v1's ``FCOSHead.fcos_target`` for a whole batch).

    ``regress_ranges``: one ``(lo, hi)`` per level, ``hi`` may be ``inf``.  ``gt_bboxes``: (B, G, 4) float32 xyxy,
    ``gt_labels``: (B, G) int64 in 1..C or ``None`` (every positive gets 1), ``gt_counts``: (B,) int32, all CUDA; rows
    past ``gt_counts[b]`` are padding and never read.  For a point and a ground truth, ``l = x - x1``, ``t = y - y1``,
    ``r = x2 - x``, ``b = y2 - y``; the ground truth is a candidate if ``min(l, t, r, b) > 0`` — with
    ``center_sample_radius = rho`` the same test against the centre box ``(max(cx - rho*s, x1), max(cy - rho*s, y1),
    min(cx + rho*s, x2), min(cy + rho*s, y2))`` — and ``lo <= max(l, t, r, b) <= hi`` for the point's level.  The
    candidate of the smallest area ``(x2 - x1 + 1)*(y2 - y1 + 1)`` wins, ties go to the lowest index.

    Returns ``labels`` (B, N) int64 (0: no candidate), ``bbox_targets`` (B, N, 4) float32 (the winner's ``l, t, r, b``, or
    zeros), ``assigned_gt_inds`` (B, N) int32 (index + 1, or 0) and ``num_pos`` (B,) int32.  Everything is exact fp32 in
    the order written.  Limits: 1..8 levels, B 1..64, G <= 256, N <= 2^20."""
    return _f.fcos_target(featmap_sizes, strides, regress_ranges, gt_bboxes, gt_labels, gt_counts,
                          center_sample_radius)


class FcosLossFunction(torch.autograd.Function):
    """One autograd node for all levels and the three losses: ``apply(meta, L, has_scales, labels, bbox_targets,
    *scales, *cls_scores, *bbox_preds, *centernesses)`` with ``meta = (loss_type, gamma, alpha, eps)``.  Targets get no
    gradient."""

    @staticmethod
    def forward(ctx, meta, L, has_scales, labels, bbox_targets, *rest):
        scales = rest[0] if has_scales else None
        heads = rest[1:] if has_scales else rest
        losses, norm, scale_sums = _f.fcos_loss_fwd(heads[:L], heads[L:2 * L], heads[2 * L:], labels, bbox_targets,
                                                    scales, *meta)
        ctx.save_for_backward(labels, bbox_targets, *rest)
        ctx.meta, ctx.L, ctx.has_scales, ctx.norm, ctx.scale_sums = meta, L, has_scales, norm, scale_sums
        return losses

    @staticmethod
    def backward(ctx, g):
        labels, bbox_targets, rest = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:]
        L = ctx.L
        scales = rest[0] if ctx.has_scales else None
        heads = rest[1:] if ctx.has_scales else rest
        g = g.to(torch.float32).contiguous()
        dcls, dreg, dctr, dscales = _f.fcos_loss_bwd(heads[:L], heads[L:2 * L], heads[2 * L:], labels, bbox_targets,
                                                     scales, g, ctx.norm, ctx.scale_sums, *ctx.meta)
        return (None,) * 5 + ((dscales,) if ctx.has_scales else ()) + tuple(dcls) + tuple(dreg) + tuple(dctr)


def fcos_loss(cls_scores, bbox_preds, centernesses, labels, bbox_targets, scales=None, loss_type="iou", gamma=2.0,
              alpha=0.25, eps=1e-6):
    """Focal classification loss, centre-ness weighted IoU (or GIoU) box loss and centre-ness loss of an FCOS head over
    all levels (mmdetection v1's ``FCOSHead.loss``).

    ``cls_scores[l]``: (B, C, H_l, W_l) logits, ``bbox_preds[l]``: (B, 4, H_l, W_l) raw regression outputs in
    (l, t, r, b) order, ``centernesses[l]``: (B, 1, H_l, W_l) logits; float32 / bfloat16 / float16 (one dtype per call),
    NCHW-contiguous or channels_last (levels may differ), read in place.  ``labels`` (B, N) int64 and ``bbox_targets``
    (B, N, 4) float32 are :func:`fcos_target`'s.  ``scales``: ``None`` or a CUDA float32 (L,) tensor, the head's
    per-level ``Scale`` parameters: the predicted distances are ``exp(scales[l] * bbox_preds[l])``, the exponential is
    taken inside the kernels.

    ``loss_cls`` is :func:`anchor_head_loss`'s focal term over all B*N points divided by (positives + B);
    ``loss_bbox`` is ``-log(max(iou, eps))`` (``loss_type='iou'``) or ``1 - giou`` (``'giou'``) of the '+1' boxes spanned
    by the distances, weighted by the centre-ness target ``c* = sqrt(min(l*,r*)/max(l*,r*) * min(t*,b*)/max(t*,b*))`` and
    divided by the sum of the weights (0 without positives); ``loss_centerness`` is the sigmoid cross entropy of the
    centre-ness logit against ``c*`` over positives, divided by max(positives, 1).  Points with label 0 never have their
    ``bbox_preds`` / ``centernesses`` read and get gradient exactly 0.

    Returns ``losses`` (3,) float32 = [loss_cls, loss_bbox, loss_centerness]; its backward gives every head output a
    gradient of its own shape, dtype and strides and ``scales`` an (L,) float32 gradient.  Forward is two launches,
    backward one; sums are fp64 in an order fixed by the shapes."""
    cls_scores, bbox_preds, centernesses = list(cls_scores), list(bbox_preds), list(centernesses)
    if not len(cls_scores) == len(bbox_preds) == len(centernesses):
        raise ValueError("%d cls_scores, %d bbox_preds, %d centernesses" % (len(cls_scores), len(bbox_preds),
                                                                             len(centernesses)))
    meta = (loss_type, gamma, alpha, eps)
    sc = () if scales is None else (scales,)
    return FcosLossFunction.apply(meta, len(cls_scores), scales is not None, labels, bbox_targets, *sc, *cls_scores,
                                  *bbox_preds, *centernesses)


def fcos_detections(cls_scores, bbox_preds, centernesses, strides, img_shapes, scales=None, scale_factors=None,
                    nms_pre=1000, score_thr=0.05, nms_thr=0.5, max_per_img=100, return_dense=False, nms=None):
    """Detections from an FCOS head's outputs (mmdetection v1's ``FCOSHead.get_bboxes`` for a whole batch).

    Head outputs and ``scales`` as in :func:`fcos_loss`; ``strides``: one integer per level; ``img_shapes``: CUDA int32
    (B, 2) of (h, w); ``scale_factors``: ``None``, a positive number or a CUDA float32 (B,).

    With ``sg(v) = 1 / (1 + exp(-v))`` the key of a point is ``sg(max_c cls_c) * sg(ctr)``; a level with more than
    ``nms_pre > 0`` points keeps the ``nms_pre`` first by (key desc, point asc), any other level all of them.  The kept
    points, in ascending point order, become dense rows: scores ``sg(cls_c) * sg(ctr)`` behind a zero background column
    (``score_thr`` applies to the product), boxes ``(x - d_l, y - d_t, x + d_r, y + d_b)`` with ``d = exp(scale * reg)``,
    clipped to the image and divided by its scale factor.  Then :func:`multiclass_nms`.  Returns ``dets``
    (B, max_per_img, 5) float32, ``labels`` (B, max_per_img) int64 (class ``c``), ``point_idx`` (B, max_per_img) int64
    (row of the pyramid; -1 on unused rows) and ``counts`` (B,) int32 (-1 for an image with more than 4096 candidates in
    one class); with ``return_dense=True`` also ``dense_scores`` (B*K, C+1), ``dense_boxes`` (B*K, 4), ``batch_idx``
    (B*K,) int32, ``dense_point_idx`` (B*K,) int64 and ``row_idx`` (B, max_per_img) int64:
    ``multiclass_nms(dense_boxes, dense_scores, batch_idx, B, ...)`` reproduces the first outputs bit for bit.  Limits:
    1..8 levels, B 1..64, C 1..1023, ``nms_pre`` 0..4096, B*K <= 2^18, ``max_per_img`` 1..8192.  NaN logits are
    unsupported.  ``nms``: as :func:`multiclass_nms` takes it (soft-NMS: one launch fewer)."""
    out = _f.fcos_detections(cls_scores, bbox_preds, centernesses, strides, img_shapes, scales, scale_factors, nms_pre,
                             score_thr, nms_thr, max_per_img, nms)
    return out if return_dense else out[:4]
