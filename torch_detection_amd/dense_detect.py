"""Single-stage (RetinaNet-style) dense anchor heads: test-time detections and training targets (HIP kernels of
csrc/dense_detect.hip; DESIGN.md §4l has the specification, tests/dense_detect_ref.py restates it).

``anchor_head_detections`` turns the head's per-level ``(B, A*C, H, W)`` class logits and ``(B, 4A, H, W)`` deltas into
per-image detections in seven kernel launches for any batch size, number of levels and class count.
``anchor_target_all`` is ``anchor_target`` without sampling and with the ground truths' classes as labels: what a
focal-loss head trains on, in the shapes ``anchor_head_loss`` reads.  Nothing synchronises with the host, so both can
be captured in a graph; outputs have fixed shapes and are a pure function of the inputs.
"""
from . import dense_detect_ops as _d

__all__ = ["anchor_head_detections", "anchor_head_detections_plan", "anchor_target_all"]

anchor_head_detections_plan = _d.anchor_head_detections_plan


def anchor_head_detections(cls_scores, bbox_preds, anchors, img_shapes, scale_factors=None, nms_pre=1000,
                           score_thr=0.05, nms_thr=0.5, max_per_img=100, target_means=(0, 0, 0, 0),
                           target_stds=(1, 1, 1, 1), wh_ratio_clip=16 / 1000, return_dense=False, nms=None):
    """Detections from a sigmoid anchor head's outputs (mmdetection's ``AnchorHead.get_bboxes`` for a whole batch).

    ``cls_scores[l]``: (B, A*C, H_l, W_l) logits, class channel ``a*C + c``; ``bbox_preds[l]``: (B, 4A, H_l, W_l)
    deltas, channel ``4a + j`` — exactly what ``anchor_head_loss`` takes; float32 / bfloat16 / float16 (one dtype per
    call), read in place through their strides (NCHW-contiguous or channels_last, levels may differ).  ``anchors``: a
    per-level list of (H_l*W_l*A, 4) float32 in (y, x, a) order, or their concatenation.  ``img_shapes``: CUDA int32
    (B, 2) of (h, w); ``scale_factors``: ``None``, a positive number or a CUDA float32 (B,).

    Per (image, level) the key of an anchor is the maximum of its C logits; a level with more than ``nms_pre > 0``
    anchors keeps the ``nms_pre`` first by (key desc, anchor asc), any other level all of them.  The kept anchors, in
    ascending anchor order, become dense rows: scores ``1 / (1 + exp(-x))`` behind a zero background column, boxes
    ``delta2bbox`` of the anchor clipped to the image and divided by its scale factor.  Then :func:`multiclass_nms`.
    Returns ``dets`` (B, max_per_img, 5) float32, ``labels`` (B, max_per_img) int64 (class ``c``), ``anchor_idx``
    (B, max_per_img) int64 (row of the concatenated pyramid; -1 on unused rows) and ``counts`` (B,) int32 (-1 for an
    image with more than 4096 candidates in one class); with ``return_dense=True`` also ``dense_scores`` (B*K, C+1),
    ``dense_boxes`` (B*K, 4), ``batch_idx`` (B*K,) int32, ``dense_anchor_idx`` (B*K,) int64 and ``row_idx``
    (B, max_per_img) int64: ``multiclass_nms(dense_boxes, dense_scores, batch_idx, B, ...)`` reproduces the first
    outputs bit for bit.  Limits: 1..8 levels, B 1..64, C 1..1023, ``nms_pre`` 0..4096, B*K <= 2^18, ``max_per_img``
    1..8192.  NaN logits are unsupported.  ``nms``: as :func:`multiclass_nms` takes it (soft-NMS: one launch fewer)."""
    out = _d.anchor_head_detections(cls_scores, bbox_preds, anchors, img_shapes, scale_factors, nms_pre, score_thr,
                                    nms_thr, max_per_img, target_means, target_stds, wh_ratio_clip, nms)
    return out if return_dense else out[:4]


def anchor_target_all(anchors, valid_flags, gt_bboxes, gt_labels, gt_counts, img_shapes, pos_iou_thr=0.5,
                      neg_iou_thr=0.4, min_pos_iou=0.0, allowed_border=-1, target_means=(0, 0, 0, 0),
                      target_stds=(1, 1, 1, 1), gt_max_assign_all=True):
    """Training targets of a focal-loss anchor head: :func:`anchor_target`'s assignment (valid flags, ``allowed_border``
    against ``img_shapes``, the six steps of ``assign_max_iou``), no sampling.

    ``gt_labels``: (B, G) int64 with values in 1..C, or ``None`` (every positive gets 1).  Returns ``labels`` (B, N)
    int64 (the assigned ground truth's label on positives, else 0), ``label_weights`` (B, N) float32 (1 on positives
    and negatives, 0 on ignored and non-participating anchors), ``bbox_targets`` / ``bbox_weights`` (B, N, 4) float32
    (``bbox2delta`` / 1 on positives, else 0), ``num_pos`` / ``num_neg`` (B,) int32 and ``assigned_gt_inds`` (B, N)
    int32.  ``num_pos`` feeds ``anchor_head_loss(..., avg_factor=num_pos)`` directly."""
    return _d.anchor_target_all(anchors, valid_flags, gt_bboxes, gt_labels, gt_counts, img_shapes, pos_iou_thr,
                                neg_iou_thr, min_pos_iou, gt_max_assign_all, allowed_border, target_means, target_stds)
