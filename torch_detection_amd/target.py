"""Training-target assignment and sampling for the RPN and the RoI heads (HIP kernels of csrc/target.hip, bit-exact
against tests/target_ref.py; DESIGN.md §4d has the exact spec).

The reference has no assigner (``core/__init__.py`` is an empty file); names and semantics follow the mmdetection
v0.x/v1 lineage (``MaxIoUAssigner``, ``RandomSampler``, ``anchor_target``, ``bbox_target``) on inclusive '+1' float32
xyxy boxes.  Ground truths come padded as the reference's ``bbox_pad`` (datasets/utils/bbox.py:238-256) stacks them:
``gt_bboxes`` (B, G, 4) with zero rows past ``gt_counts`` (B,) int32.  ``boxes`` / ``anchors`` are (N, 4), shared by
all images, or (B, N, 4).  Nothing here synchronises with the host: every call can be captured in a graph.
"""
from . import libra_ops as _b
from . import target_ops as _t


def assign_max_iou(boxes, gt_bboxes, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, gt_max_assign_all=True,
                   valid=None):
    """Max-IoU assignment of every box of every image.  Returns ``assigned_gt_inds`` (B, N) int32 (-1 ignored or not
    taking part, 0 negative, j + 1 ground truth j) and ``max_overlaps`` (B, N) float32.  ``valid``: uint8 (or bool), (N,) shared
    by all images or (B, N); a box whose byte is 0 does not take part.  Scalar thresholds only."""
    return _t.assign_max_iou(boxes, gt_bboxes, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all,
                             valid)


def sample_assigned(assigned_gt_inds, num, pos_fraction, neg_pos_ub=-1, keys=None, seed=0):
    """Random sampling of an assignment: per image the ``min(#pos, int(num * pos_fraction))`` positives and the
    ``min(#neg, num - pos [, int(neg_pos_ub * max(1, pos))])`` negatives with the smallest (key, index).  ``keys``:
    (B, N) int32, non-negative; None: the integer hash of (seed, image, index) of DESIGN.md §4d.  Returns ``pos_mask``,
    ``neg_mask`` (B, N) uint8 and ``num_pos``, ``num_neg`` (B,) int32."""
    return _t.sample_assigned(assigned_gt_inds, num, pos_fraction, neg_pos_ub, keys, seed)


def anchor_target(anchors, valid_flags, gt_bboxes, gt_counts, img_shapes, pos_iou_thr=0.7, neg_iou_thr=0.3,
                  min_pos_iou=0.3, num=256, pos_fraction=0.5, neg_pos_ub=-1, allowed_border=0,
                  target_means=(0, 0, 0, 0), target_stds=(1, 1, 1, 1), keys=None, seed=0, gt_max_assign_all=True):
    """RPN training targets of a batch in five launches.  ``valid_flags``: uint8 (N,) or (B, N) (images of different
    sizes share the anchors but not the flags), or None; ``img_shapes``: CUDA int32 (B, 2) of (h, w); with ``allowed_border >= 0`` an anchor takes part only
    if ``x1 >= -border, y1 >= -border, x2 < w + border, y2 < h + border``.  Returns ``labels`` (B, N) int64 (1 on
    sampled positives), ``label_weights`` (B, N) float32 (1 on sampled positives and negatives), ``bbox_targets`` and
    ``bbox_weights`` (B, N, 4) float32 (``bbox2delta`` of the anchor and its ground truth / 1 on sampled positives),
    ``num_pos``, ``num_neg`` (B,) int32 and ``assigned_gt_inds`` (B, N) int32."""
    return _t.anchor_target(anchors, valid_flags, gt_bboxes, gt_counts, img_shapes, pos_iou_thr, neg_iou_thr,
                            min_pos_iou, gt_max_assign_all, num, pos_fraction, neg_pos_ub, allowed_border,
                            target_means, target_stds, keys, seed)


def sample_assigned_iou_balanced(assigned_gt_inds, max_overlaps, num, pos_fraction, neg_pos_ub=-1, floor_thr=-1.0,
                                 floor_fraction=0.0, num_bins=3, keys=None, seed=0):
    """:func:`sample_assigned` with the negatives chosen by IoU-balanced sampling (Libra R-CNN, in the lineage of
    mmdetection v1's ``IoUBalancedNegSampler``): when an image has more negatives than it may keep, they
    are drawn evenly from ``num_bins`` bins of ``max_overlaps`` between ``floor_thr`` and the image's largest overlap,
    "k at random from a set" being the k smallest (key, index) of the set; ``floor_fraction`` of them may come from below
    ``floor_thr``.  ``max_overlaps``: (B, N) float32, as :func:`assign_max_iou` returns it.  The same four outputs."""
    return _b.sample_assigned_iou_balanced(assigned_gt_inds, max_overlaps, num, pos_fraction, neg_pos_ub, floor_thr,
                                           floor_fraction, num_bins, keys, seed)


def sample_rois(proposals, counts, gt_bboxes, gt_labels, gt_counts, pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5,
                num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True, target_means=(0, 0, 0, 0),
                target_stds=(0.1, 0.1, 0.2, 0.2), keys=None, seed=0, gt_max_assign_all=True, neg_sampler='random',
                floor_thr=-1.0, floor_fraction=0.0, num_bins=3):
    """RoI-head training samples and targets from ``rpn_proposals``' padded output (``proposals`` (B, P, 5), ``counts``
    (B,)), in five launches.  Candidates of an image: its ground truths first (``add_gt_as_proposals``), then its
    ``counts[b]`` proposals; ``gt_labels``: (B, G) int64.  Fixed shapes: image b owns rows ``[b * num, (b + 1) * num)``
    — sampled positives in ascending candidate index, then sampled negatives likewise, then padding (batch index -1,
    zeros, weight 0), which ``roi_align`` treats as invalid rows.  Returns ``rois`` (B*num, 5) = [b, x1, y1, x2, y2],
    ``labels`` (B*num,) int64, ``label_weights``, ``bbox_targets`` (B*num, 4) class-agnostic, ``bbox_weights``,
    ``pos_assigned_gt_inds`` (B*num,) int32 (-1 off the positives), ``num_pos``, ``num_neg``.
    ``neg_sampler``: ``'random'``, or ``'iou_balanced'`` with ``floor_thr`` / ``floor_fraction`` / ``num_bins``
    (:func:`sample_assigned_iou_balanced`), which replaces only the choice of the negatives."""
    if neg_sampler == 'iou_balanced':
        return _b.sample_rois_iou_balanced(proposals, counts, gt_bboxes, gt_labels, gt_counts, pos_iou_thr, neg_iou_thr,
                                           min_pos_iou, gt_max_assign_all, num, pos_fraction, neg_pos_ub,
                                           add_gt_as_proposals, target_means, target_stds, keys, seed, floor_thr,
                                           floor_fraction, num_bins)
    if neg_sampler != 'random':
        raise ValueError("neg_sampler must be 'random' or 'iou_balanced', got %r" % (neg_sampler,))
    return _t.sample_rois(proposals, counts, gt_bboxes, gt_labels, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou,
                          gt_max_assign_all, num, pos_fraction, neg_pos_ub, add_gt_as_proposals, target_means,
                          target_stds, keys, seed)
