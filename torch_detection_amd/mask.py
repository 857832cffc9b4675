"""The mask branch of Mask R-CNN around the mask head's convolutions (HIP kernels of csrc/mask.hip; DESIGN.md §4g has
the exact arithmetic, tests/mask_ref.py restates it): polygon mask targets for ``sample_rois``' positives, the mask loss
with its gradient, and at test time rois from the detections and the paste of the predicted masks into a canvas.

Nothing here synchronises with the host or allocates inside the library, so a training or test step that uses these
stays capturable in a graph.  The semantics follow mmdetection v1 (``mask_target``, ``FCNMaskHead.loss``,
``get_seg_masks``); the arithmetic is the project's own.
"""
import numpy as np
import torch

from . import mask_ops as _m
from .losses import _avg_tensors

__all__ = ["MaskHeadLossFunction", "pack_polygons", "mask_target", "mask_head_loss", "rois_from_detections",
           "mask_head_masks"]


def pack_polygons(gt_mask_polys, G):
    """The reference's ``gt_mask_polys`` of a batch (per image a list of instances, per instance a list of flat
    ``[x0, y0, x1, y1, ...]`` polygons of at least 6 numbers, in the network-input frame) as three CPU tensors:
    ``poly_xy`` (P, 2) float32 vertices, ``poly_offsets`` (Q+1,) int32 (polygon q owns vertices
    ``[poly_offsets[q], poly_offsets[q+1])``) and ``gt_poly_offsets`` (B, G+1) int32 (ground truth j of image b owns
    polygons ``[gt_poly_offsets[b, j], gt_poly_offsets[b, j+1])``; instances past an image's own get empty ranges).
    Plain host code: it runs once per batch in the data loader, next to the padding of ``gt_bboxes`` to G."""
    G = int(G)
    B = len(gt_mask_polys)
    if G < 0 or B < 1:
        raise ValueError("pack_polygons takes at least one image and G >= 0")
    xy, poly_offsets = [], [0]
    gt_poly_offsets = np.zeros((B, G + 1), np.int32)
    for b, instances in enumerate(gt_mask_polys):
        if len(instances) > G:
            raise ValueError("image %d has %d instances, more than G = %d" % (b, len(instances), G))
        gt_poly_offsets[b, 0] = len(poly_offsets) - 1
        for j, polys in enumerate(instances):
            for poly in polys:
                p = np.asarray(poly, np.float32).reshape(-1)
                if p.size < 6 or p.size % 2:
                    raise ValueError("image %d, instance %d: a polygon is a flat [x0, y0, x1, y1, ...] of at least 6 "
                                     "numbers, got %d" % (b, j, p.size))
                xy.append(p.reshape(-1, 2))
                poly_offsets.append(poly_offsets[-1] + p.size // 2)
            gt_poly_offsets[b, j + 1] = len(poly_offsets) - 1
        gt_poly_offsets[b, len(instances) + 1:] = len(poly_offsets) - 1
    poly_xy = np.concatenate(xy, 0) if xy else np.zeros((0, 2), np.float32)
    return (torch.from_numpy(np.ascontiguousarray(poly_xy)), torch.tensor(poly_offsets, dtype=torch.int32),
            torch.from_numpy(gt_poly_offsets))


def mask_target(rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_size=28):
    """Mask targets of ``sample_rois``' rows (or any slice of them, e.g. each image's positive block), in one launch.

    ``rois``: (R, 5) float32 = (batch_idx, x1, y1, x2, y2); ``pos_assigned_gt_inds``: (R,) int32; the polygon tensors
    are :func:`pack_polygons`' on the device.  Row r is valid iff its truncated batch index is in ``[0, B)`` and
    ``0 <= pos_assigned_gt_inds[r] < G``; an invalid row (a negative, padding) gets zeros and weight 0.  The box is
    truncated to integers, ``w = max(x2 - x1 + 1, 1)``; cell (i, j) of the M x M grid is 1 iff its centre
    ``(x1 + ((j + 0.5) w) / M, y1 + ((i + 0.5) h) / M)`` lies inside any polygon of the instance (even-odd rule per
    polygon, union across polygons).  Returns ``mask_targets`` (R, M, M) uint8 and ``mask_weights`` (R,) float32."""
    return _m.mask_target(rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_size)


class MaskHeadLossFunction(torch.autograd.Function):
    """``apply(avg_number, n_avg, mask_targets, labels, mask_weights, *avg_tensors, mask_pred)``."""

    @staticmethod
    def forward(ctx, avg_number, n_avg, mask_targets, labels, mask_weights, *rest):
        avg_ts, mask_pred = rest[:n_avg], rest[n_avg]
        avg_factor = avg_number if n_avg == 0 else tuple(avg_ts)
        loss, avg = _m.mask_head_loss_fwd(mask_pred, mask_targets, labels, mask_weights, avg_factor)
        ctx.save_for_backward(mask_targets, labels, mask_weights, mask_pred)
        ctx.n_avg, ctx.avg = n_avg, avg
        return loss

    @staticmethod
    def backward(ctx, g):
        mask_targets, labels, mask_weights, mask_pred = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        dpred = _m.mask_head_loss_bwd(mask_pred, mask_targets, labels, mask_weights, g, ctx.avg)
        return (None,) * (5 + ctx.n_avg) + (dpred,)


def mask_head_loss(mask_pred, mask_targets, labels, mask_weights, avg_factor=None):
    """Binary cross entropy of the mask head on :func:`mask_target`'s rows.  ``mask_pred``: (R, C, M, M) logits,
    float32 / bfloat16 / float16, NCHW-contiguous or channels_last, C counting the background; row r reads channel
    ``labels[r]`` (1..C-1; ``C == 1`` is class-agnostic and reads channel 0).  ``loss = sum_r w_r sum_ij l / (D M^2)``
    with ``D = avg_factor`` as :func:`bbox_head_loss` takes it, or None for the number of rows with ``w > 0`` (counted on
    the device, at least 1).  Rows with weight 0 are never read.  Returns a (1,) float32 loss; its backward gives
    ``mask_pred`` a gradient of its own shape, dtype and strides, exact zeros off the rows' channels."""
    avg_ts, _ = _avg_tensors(avg_factor)
    return MaskHeadLossFunction.apply(avg_factor if not avg_ts else None, len(avg_ts), mask_targets, labels,
                                      mask_weights, *avg_ts, mask_pred)


def rois_from_detections(dets, counts, scale_factors=None):
    """``multiclass_nms``' / ``bbox_head_detections``' padded (B, max_num, 5) detections and (B,) int32 counts ->
    (B*max_num, 5) rois (b, x1 s, y1 s, x2 s, y2 s) for the mask head's RoIAlign; ``scale_factors``: None, a positive
    number or a CUDA float32 (B,) (detections rescaled to the original image go back to the network-input frame).  Rows
    at or past ``counts[b]`` (all of them for the overflow marker -1) are (-1, 0, 0, 0, 0).  No host synchronisation."""
    return _m.rois_from_detections(dets, counts, scale_factors)


def mask_head_masks(mask_pred, dets, labels, counts, out_shape, img_shapes=None, thr=0.5, packed=False):
    """Pastes the predicted masks into a canvas (mmdetection's ``get_seg_masks`` for a whole batch, one launch).

    ``mask_pred``: (B*max_num, C, M, M) logits in the row order of :func:`rois_from_detections`; ``dets`` (B, max_num, 5)
    in the frame of the canvas, ``labels`` (B, max_num) int64 0-based foreground labels (channel ``labels + 1``, or 0
    when ``C == 1``) and ``counts`` (B,) int32 as ``multiclass_nms`` returns them; ``out_shape = (H, W)``;
    ``img_shapes``: optional CUDA int32 (B, 2) of (h, w) — pixels outside an image's own size stay 0.  Inside the
    truncated box a pixel is the bilinear sample of ``sigmoid(mask_pred)`` compared ``> thr``; everything else is 0.
    Returns (B*max_num, H, W) uint8, or with ``packed=True`` (B*max_num, H, 8*ceil(W/64)) uint8 where bit ``x % 8`` of
    byte ``x // 8`` is pixel x (``np.unpackbits(a, axis=-1, bitorder='little')[..., :W]`` unpacks it)."""
    return _m.mask_head_masks(mask_pred, dets, labels, counts, out_shape, img_shapes, thr, bool(packed))
