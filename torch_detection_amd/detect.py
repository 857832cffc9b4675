"""Test-time detections: the last stage of a two-stage detector (HIP kernels of csrc/detect.hip; DESIGN.md §4f has the
specification, tests/detect_ref.py restates it).

``bbox_head_detections`` turns the box head's ``(R, C)`` class logits and ``(R, 4C)`` deltas into per-image detections
in five kernel launches for any batch size, class count and RoI count: softmax and decode, one segment per (image,
class) with its candidates in score order, the segmented NMS of ``batched_nms``, and a per-image top-k.
``multiclass_nms`` is the same pipeline from dense boxes and scores (four launches) — the last stage of a single-stage
test path as well.  Nothing synchronises with the host, so both can be captured in a graph; outputs have fixed shapes
and are a pure function of the inputs.
"""
from . import detect_ops as _d

__all__ = ["multiclass_nms", "bbox_head_detections"]


def multiclass_nms(multi_bboxes, multi_scores, batch_idx, num_imgs, score_thr=0.05, nms_thr=0.5, max_num=100,
                   nms=None):
    """Per-class NMS and per-image top-k.

    ``multi_bboxes``: (N, 4(C-1)) float32 class-specific boxes (class ``c`` reads columns ``4(c-1)..``) or (N, 4)
    class-agnostic; ``multi_scores``: (N, C) float32, column 0 is background and never a candidate; ``batch_idx``: (N,)
    int32 / int64 image of each row, or ``None`` for one image — rows whose index is outside ``[0, num_imgs)`` are
    ignored (the -1 padding of ``rois_from_proposals``), and an image's rows may lie anywhere.

    Candidates of (image, class ``c >= 1``) are the image's rows with ``score > score_thr`` (strictly); each such
    segment is ordered by (score desc, row asc) and goes through greedy NMS (``iou > nms_thr``, '+1' areas) exactly as
    ``batched_nms``; per image the best ``min(max_num, survivors)`` by (score desc, class asc, row asc) are kept, always
    in that order.  Returns ``dets`` (B, max_num, 5) float32 = [x1, y1, x2, y2, score], ``labels`` (B, max_num) int64
    (``c - 1``), ``row_idx`` (B, max_num) int64 (the source row) and ``counts`` (B,) int32; unused rows are 0 / -1 / -1.
    A segment holds at most 4096 candidates: an image with a longer one gets ``counts[b] = -1`` and empty rows.  NaN
    scores are unsupported.  Limits: ``num_imgs`` 1..64, C 2..1024, N <= 2^18, ``max_num`` 1..8192.

    ``nms``: ``None`` (greedy NMS at ``nms_thr``), ``dict(type='nms', iou_thr=t)`` (the same at ``t``) or
    ``dict(type='soft_nms', iou_thr=0.5, min_score=0.001, method='linear', sigma=0.5)`` (``method`` 'linear', 'gaussian'
    or 'naive'): soft-NMS per (image, class), ``dets[..., 4]`` is then the decayed score and the order is
    by it.  Giving ``nms`` together with a ``nms_thr`` other than 0.5 is refused."""
    return _d.multiclass_nms(multi_bboxes, multi_scores, batch_idx, num_imgs, score_thr, nms_thr, max_num, nms)


def bbox_head_detections(rois, cls_score, bbox_pred, img_shapes, scale_factors=None, score_thr=0.05, nms_thr=0.5,
                         max_per_img=100, target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2),
                         wh_ratio_clip=16 / 1000, return_dense=False, nms=None):
    """Detections from the box head's outputs (mmdetection's ``get_det_bboxes`` for a whole batch).

    ``rois``: (R, 5) float32 = (batch_idx, x1, y1, x2, y2) as ``roi_align`` takes them (rows with an index outside
    ``[0, B)`` are ignored); ``cls_score``: (R, C) softmax logits, class 0 background; ``bbox_pred``: (R, 4C) deltas,
    column block ``4c..`` for class ``c``, or (R, 4) class-agnostic — float32 / bfloat16 / float16, one dtype per call;
    ``img_shapes``: CUDA int32 (B, 2) of (h, w); ``scale_factors``: ``None``, a positive number or a CUDA float32 (B,).

    Scores are the softmax of ``bbox_head_loss`` operation for operation (fp64 row sum in a fixed order, one fp32
    division per class); boxes are ``delta2bbox`` against ``rois[:, 1:]`` clipped to the image's ``img_shapes`` row,
    then divided by the image's scale factor when one is given; then :func:`multiclass_nms` with ``batch_idx =
    rois[:, 0]``.  Returns ``(dets, labels, row_idx, counts)`` as :func:`multiclass_nms`; with ``return_dense=True``
    also the (R, C) float32 scores and the (R, 4(C-1)) or (R, 4) float32 boxes the selection read (rows of ignored RoIs
    are 0).  ``nms``: as :func:`multiclass_nms` takes it.  Limits: those of :func:`multiclass_nms`, R <= 2^18."""
    out = _d.bbox_head_detections(rois, cls_score, bbox_pred, img_shapes, scale_factors, score_thr, nms_thr, max_per_img,
                                  target_means, target_stds, wh_ratio_clip, nms)
    return out if return_dense else out[:4]
