"""Host wrappers of the test-time detection kernels (csrc/detect.hip), written in the vocabulary of
``_args.py``: every shape, dtype and limit is checked here, before any launch (ValueError) — shapes and
limits first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated here, the
library allocates nothing and never synchronises, so every call can be captured in a graph.

Like ``loss_ops.py`` and ``target_ops.py`` these live beside ``ops.py`` rather than in it; ``tests/test_gpu_detect.py``
puts THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, batch, f4, integer, nms_config, number, on_device, tensor
from .ops import _aligned_ws, _clip, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)


def _limits(N, C, B, max_num, score_thr, nms_thr, what, nms=None):
    """The limits both entry points share -> (max_num, score_thr, nms_thr, soft); ``soft`` is None on the greedy path,
    else the ``tdn_soft_nms_config`` of ``nms`` (``_args.nms_config``)."""
    if not 2 <= C <= _lib.DET_MAX_CLASSES:
        raise ValueError("%s has %d columns: C must be in 2..%d (column 0 is background)"
                         % (what, C, _lib.DET_MAX_CLASSES))
    if N > _lib.DET_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (N, _lib.DET_MAX_ROWS))
    batch(B)
    max_num = integer(max_num, "max_num", 1, _lib.RPN_MAX_NUM)
    score_thr = number(score_thr, "score_thr")
    nms_thr, soft = nms_config(nms, nms_thr)
    if B * (C - 1) * min(N, _lib.NMS_SEG_MAX) >= 1 << 31:
        raise ValueError("B * (C - 1) * min(N, %d) = %d segment rows: the workspace is indexed with 31 bits"
                         % (_lib.NMS_SEG_MAX, B * (C - 1) * min(N, _lib.NMS_SEG_MAX)))
    return max_num, score_thr, nms_thr, soft


def _outputs(B, max_num, dev):
    return (torch.empty(B, max_num, 5, dtype=torch.float32, device=dev),
            torch.empty(B, max_num, dtype=torch.int64, device=dev),
            torch.empty(B, max_num, dtype=torch.int64, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev))


def multiclass_nms(multi_bboxes, multi_scores, batch_idx, num_imgs, score_thr, nms_thr, max_num, nms=None):
    """Per-class NMS and per-image top-k of dense boxes and scores (tdn_multiclass_nms; with a soft ``nms``
    tdn_multiclass_nms_soft).  Returns (dets (B, max_num, 5) float32, labels (B, max_num) int64, row_idx (B, max_num)
    int64, counts (B,) int32)."""
    N, C = tensor(multi_scores, "multi_scores", torch.float32, ("N", "C"))
    B = int(num_imgs)
    max_num, score_thr, nms_thr, soft = _limits(N, C, B, max_num, score_thr, nms_thr, "multi_scores", nms)
    cols = tensor(multi_bboxes, "multi_bboxes", torch.float32, (N, (4 * (C - 1), 4)))[1]
    if batch_idx is not None:
        tensor(batch_idx, "batch_idx", (torch.int32, torch.int64), (N,))
    elif B != 1:
        raise ValueError("batch_idx=None means one image, got num_imgs=%d" % B)
    on_device([("multi_scores", multi_scores), ("multi_bboxes", multi_bboxes), ("batch_idx", batch_idx)])
    dev = multi_scores.device
    lib = _lib.load()
    query = lib.tdn_multiclass_nms_soft_workspace_bytes if soft else lib.tdn_multiclass_nms_workspace_bytes
    nbytes = _lib.ws_bytes(query(N, C, B), "multiclass_nms")
    dets, labels, row_idx, counts = _outputs(B, max_num, dev)
    ws, wp = _aligned_ws(nbytes, dev)
    if soft:
        _lib.check(lib.tdn_multiclass_nms_soft(_ptr(multi_bboxes), cols, _ptr(multi_scores), _ptr(batch_idx),
                                               batch_idx.element_size() if batch_idx is not None else 0, N, C, B,
                                               score_thr, ctypes.byref(soft), max_num, _ptr(dets), _ptr(labels),
                                               _ptr(row_idx), _ptr(counts), wp, nbytes, _lib.stream_ptr()),
                   "tdn_multiclass_nms_soft")
        return dets, labels, row_idx, counts
    _lib.check(lib.tdn_multiclass_nms(_ptr(multi_bboxes), cols, _ptr(multi_scores), _ptr(batch_idx),
                                      batch_idx.element_size() if batch_idx is not None else 0, N, C, B, score_thr,
                                      nms_thr, max_num, _ptr(dets), _ptr(labels), _ptr(row_idx), _ptr(counts), wp,
                                      nbytes, _lib.stream_ptr()), "tdn_multiclass_nms")
    return dets, labels, row_idx, counts


def bbox_head_detections(rois, cls_score, bbox_pred, img_shapes, scale_factors, score_thr, nms_thr, max_per_img,
                         target_means, target_stds, wh_ratio_clip, nms=None):
    """Softmax, decode, per-class NMS and per-image top-k of the box head's outputs (tdn_bbox_detections; with a soft
    ``nms`` tdn_bbox_detections_soft).  Returns
    (dets, labels, row_idx, counts) as ``multiclass_nms`` and the dense (R, C) float32 scores and (R, 4(C-1)) or (R, 4)
    float32 boxes the selection read."""
    R = tensor(rois, "rois", torch.float32, ("R", 5))[0]                  # (batch_idx, x1, y1, x2, y2)
    C = tensor(cls_score, "cls_score", tuple(CODES), (R, "C"))[1]
    B = tensor(img_shapes, "img_shapes", torch.int32, ("B", 2))[0]          # (h, w)
    max_num, score_thr, nms_thr, soft = _limits(R, C, B, max_per_img, score_thr, nms_thr, "cls_score", nms)
    cols = tensor(bbox_pred, "bbox_pred", cls_score.dtype, (R, (4 * C, 4)))[1]
    scale_t, scale_v = None, 0.0
    if torch.is_tensor(scale_factors):              # or None, or a positive number
        tensor(scale_factors, "scale_factors", torch.float32, (B,))
        scale_t = scale_factors
    elif scale_factors is not None:
        scale_v = number(scale_factors, "scale_factors", positive=True)
    means, stds = f4(target_means, "target_means"), f4(target_stds, "target_stds")
    clip = _clip(wh_ratio_clip)
    on_device([("rois", rois), ("cls_score", cls_score), ("bbox_pred", bbox_pred), ("img_shapes", img_shapes),
               ("scale_factors", scale_t)])
    dev = rois.device
    lib = _lib.load()
    query = lib.tdn_bbox_detections_soft_workspace_bytes if soft else lib.tdn_bbox_detections_workspace_bytes
    nbytes = _lib.ws_bytes(query(R, C, B), "bbox_head_detections")
    dets, labels, row_idx, counts = _outputs(B, max_num, dev)
    scores = torch.empty(R, C, dtype=torch.float32, device=dev)
    boxes = torch.empty(R, 4 if cols == 4 else 4 * (C - 1), dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    fn, what = (lib.tdn_bbox_detections_soft, "tdn_bbox_detections_soft") if soft else \
        (lib.tdn_bbox_detections, "tdn_bbox_detections")
    _lib.check(fn(_ptr(rois), _ptr(cls_score), _ptr(bbox_pred), CODES[cls_score.dtype], R, C, cols, B, _ptr(img_shapes),
                  _ptr(scale_t), scale_v, means, stds, clip, score_thr, ctypes.byref(soft) if soft else nms_thr, max_num,
                  _ptr(scores), _ptr(boxes), _ptr(dets), _ptr(labels), _ptr(row_idx), _ptr(counts), wp, nbytes,
                  _lib.stream_ptr()), what)
    return dets, labels, row_idx, counts, scores, boxes
