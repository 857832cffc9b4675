"""Host wrappers of the test-time detection kernels (csrc/detect.hip): every shape, dtype and limit is
checked here, before any launch (ValueError) — shapes and limits first, so that those refusals need no GPU, the device
last; outputs and the workspace are allocated here, the library allocates nothing and never synchronises, so every call
can be captured in a graph.

Like ``loss_ops.py`` and ``target_ops.py`` these live beside ``ops.py`` rather than in it; ``tests/test_gpu_detect.py``
puts THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from .loss_ops import _CODES, _chk_cuda, _number
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)


def _limits(N, C, B, max_num, score_thr, nms_thr, what):
    """The limits both entry points share -> (max_num, score_thr, nms_thr)."""
    if not 2 <= C <= _lib.DET_MAX_CLASSES:
        raise ValueError("%s has %d columns: C must be in 2..%d (column 0 is background)"
                         % (what, C, _lib.DET_MAX_CLASSES))
    if N > _lib.DET_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (N, _lib.DET_MAX_ROWS))
    if not 1 <= B <= 64:
        raise ValueError("the number of images must be in 1..64, got %d" % B)
    max_num = int(max_num)
    if not 1 <= max_num <= _lib.RPN_MAX_NUM:
        raise ValueError("max_num must be in 1..%d, got %d" % (_lib.RPN_MAX_NUM, max_num))
    score_thr, nms_thr = _number(score_thr, "score_thr"), _number(nms_thr, "nms_thr")
    if B * (C - 1) * min(N, _lib.NMS_SEG_MAX) >= 1 << 31:
        raise ValueError("B * (C - 1) * min(N, %d) = %d segment rows: the workspace is indexed with 31 bits"
                         % (_lib.NMS_SEG_MAX, B * (C - 1) * min(N, _lib.NMS_SEG_MAX)))
    return max_num, score_thr, nms_thr


def _outputs(B, max_num, dev):
    return (torch.empty(B, max_num, 5, dtype=torch.float32, device=dev),
            torch.empty(B, max_num, dtype=torch.int64, device=dev),
            torch.empty(B, max_num, dtype=torch.int64, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev))


def multiclass_nms(multi_bboxes, multi_scores, batch_idx, num_imgs, score_thr, nms_thr, max_num):
    """Per-class NMS and per-image top-k of dense boxes and scores (tdn_multiclass_nms).  Returns (dets (B, max_num, 5)
    float32, labels (B, max_num) int64, row_idx (B, max_num) int64, counts (B,) int32)."""
    if not torch.is_tensor(multi_scores) or multi_scores.dtype != torch.float32 or multi_scores.dim() != 2 or \
            not multi_scores.is_contiguous():
        raise ValueError("multi_scores must be a contiguous float32 (N, C) tensor")
    N, C = multi_scores.shape
    B = int(num_imgs)
    max_num, score_thr, nms_thr = _limits(N, C, B, max_num, score_thr, nms_thr, "multi_scores")
    if not torch.is_tensor(multi_bboxes) or multi_bboxes.dtype != torch.float32 or multi_bboxes.dim() != 2 or \
            not multi_bboxes.is_contiguous() or multi_bboxes.shape[0] != N or \
            multi_bboxes.shape[1] not in (4, 4 * (C - 1)):
        raise ValueError("multi_bboxes must be a contiguous float32 (%d, %d) or (%d, 4) tensor" % (N, 4 * (C - 1), N))
    if batch_idx is None:
        if B != 1:
            raise ValueError("batch_idx=None means one image, got num_imgs=%d" % B)
    elif not torch.is_tensor(batch_idx) or batch_idx.dtype not in (torch.int32, torch.int64) or \
            tuple(batch_idx.shape) != (N,) or not batch_idx.is_contiguous():
        raise ValueError("batch_idx must be a contiguous int32 or int64 (%d,) tensor, or None" % N)
    _chk_cuda([("multi_scores", multi_scores), ("multi_bboxes", multi_bboxes), ("batch_idx", batch_idx)])
    dev = multi_scores.device
    dets, labels, row_idx, counts = _outputs(B, max_num, dev)
    lib = _lib.load()
    nbytes = lib.tdn_multiclass_nms_workspace_bytes(N, C, B)
    if nbytes < 0:
        raise ValueError("multiclass_nms: %s" % lib.tdn_last_error().decode())
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_multiclass_nms(_ptr(multi_bboxes), multi_bboxes.shape[1], _ptr(multi_scores), _ptr(batch_idx),
                                      batch_idx.element_size() if batch_idx is not None else 0, N, C, B, score_thr,
                                      nms_thr, max_num, _ptr(dets), _ptr(labels), _ptr(row_idx), _ptr(counts), wp,
                                      nbytes, _lib.stream_ptr()), "tdn_multiclass_nms")
    return dets, labels, row_idx, counts


def _f4(vals, name):
    try:
        vals = [float(v) for v in vals]
    except TypeError:
        vals = []
    if len(vals) != 4 or any(v != v or v in (float("inf"), float("-inf")) for v in vals):
        raise ValueError("%s must have 4 finite entries" % name)
    return (ctypes.c_float * 4)(*vals)


def bbox_head_detections(rois, cls_score, bbox_pred, img_shapes, scale_factors, score_thr, nms_thr, max_per_img,
                         target_means, target_stds, wh_ratio_clip):
    """Softmax, decode, per-class NMS and per-image top-k of the box head's outputs (tdn_bbox_detections).  Returns
    (dets, labels, row_idx, counts) as ``multiclass_nms`` and the dense (R, C) float32 scores and (R, 4(C-1)) or (R, 4)
    float32 boxes the selection read."""
    if not torch.is_tensor(rois) or rois.dtype != torch.float32 or rois.dim() != 2 or rois.shape[1] != 5 or \
            not rois.is_contiguous():
        raise ValueError("rois must be a contiguous float32 (R, 5) tensor of (batch_idx, x1, y1, x2, y2)")
    R = rois.shape[0]
    if not torch.is_tensor(cls_score) or cls_score.dim() != 2 or cls_score.dtype not in _CODES or \
            not cls_score.is_contiguous() or cls_score.shape[0] != R:
        raise ValueError("cls_score must be a contiguous (%d, C) float32 / bfloat16 / float16 tensor" % R)
    C = cls_score.shape[1]
    if not torch.is_tensor(img_shapes) or img_shapes.dtype != torch.int32 or img_shapes.dim() != 2 or \
            img_shapes.shape[1] != 2 or not img_shapes.is_contiguous():
        raise ValueError("img_shapes must be a contiguous int32 (B, 2) tensor of (h, w)")
    B = img_shapes.shape[0]
    max_num, score_thr, nms_thr = _limits(R, C, B, max_per_img, score_thr, nms_thr, "cls_score")
    if not torch.is_tensor(bbox_pred) or bbox_pred.dim() != 2 or bbox_pred.dtype != cls_score.dtype or \
            not bbox_pred.is_contiguous() or bbox_pred.shape[0] != R or bbox_pred.shape[1] not in (4, 4 * C):
        raise ValueError("bbox_pred must be a contiguous (%d, %d) or (%d, 4) tensor of cls_score's dtype" %
                         (R, 4 * C, R))
    scale_t, scale_v = None, 0.0
    if torch.is_tensor(scale_factors):
        if scale_factors.dtype != torch.float32 or tuple(scale_factors.shape) != (B,) or \
                not scale_factors.is_contiguous():
            raise ValueError("scale_factors must be None, a positive number or a contiguous float32 (%d,) tensor" % B)
        scale_t = scale_factors
    elif scale_factors is not None:
        scale_v = _number(scale_factors, "scale_factors", positive=True)
    means, stds = _f4(target_means, "target_means"), _f4(target_stds, "target_stds")
    clip = _number(wh_ratio_clip, "wh_ratio_clip")
    if not 0.0 < clip < 1.0:
        raise ValueError("wh_ratio_clip must be in (0, 1), got %r" % clip)
    _chk_cuda([("rois", rois), ("cls_score", cls_score), ("bbox_pred", bbox_pred), ("img_shapes", img_shapes),
               ("scale_factors", scale_t)])
    dev = rois.device
    dets, labels, row_idx, counts = _outputs(B, max_num, dev)
    scores = torch.empty(R, C, dtype=torch.float32, device=dev)
    boxes = torch.empty(R, 4 if bbox_pred.shape[1] == 4 else 4 * (C - 1), dtype=torch.float32, device=dev)
    lib = _lib.load()
    nbytes = lib.tdn_bbox_detections_workspace_bytes(R, C, B)
    if nbytes < 0:
        raise ValueError("bbox_head_detections: %s" % lib.tdn_last_error().decode())
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_bbox_detections(_ptr(rois), _ptr(cls_score), _ptr(bbox_pred), _CODES[cls_score.dtype], R, C,
                                       bbox_pred.shape[1], B, _ptr(img_shapes), _ptr(scale_t), scale_v, means, stds,
                                       clip, score_thr, nms_thr, max_num, _ptr(scores), _ptr(boxes), _ptr(dets),
                                       _ptr(labels), _ptr(row_idx), _ptr(counts), wp, nbytes, _lib.stream_ptr()),
               "tdn_bbox_detections")
    return dets, labels, row_idx, counts, scores, boxes
