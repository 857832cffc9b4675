"""Host wrappers of the Cascade R-CNN kernels (the refine section of csrc/detect.hip and its stage-averaged first launch;
DESIGN.md §4q), written in the vocabulary of ``_args.py``: every shape, dtype and limit is checked here,
before any launch (ValueError) — shapes and limits first, so that those refusals need no GPU, the device last; outputs
and the workspace are allocated here, the library allocates nothing and never synchronises, so every call can be
captured in a graph.  ``tests/test_gpu_cascade.py`` puts THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, batch, f4, integer, number, on_device, tensor
from .detect_ops import _limits
from .ops import _aligned_ws, _clip, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)


def refine_ws_bytes(R, B):
    """TDN_REFINE_WS_BYTES of include/tdn.h: one int32 per (chunk of REFINE_CHUNK rows, image), 256-aligned."""
    return (-(-R // _lib.REFINE_CHUNK) * B * 4 + 255) & ~255


def refine_bboxes(rois, bbox_pred, img_shapes, labels, cls_score, pos_assigned_gt_inds, gt_bboxes, max_per_img,
                  target_means, target_stds, wh_ratio_clip):
    """Every RoI decoded by the deltas of its class (tdn_refine_bboxes).  ``max_per_img=None``: (R, 5) float32 rois, row
    for row; ``max_per_img=P``: (proposals (B, P, 5) float32, counts (B,) int32), as ``sample_rois`` reads them."""
    R = tensor(rois, "rois", torch.float32, ("R", 5))[0]                  # (batch_idx, x1, y1, x2, y2)
    cols = tensor(bbox_pred, "bbox_pred", tuple(CODES), (R, "4C"))[1]
    B = batch(tensor(img_shapes, "img_shapes", torch.int32, ("B", 2))[0])  # (h, w)
    if (labels is None) == (cls_score is None):
        raise ValueError("exactly one of labels and cls_score must be given")
    if cls_score is not None:
        C = tensor(cls_score, "cls_score", bbox_pred.dtype, (R, "C"))[1]
        if cols not in (4, 4 * C):
            raise ValueError("bbox_pred has %d columns: neither 4 nor 4 * C = %d" % (cols, 4 * C))
    else:
        tensor(labels, "labels", torch.int64, (R,))
        if cols == 0 or cols % 4:
            raise ValueError("bbox_pred must have 4C columns with C >= 1, got %d" % cols)
        C = cols // 4
    if not 1 <= C <= _lib.DET_MAX_CLASSES:
        raise ValueError("C = %d classes: must be in 1..%d" % (C, _lib.DET_MAX_CLASSES))
    if R > _lib.DET_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (R, _lib.DET_MAX_ROWS))
    P = 0 if max_per_img is None else integer(max_per_img, "max_per_img", 1, _lib.RPN_MAX_NUM)
    G = 0
    if (pos_assigned_gt_inds is None) != (gt_bboxes is None):
        raise ValueError("pos_assigned_gt_inds and gt_bboxes go together")
    if gt_bboxes is not None:
        if not P:
            raise ValueError("pos_assigned_gt_inds / gt_bboxes drop ground truths in compacted mode only: give max_per_img")
        tensor(pos_assigned_gt_inds, "pos_assigned_gt_inds", torch.int32, (R,))
        G = tensor(gt_bboxes, "gt_bboxes", torch.float32, (B, "G", 4))[1]
        if G < 1:
            raise ValueError("gt_bboxes must hold at least one (padded) box per image")
    means, stds = f4(target_means, "target_means"), f4(target_stds, "target_stds")
    clip = _clip(wh_ratio_clip)
    on_device([("rois", rois), ("bbox_pred", bbox_pred), ("img_shapes", img_shapes), ("labels", labels),
               ("cls_score", cls_score), ("pos_assigned_gt_inds", pos_assigned_gt_inds), ("gt_bboxes", gt_bboxes)])
    dev = rois.device
    lib = _lib.load()
    out = props = counts = ws = wp = None
    nbytes = 0
    if P:
        props = torch.empty(B, P, 5, dtype=torch.float32, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        nbytes = refine_ws_bytes(R, B)
        if nbytes:
            ws, wp = _aligned_ws(nbytes, dev)
    else:
        out = torch.empty(R, 5, dtype=torch.float32, device=dev)
    _lib.check(lib.tdn_refine_bboxes(_ptr(rois), _ptr(bbox_pred), CODES[bbox_pred.dtype], R, cols, B, _ptr(img_shapes),
                                     _ptr(labels), _ptr(cls_score), C, _ptr(pos_assigned_gt_inds), _ptr(gt_bboxes), G,
                                     means, stds, clip, P, _ptr(out), _ptr(props), _ptr(counts), wp, nbytes,
                                     _lib.stream_ptr()), "tdn_refine_bboxes")
    return (props, counts) if P else out


def cascade_detections(rois, cls_scores, bbox_pred, img_shapes, scale_factors, score_thr, nms_thr, max_per_img,
                       target_means, target_stds, wh_ratio_clip, nms=None):
    """``detect_ops.bbox_head_detections`` on the mean of the stages' class logits (tdn_cascade_detections; with a soft
    ``nms`` tdn_cascade_detections_soft).  Returns
    (dets, labels, row_idx, counts) and the dense (R, C) float32 scores and (R, 4(C-1)) or (R, 4) float32 boxes."""
    if not isinstance(cls_scores, (list, tuple)) or not 1 <= len(cls_scores) <= _lib.CASCADE_MAX_STAGES:
        raise ValueError("cls_scores must be a list of 1..%d tensors" % _lib.CASCADE_MAX_STAGES)
    R = tensor(rois, "rois", torch.float32, ("R", 5))[0]                  # (batch_idx, x1, y1, x2, y2)
    C = tensor(cls_scores[0], "cls_scores[0]", tuple(CODES), (R, "C"))[1]
    dtype = cls_scores[0].dtype
    for s, x in enumerate(cls_scores[1:], 1):
        tensor(x, "cls_scores[%d]" % s, dtype, (R, C))
    B = tensor(img_shapes, "img_shapes", torch.int32, ("B", 2))[0]          # (h, w)
    max_num, score_thr, nms_thr, soft = _limits(R, C, B, max_per_img, score_thr, nms_thr, "cls_scores[0]", nms)
    cols = tensor(bbox_pred, "bbox_pred", dtype, (R, (4 * C, 4)))[1]
    scale_t, scale_v = None, 0.0
    if torch.is_tensor(scale_factors):              # or None, or a positive number
        tensor(scale_factors, "scale_factors", torch.float32, (B,))
        scale_t = scale_factors
    elif scale_factors is not None:
        scale_v = number(scale_factors, "scale_factors", positive=True)
    means, stds = f4(target_means, "target_means"), f4(target_stds, "target_stds")
    clip = _clip(wh_ratio_clip)
    on_device([("rois", rois), ("bbox_pred", bbox_pred), ("img_shapes", img_shapes), ("scale_factors", scale_t)] +
              [("cls_scores[%d]" % s, x) for s, x in enumerate(cls_scores)])
    dev = rois.device
    lib = _lib.load()
    query = lib.tdn_cascade_detections_soft_workspace_bytes if soft else lib.tdn_bbox_detections_workspace_bytes
    nbytes = _lib.ws_bytes(query(R, C, B), "cascade_detections")
    dets = torch.empty(B, max_num, 5, dtype=torch.float32, device=dev)
    labels = torch.empty(B, max_num, dtype=torch.int64, device=dev)
    row_idx = torch.empty(B, max_num, dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty(R, C, dtype=torch.float32, device=dev)
    boxes = torch.empty(R, 4 if cols == 4 else 4 * (C - 1), dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    stages = (ctypes.c_void_p * len(cls_scores))(*[x.data_ptr() for x in cls_scores])
    fn, what = (lib.tdn_cascade_detections_soft, "tdn_cascade_detections_soft") if soft else \
        (lib.tdn_cascade_detections, "tdn_cascade_detections")
    _lib.check(fn(_ptr(rois), stages, len(cls_scores), _ptr(bbox_pred), CODES[dtype], R, C, cols, B, _ptr(img_shapes),
                  _ptr(scale_t), scale_v, means, stds, clip, score_thr, ctypes.byref(soft) if soft else nms_thr, max_num,
                  _ptr(scores), _ptr(boxes), _ptr(dets), _ptr(labels), _ptr(row_idx), _ptr(counts), wp, nbytes,
                  _lib.stream_ptr()), what)
    return dets, labels, row_idx, counts, scores, boxes
