"""Host wrappers of the single-stage head kernels (csrc/dense_detect.hip), written in the vocabulary of
``_args.py``: every shape, dtype and limit is checked here, before any launch (ValueError) — shapes,
limits and scalars first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated
here, the library allocates nothing and never synchronises, so every call can be captured in a graph.

Like ``detect_ops.py`` and ``target_ops.py`` these live beside ``ops.py`` rather than in it;
``tests/test_gpu_dense_detect.py`` puts THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, batch, f4, integer, nms_config, number, on_device, tensor
from .ops import _aligned_ws, _clip, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)
from .target_ops import _boxes, _gt, _thresholds, _valid

F32 = torch.float32


def _levels(level_shapes, num_anchors, num_classes):
    """[(H, W)] -> the level table with shapes only (strides of NCHW-contiguous tensors), A, C."""
    L = len(level_shapes)
    if not 1 <= L <= _lib.DENSE_MAX_LEVELS:
        raise ValueError("a dense head has 1..%d levels, got %d" % (_lib.DENSE_MAX_LEVELS, L))
    A, C = integer(num_anchors, "num_anchors", 1), integer(num_classes, "num_classes", 1, _lib.DET_MAX_CLASSES - 1)
    arr = (_lib.DenseLevel * L)()
    for l, (H, W) in enumerate(level_shapes):
        H, W = integer(H, "level %d height" % l, 1), integer(W, "level %d width" % l, 1)
        arr[l].H, arr[l].W = H, W
        arr[l].cls_strides[:] = [A * C * H * W, H * W, W, 1]
        arr[l].reg_strides[:] = [4 * A * H * W, H * W, W, 1]
    return arr, L, A, C


def _config(dtype, A, C, nms_pre, max_per_img, score_thr, nms_thr, means, stds, wh_ratio_clip, nms=None):
    """-> (tdn_dense_config, soft); ``soft`` is None on the greedy path, else ``nms``' tdn_soft_nms_config."""
    cfg = _lib.DenseConfig()
    cfg.dtype, cfg.num_anchors, cfg.num_classes = CODES[dtype], A, C
    cfg.nms_pre = integer(nms_pre, "nms_pre", 0, _lib.NMS_SEG_MAX)
    cfg.max_num = integer(max_per_img, "max_per_img", 1, _lib.RPN_MAX_NUM)
    cfg.score_thr = number(score_thr, "score_thr")
    cfg.nms_thr, soft = nms_config(nms, nms_thr)
    cfg.means, cfg.stds = f4(means, "target_means"), f4(stds, "target_stds")
    cfg.wh_ratio_clip = _clip(wh_ratio_clip)
    return cfg, soft


def _kept(arr, L, B, A, C, nms_pre):
    """K = the dense rows per image, checked against the row limits of the selection."""
    K = 0
    for l in range(L):
        n = arr[l].H * arr[l].W * A
        if B * n * C >= 1 << 31:
            raise ValueError("level %d holds %d logits: a level tensor must have fewer than 2^31 elements"
                             % (l, B * n * C))
        K += nms_pre if 0 < nms_pre < n else n
    if B * K > _lib.DET_MAX_ROWS:
        raise ValueError("B * K = %d dense rows (max %d): lower nms_pre" % (B * K, _lib.DET_MAX_ROWS))
    if B * C * min(B * K, _lib.NMS_SEG_MAX) >= 1 << 31:
        raise ValueError("B * C * min(B * K, %d) = %d segment rows: the workspace is indexed with 31 bits"
                         % (_lib.NMS_SEG_MAX, B * C * min(B * K, _lib.NMS_SEG_MAX)))
    return K


def anchor_head_detections_plan(level_shapes, num_imgs, num_anchors, num_classes, nms_pre):
    """What ``anchor_head_detections`` would launch for levels of ``level_shapes`` = [(H, W)] (tdn_dense_detections_plan,
    host only): a dict of K (dense rows per image), rows (B * K), anchors (per image), launches, key_workgroups (the grid
    of the class-maximum launch), selecting (levels with more than nms_pre anchors), key_words (of the workspace) and
    kept (k_l per level)."""
    arr, L, A, C = _levels(level_shapes, num_anchors, num_classes)
    B = batch(int(num_imgs))
    cfg, _ = _config(F32, A, C, nms_pre, 1, 0.0, 0.5, (0, 0, 0, 0), (1, 1, 1, 1), 16 / 1000)
    _kept(arr, L, B, A, C, cfg.nms_pre)
    out = (ctypes.c_int32 * 16)()
    if _lib.load().tdn_dense_detections_plan(arr, L, B, ctypes.byref(cfg), out) != 0:
        raise ValueError("anchor_head_detections_plan: %s" % _lib.load().tdn_last_error().decode())
    return {"K": out[0], "rows": out[1], "anchors": out[2], "launches": out[3], "key_workgroups": out[4],
            "selecting": out[5], "key_words": out[6], "kept": list(out[8:8 + L])}


def anchor_head_detections(cls_scores, bbox_preds, anchors, img_shapes, scale_factors, nms_pre, score_thr, nms_thr,
                           max_per_img, target_means, target_stds, wh_ratio_clip, nms=None):
    """Sigmoid scores, decode, per-level top-nms_pre, per-class NMS and per-image top-k of a single-stage head's outputs
    (tdn_dense_detections; with a soft ``nms`` tdn_dense_detections_soft).  Returns (dets, labels, anchor_idx, counts, dense_scores, dense_boxes, batch_idx,
    dense_anchor_idx, row_idx)."""
    L = len(cls_scores)
    if not (1 <= L <= _lib.DENSE_MAX_LEVELS) or len(bbox_preds) != L:
        raise ValueError("anchor_head_detections takes 1..%d levels with one cls_score / bbox_pred each"
                         % _lib.DENSE_MAX_LEVELS)
    first = tensor(bbox_preds[0], "bbox_preds[0]", tuple(CODES), ("B", "4A", "H", "W"), contiguous=False)
    B, dtype = batch(first[0]), bbox_preds[0].dtype
    if first[1] == 0 or first[1] % 4:
        raise ValueError("bbox_preds[0] must have 4A channels with A >= 1, got %d" % first[1])
    A = first[1] // 4
    AC = tensor(cls_scores[0], "cls_scores[0]", dtype, (B, "A*C", first[2], first[3]), contiguous=False)[1]
    if AC == 0 or AC % A:
        raise ValueError("cls_scores[0] must have A*C channels with A = %d and C >= 1, got %d" % (A, AC))
    C = AC // A
    if not 1 <= C <= _lib.DET_MAX_CLASSES - 1:
        raise ValueError("C = %d classes: must be in 1..%d" % (C, _lib.DET_MAX_CLASSES - 1))
    cfg, soft = _config(dtype, A, C, nms_pre, max_per_img, score_thr, nms_thr, target_means, target_stds, wh_ratio_clip,
                        nms)
    arr = (_lib.DenseLevel * L)()
    named, sizes = [], []
    for l, (c, d) in enumerate(zip(cls_scores, bbox_preds)):
        cn, dn = "cls_scores[%d]" % l, "bbox_preds[%d]" % l
        _, _, H, W = tensor(d, dn, dtype, (B, 4 * A, "H", "W"), contiguous=False) if l else first
        tensor(c, cn, dtype, (B, A * C, H, W), contiguous=False)
        named += [(cn, c), (dn, d)]
        sizes.append(H * W * A)
        v = arr[l]
        v.cls, v.reg = c.data_ptr(), d.data_ptr()
        v.cls_strides[:] = list(c.stride())
        v.reg_strides[:] = list(d.stride())
        v.H, v.W = H, W
    if torch.is_tensor(anchors):                     # the concatenated pyramid
        tensor(anchors, "anchors", F32, (sum(sizes), 4))
        named.append(("anchors", anchors))
        off = 0
        for l, n in enumerate(sizes):
            arr[l].anchors = anchors.data_ptr() + 16 * off
            off += n
    else:
        if len(anchors) != L:
            raise ValueError("anchors must be one (N, 4) tensor or one tensor per level")
        for l, (a, n) in enumerate(zip(anchors, sizes)):
            tensor(a, "anchors[%d]" % l, F32, (n, 4))
            named.append(("anchors[%d]" % l, a))
            arr[l].anchors = a.data_ptr()
    tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    scale_t = None
    if torch.is_tensor(scale_factors):              # or None, or a positive number
        tensor(scale_factors, "scale_factors", F32, (B,))
        scale_t = scale_factors
    elif scale_factors is not None:
        cfg.scale_factor = number(scale_factors, "scale_factors", positive=True)
    K = _kept(arr, L, B, A, C, cfg.nms_pre)
    on_device(named + [("img_shapes", img_shapes), ("scale_factors", scale_t)])
    dev = cls_scores[0].device
    lib = _lib.load()
    query = lib.tdn_dense_detections_soft_workspace_bytes if soft else lib.tdn_dense_detections_workspace_bytes
    nbytes = _lib.ws_bytes(query(arr, L, B, ctypes.byref(cfg)), "anchor_head_detections")
    M = cfg.max_num
    dense_scores = torch.empty(B * K, C + 1, dtype=F32, device=dev)
    dense_boxes = torch.empty(B * K, 4, dtype=F32, device=dev)
    batch_idx = torch.empty(B * K, dtype=torch.int32, device=dev)
    dense_anchor_idx = torch.empty(B * K, dtype=torch.int64, device=dev)
    dets = torch.empty(B, M, 5, dtype=F32, device=dev)
    labels = torch.empty(B, M, dtype=torch.int64, device=dev)
    row_idx = torch.empty(B, M, dtype=torch.int64, device=dev)
    anchor_idx = torch.empty(B, M, dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    outs = (_ptr(dense_scores), _ptr(dense_boxes), _ptr(batch_idx), _ptr(dense_anchor_idx), _ptr(dets), _ptr(labels),
            _ptr(row_idx), _ptr(anchor_idx), _ptr(counts), wp, nbytes, _lib.stream_ptr())
    if soft:
        _lib.check(lib.tdn_dense_detections_soft(arr, L, B, _ptr(img_shapes), _ptr(scale_t), ctypes.byref(cfg),
                                                 ctypes.byref(soft), *outs), "tdn_dense_detections_soft")
    else:
        _lib.check(lib.tdn_dense_detections(arr, L, B, _ptr(img_shapes), _ptr(scale_t), ctypes.byref(cfg), *outs),
                   "tdn_dense_detections")
    return dets, labels, anchor_idx, counts, dense_scores, dense_boxes, batch_idx, dense_anchor_idx, row_idx


def anchor_target_all(anchors, valid_flags, gt_bboxes, gt_labels, gt_counts, img_shapes, pos_iou_thr, neg_iou_thr,
                      min_pos_iou, gt_max_assign_all, allowed_border, means, stds):
    """Unsampled, class-labelled anchor targets (tdn_anchor_target_all).  Returns (labels, label_weights, bbox_targets,
    bbox_weights, num_pos, num_neg, assigned)."""
    B, G = _gt(gt_bboxes, gt_counts)
    N, stride = _boxes(anchors, B, "anchors")
    if N < 1:
        raise ValueError("anchors must hold at least one box")
    valid_flags, vstride = _valid(valid_flags, B, N, "valid_flags")
    if gt_labels is not None:
        tensor(gt_labels, "gt_labels", torch.int64, (B, G))
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    cfg.means, cfg.stds = f4(means, "target_means"), f4(stds, "target_stds")
    cfg.allowed_border = int(allowed_border)
    if cfg.allowed_border >= 0 or img_shapes is not None:
        tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    on_device([("anchors", anchors), ("valid_flags", valid_flags), ("gt_bboxes", gt_bboxes), ("gt_labels", gt_labels),
               ("gt_counts", gt_counts), ("img_shapes", img_shapes)])
    dev = anchors.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_anchor_target_all_workspace_bytes(B, N, G), "anchor_target_all")
    labels = torch.empty(B, N, dtype=torch.int64, device=dev)
    label_weights = torch.empty(B, N, dtype=F32, device=dev)
    bbox_targets = torch.empty(B, N, 4, dtype=F32, device=dev)
    bbox_weights = torch.empty(B, N, 4, dtype=F32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    assigned = torch.empty(B, N, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_anchor_target_all(_ptr(anchors), stride, _ptr(valid_flags), vstride, _ptr(gt_bboxes),
                                         _ptr(gt_labels), _ptr(gt_counts), _ptr(img_shapes), B, N, G, ctypes.byref(cfg),
                                         _ptr(labels), _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights),
                                         _ptr(num_pos), _ptr(num_neg), _ptr(assigned), wp, nbytes, _lib.stream_ptr()),
               "tdn_anchor_target_all")
    return labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, assigned
