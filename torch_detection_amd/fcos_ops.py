"""Host wrappers of the FCOS kernels (csrc/fcos.hip), written in the vocabulary of ``_args.py``
(DESIGN.md §5e): every shape, dtype, layout and limit is checked here, before any launch (ValueError) — shapes, limits
and scalars first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated here,
the library allocates nothing and never synchronises, so every call can be captured in a graph.

Like ``dense_detect_ops.py`` these live beside ``ops.py`` rather than in it; ``tests/test_gpu_fcos.py`` puts THIS module
under the guard of ``tests/guard_util.py``.
"""
import ctypes
import math

import torch

from . import _lib
from ._args import CODES, batch, integer, nms_config, number, on_device, tensor
from .loss_ops import _layout
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)
from .target_ops import _gt

F32 = torch.float32
MAX_STRIDE = 1 << 15
MAX_EXTENT = 1 << 24


def _pyramid(featmap_sizes, strides, regress_ranges=None):
    """[(H, W)], [stride] (, [(lo, hi)]) -> (the level table, L, N = points per image)."""
    featmap_sizes, strides = list(featmap_sizes), list(strides)
    L = len(featmap_sizes)
    if not 1 <= L <= _lib.FCOS_MAX_LEVELS:
        raise ValueError("an FCOS pyramid has 1..%d levels, got %d" % (_lib.FCOS_MAX_LEVELS, L))
    if len(strides) != L:
        raise ValueError("%d featmap_sizes but %d strides" % (L, len(strides)))
    if regress_ranges is not None:
        regress_ranges = list(regress_ranges)
        if len(regress_ranges) != L:
            raise ValueError("%d featmap_sizes but %d regress_ranges" % (L, len(regress_ranges)))
    arr = (_lib.FcosLevel * L)()
    N = 0
    for l, (size, s) in enumerate(zip(featmap_sizes, strides)):
        if len(size) != 2:
            raise ValueError("featmap_sizes[%d] must be (H, W)" % l)
        H, W = integer(size[0], "level %d height" % l, 1), integer(size[1], "level %d width" % l, 1)
        s = integer(s, "strides[%d]" % l, 1, MAX_STRIDE)
        if H * s >= MAX_EXTENT or W * s >= MAX_EXTENT:
            raise ValueError("level %d spans %d x %d pixels: must stay below 2^24" % (l, H * s, W * s))
        arr[l].H, arr[l].W, arr[l].stride = H, W, s
        if regress_ranges is not None:
            try:
                lo, hi = (float(v) for v in regress_ranges[l])
            except (TypeError, ValueError):
                raise ValueError("regress_ranges[%d] must be a pair (lo, hi)" % l) from None
            if math.isnan(lo) or math.isnan(hi) or lo > hi or math.isinf(lo):
                raise ValueError("regress_ranges[%d] must be finite lo <= hi (hi may be inf), got (%r, %r)"
                                 % (l, lo, hi))
            arr[l].lo, arr[l].hi = lo, hi
        N += H * W
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%d points per image (max %d)" % (N, _lib.TARGET_MAX_BOXES))
    return arr, L, N


def fcos_points(featmap_sizes, strides, device=None):
    """(N, 4) float32 rows (x, y, stride, level) of the pyramid's points, level-major (tdn_fcos_points)."""
    arr, L, N = _pyramid(featmap_sizes, strides)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("fcos_points: device must be a CUDA device")
    points = torch.empty(N, 4, dtype=F32, device=dev)
    on_device([("points", points)])
    _lib.check(_lib.load().tdn_fcos_points(arr, L, _ptr(points), _lib.stream_ptr()), "tdn_fcos_points")
    return points


def fcos_target(featmap_sizes, strides, regress_ranges, gt_bboxes, gt_labels, gt_counts, center_sample_radius):
    """Point targets (tdn_fcos_target).  Returns (labels, bbox_targets, assigned_gt_inds, num_pos)."""
    arr, L, N = _pyramid(featmap_sizes, strides, regress_ranges)
    B, G = _gt(gt_bboxes, gt_counts)
    if gt_labels is not None:
        tensor(gt_labels, "gt_labels", torch.int64, (B, G))
    radius = 0.0 if center_sample_radius is None else number(center_sample_radius, "center_sample_radius",
                                                             positive=True)
    on_device([("gt_bboxes", gt_bboxes), ("gt_labels", gt_labels), ("gt_counts", gt_counts)])
    dev = gt_bboxes.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_fcos_target_workspace_bytes(arr, L, B, G), "fcos_target")
    labels = torch.empty(B, N, dtype=torch.int64, device=dev)
    bbox_targets = torch.empty(B, N, 4, dtype=F32, device=dev)
    assigned = torch.empty(B, N, dtype=torch.int32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_fcos_target(arr, L, B, _ptr(gt_bboxes), _ptr(gt_labels), _ptr(gt_counts), G, radius,
                                   _ptr(labels), _ptr(bbox_targets), _ptr(assigned), _ptr(num_pos), wp, nbytes,
                                   _lib.stream_ptr()), "tdn_fcos_target")
    return labels, bbox_targets, assigned, num_pos


def _heads(cls_scores, bbox_preds, centernesses, strides, who, max_classes):
    """Checks of the head outputs of one call -> (the level table, L, B, C, N, dtype, (name, tensor) pairs)."""
    cls_scores, bbox_preds, centernesses = list(cls_scores), list(bbox_preds), list(centernesses)
    L = len(cls_scores)
    if not 1 <= L <= _lib.FCOS_MAX_LEVELS or len(bbox_preds) != L or len(centernesses) != L:
        raise ValueError("%s takes 1..%d levels with one cls_score, one bbox_pred and one centerness each"
                         % (who, _lib.FCOS_MAX_LEVELS))
    B, C, _, _ = tensor(cls_scores[0], "cls_scores[0]", tuple(CODES), ("B", "C", "H", "W"), contiguous=False)
    batch(B)
    if not 1 <= C <= max_classes:
        raise ValueError("C = %d classes: must be in 1..%d" % (C, max_classes))
    dtype = cls_scores[0].dtype
    sizes, flags, named = [], [], []
    for l, (c, r, z) in enumerate(zip(cls_scores, bbox_preds, centernesses)):
        cn, rn, zn = "cls_scores[%d]" % l, "bbox_preds[%d]" % l, "centernesses[%d]" % l
        _, _, H, W = tensor(c, cn, dtype, (B, C, "H", "W"), contiguous=False)
        if H < 1 or W < 1:
            raise ValueError("level %d: empty cls_score %s" % (l, tuple(c.shape)))
        tensor(r, rn, dtype, (B, 4, H, W), contiguous=False)
        tensor(z, zn, dtype, (B, 1, H, W), contiguous=False)
        if B * max(C, 4) * H * W >= 1 << 31:
            raise ValueError("level %d holds 2^31 elements or more" % l)
        _layout(z, zn)                                   # one channel: both layouts are the same memory
        sizes.append((H, W))
        flags.append((_layout(c, cn), _layout(r, rn)))
        named += [(cn, c), (rn, r), (zn, z)]
    arr, _, N = _pyramid(sizes, [1] * L if strides is None else strides)
    for l, (c, r, z) in enumerate(zip(cls_scores, bbox_preds, centernesses)):
        arr[l].cls, arr[l].reg, arr[l].ctr = c.data_ptr(), r.data_ptr(), z.data_ptr()
        arr[l].cls_nhwc, arr[l].reg_nhwc = flags[l]
    return arr, L, B, C, N, dtype, named


def _scales(scales, L):
    if scales is not None:
        tensor(scales, "scales", F32, (L,))
    return scales


def _loss_setup(cls_scores, bbox_preds, centernesses, labels, bbox_targets, scales, loss_type, gamma, alpha, eps):
    arr, L, B, C, N, dtype, named = _heads(cls_scores, bbox_preds, centernesses, None, "fcos_loss",
                                           _lib.LOSS_MAX_CLASSES)
    cfg = _lib.FcosLossConfig()
    cfg.dtype, cfg.num_classes = CODES[dtype], C
    if loss_type not in ("iou", "giou"):
        raise ValueError("loss_type must be 'iou' or 'giou', got %r" % (loss_type,))
    cfg.giou = int(loss_type == "giou")
    cfg.gamma, cfg.alpha, cfg.eps = number(gamma, "gamma"), number(alpha, "alpha"), number(eps, "eps")
    if cfg.gamma < 0 or not 0 <= cfg.alpha <= 1:
        raise ValueError("focal loss needs gamma >= 0 and alpha in [0, 1]")
    if not 0 < cfg.eps < 1:
        raise ValueError("eps must be in (0, 1), got %r" % eps)
    what = "(the levels hold N = %d points per image)" % N
    for t, name, dt, shape in ((labels, "labels", torch.int64, (B, N)),
                               (bbox_targets, "bbox_targets", F32, (B, N, 4))):
        try:
            tensor(t, name, dt, shape)
        except ValueError as e:
            raise ValueError("%s %s" % (e, what)) from None
    _scales(scales, L)
    named += [("labels", labels), ("bbox_targets", bbox_targets), ("scales", scales)]
    return arr, L, B, cfg, named


def _like(t):
    """An uninitialised tensor of ``t``'s shape, dtype and strides (its memory is one flat array either way)."""
    flat = torch.empty(t.numel(), dtype=t.dtype, device=t.device)
    return flat.as_strided(tuple(t.shape), tuple(t.stride()))


def fcos_loss_fwd(cls_scores, bbox_preds, centernesses, labels, bbox_targets, scales, loss_type, gamma, alpha, eps):
    """-> (losses (3,) float32 = [loss_cls, loss_bbox, loss_centerness], the divisors (3,) float32 and the per-level
    scale sums (L,) float64 (None without ``scales``) that the backward call takes)."""
    arr, L, B, cfg, named = _loss_setup(cls_scores, bbox_preds, centernesses, labels, bbox_targets, scales, loss_type,
                                        gamma, alpha, eps)
    on_device(named)
    dev = labels.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_fcos_loss_workspace_bytes(arr, L, B, ctypes.byref(cfg)), "fcos_loss")
    losses = torch.empty(3, dtype=F32, device=dev)
    norm = torch.empty(3, dtype=F32, device=dev)
    scale_sums = torch.empty(L, dtype=torch.float64, device=dev) if scales is not None else None
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_fcos_loss_fwd(arr, L, B, ctypes.byref(cfg), _ptr(labels), _ptr(bbox_targets), _ptr(scales),
                                     _ptr(losses), _ptr(norm), _ptr(scale_sums), wp, nbytes, _lib.stream_ptr()),
               "tdn_fcos_loss_fwd")
    return losses, norm, scale_sums


def fcos_loss_bwd(cls_scores, bbox_preds, centernesses, labels, bbox_targets, scales, g, norm, scale_sums, loss_type,
                  gamma, alpha, eps):
    """Gradients of ``g . losses``: one tensor per head output with its shape, dtype and strides, and (L,) float32 for
    ``scales`` (None without).  ``g``: (3,) float32; ``norm`` / ``scale_sums``: what the forward call returned."""
    arr, L, B, cfg, named = _loss_setup(cls_scores, bbox_preds, centernesses, labels, bbox_targets, scales, loss_type,
                                        gamma, alpha, eps)
    tensor(g, "g", F32, (3,))
    tensor(norm, "norm", F32, (3,))
    if scales is not None:
        tensor(scale_sums, "scale_sums", torch.float64, (L,))
    elif scale_sums is not None:
        raise ValueError("scale_sums goes with scales")
    on_device(named + [("g", g), ("norm", norm), ("scale_sums", scale_sums)])
    dcls = [_like(t) for t in cls_scores]
    dreg = [_like(t) for t in bbox_preds]
    dctr = [_like(t) for t in centernesses]
    dscales = torch.empty(L, dtype=F32, device=labels.device) if scales is not None else None
    for l in range(L):
        arr[l].dcls, arr[l].dreg, arr[l].dctr = dcls[l].data_ptr(), dreg[l].data_ptr(), dctr[l].data_ptr()
    _lib.check(_lib.load().tdn_fcos_loss_bwd(arr, L, B, ctypes.byref(cfg), _ptr(labels), _ptr(bbox_targets),
                                             _ptr(scales), _ptr(g), _ptr(norm), _ptr(scale_sums), _ptr(dscales),
                                             _lib.stream_ptr()), "tdn_fcos_loss_bwd")
    return dcls, dreg, dctr, dscales


def _det_config(dtype, C, nms_pre, max_per_img, score_thr, nms_thr, nms=None):
    """-> (tdn_fcos_det_config, soft); ``soft`` is None on the greedy path, else ``nms``' tdn_soft_nms_config."""
    cfg = _lib.FcosDetConfig()
    cfg.dtype, cfg.num_classes = CODES[dtype], C
    cfg.nms_pre = integer(nms_pre, "nms_pre", 0, _lib.NMS_SEG_MAX)
    cfg.max_num = integer(max_per_img, "max_per_img", 1, _lib.RPN_MAX_NUM)
    cfg.score_thr = number(score_thr, "score_thr")
    cfg.nms_thr, soft = nms_config(nms, nms_thr)
    return cfg, soft


def _kept(arr, L, B, C, nms_pre):
    """K = the dense rows per image, checked against the row limits of the selection."""
    K = 0
    for l in range(L):
        n = arr[l].H * arr[l].W
        if B * n * max(C, 4) >= 1 << 31:
            raise ValueError("level %d holds 2^31 elements or more" % l)
        K += nms_pre if 0 < nms_pre < n else n
    if B * K > _lib.DET_MAX_ROWS:
        raise ValueError("B * K = %d dense rows (max %d): lower nms_pre" % (B * K, _lib.DET_MAX_ROWS))
    if B * C * min(B * K, _lib.NMS_SEG_MAX) >= 1 << 31:
        raise ValueError("B * C * min(B * K, %d) = %d segment rows: the workspace is indexed with 31 bits"
                         % (_lib.NMS_SEG_MAX, B * C * min(B * K, _lib.NMS_SEG_MAX)))
    return K


def fcos_detections_plan(featmap_sizes, num_imgs, num_classes, nms_pre):
    """What ``fcos_detections`` would launch for levels of ``featmap_sizes`` = [(H, W)] (tdn_fcos_detections_plan, host
    only): a dict of K (dense rows per image), rows (B * K), points (per image), launches, key_workgroups, selecting
    (levels with more than nms_pre points), key_words (of the workspace) and kept (k_l per level).  The key launch's
    grid is that of channels_last class logits."""
    arr, L, _ = _pyramid(featmap_sizes, [1] * len(list(featmap_sizes)))
    B = batch(int(num_imgs))
    C = integer(num_classes, "num_classes", 1, _lib.DET_MAX_CLASSES - 1)
    for l in range(L):
        arr[l].cls_nhwc = 1
    cfg, _ = _det_config(F32, C, nms_pre, 1, 0.0, 0.5)
    _kept(arr, L, B, C, cfg.nms_pre)
    out = (ctypes.c_int32 * 16)()
    if _lib.load().tdn_fcos_detections_plan(arr, L, B, ctypes.byref(cfg), out) != 0:
        raise ValueError("fcos_detections_plan: %s" % _lib.load().tdn_last_error().decode())
    return {"K": out[0], "rows": out[1], "points": out[2], "launches": out[3], "key_workgroups": out[4],
            "selecting": out[5], "key_words": out[6], "kept": list(out[8:8 + L])}


def fcos_detections(cls_scores, bbox_preds, centernesses, strides, img_shapes, scales, scale_factors, nms_pre,
                    score_thr, nms_thr, max_per_img, nms=None):
    """Centre-ness weighted sigmoid scores, point +- distance decode, per-level top-nms_pre, per-class NMS and per-image
    top-k of an FCOS head's outputs (tdn_fcos_detections; with a soft ``nms`` tdn_fcos_detections_soft).  Returns (dets, labels, point_idx, counts, dense_scores,
    dense_boxes, batch_idx, dense_point_idx, row_idx)."""
    arr, L, B, C, N, dtype, named = _heads(cls_scores, bbox_preds, centernesses, list(strides), "fcos_detections",
                                           _lib.DET_MAX_CLASSES - 1)
    cfg, soft = _det_config(dtype, C, nms_pre, max_per_img, score_thr, nms_thr, nms)
    tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    _scales(scales, L)
    scale_t = None
    if torch.is_tensor(scale_factors):              # or None, or a positive number
        tensor(scale_factors, "scale_factors", F32, (B,))
        scale_t = scale_factors
    elif scale_factors is not None:
        cfg.scale_factor = number(scale_factors, "scale_factors", positive=True)
    K = _kept(arr, L, B, C, cfg.nms_pre)
    on_device(named + [("img_shapes", img_shapes), ("scales", scales), ("scale_factors", scale_t)])
    dev = cls_scores[0].device
    lib = _lib.load()
    query = lib.tdn_fcos_detections_soft_workspace_bytes if soft else lib.tdn_fcos_detections_workspace_bytes
    nbytes = _lib.ws_bytes(query(arr, L, B, ctypes.byref(cfg)), "fcos_detections")
    M = cfg.max_num
    dense_scores = torch.empty(B * K, C + 1, dtype=F32, device=dev)
    dense_boxes = torch.empty(B * K, 4, dtype=F32, device=dev)
    batch_idx = torch.empty(B * K, dtype=torch.int32, device=dev)
    dense_point_idx = torch.empty(B * K, dtype=torch.int64, device=dev)
    dets = torch.empty(B, M, 5, dtype=F32, device=dev)
    labels = torch.empty(B, M, dtype=torch.int64, device=dev)
    row_idx = torch.empty(B, M, dtype=torch.int64, device=dev)
    point_idx = torch.empty(B, M, dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    outs = (_ptr(dense_scores), _ptr(dense_boxes), _ptr(batch_idx), _ptr(dense_point_idx), _ptr(dets), _ptr(labels),
            _ptr(row_idx), _ptr(point_idx), _ptr(counts), wp, nbytes, _lib.stream_ptr())
    if soft:
        _lib.check(lib.tdn_fcos_detections_soft(arr, L, B, _ptr(img_shapes), _ptr(scale_t), _ptr(scales),
                                                ctypes.byref(cfg), ctypes.byref(soft), *outs), "tdn_fcos_detections_soft")
    else:
        _lib.check(lib.tdn_fcos_detections(arr, L, B, _ptr(img_shapes), _ptr(scale_t), _ptr(scales), ctypes.byref(cfg),
                                           *outs), "tdn_fcos_detections")
    return dets, labels, point_idx, counts, dense_scores, dense_boxes, batch_idx, dense_point_idx, row_idx
