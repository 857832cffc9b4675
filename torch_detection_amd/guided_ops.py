"""Host wrappers of the Guided Anchoring kernels (csrc/guided.hip), written in the vocabulary of
``_args.py``: every shape, dtype, layout and limit is checked here, before any launch (ValueError) —
shapes, limits and scalars first, so that those refusals need no GPU, the device last; outputs and the workspace are
allocated here, the library allocates nothing and never synchronises, so every call can be captured in a graph.

Like ``fcos_ops.py`` these live beside ``ops.py`` rather than in it; ``tests/test_gpu_guided.py`` puts THIS module under
the guard of ``tests/guard_util.py``.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._args import CODES, batch, f4, integer, number, on_device, tensor
from .loss_ops import _avg, _layout
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)
from .target_ops import _gt, _keys, _sampling, _thresholds

F32 = torch.float32
BF16 = torch.bfloat16
MAX_STRIDE = 1 << 15
MAX_EXTENT = 1 << 24


def _f32(v):
    return float(np.float32(v))


def _pyramid(featmap_sizes, strides=None):
    """[(H, W)] (, [stride]) -> (the level table, L, N = locations per image)."""
    featmap_sizes = list(featmap_sizes)
    L = len(featmap_sizes)
    if not 1 <= L <= _lib.LOSS_MAX_LEVELS:
        raise ValueError("a Guided Anchoring pyramid has 1..%d levels, got %d" % (_lib.LOSS_MAX_LEVELS, L))
    if strides is not None:
        strides = list(strides)
        if len(strides) != L:
            raise ValueError("%d featmap_sizes but %d strides" % (L, len(strides)))
    arr = (_lib.GaLevel * L)()
    N = 0
    for l, size in enumerate(featmap_sizes):
        if len(size) != 2:
            raise ValueError("featmap_sizes[%d] must be (H, W)" % l)
        H, W = integer(size[0], "level %d height" % l, 1), integer(size[1], "level %d width" % l, 1)
        arr[l].H, arr[l].W = H, W
        if strides is not None:
            s = integer(strides[l], "strides[%d]" % l, 1, MAX_STRIDE)
            if H * s >= MAX_EXTENT or W * s >= MAX_EXTENT:
                raise ValueError("level %d spans %d x %d pixels: must stay below 2^24" % (l, H * s, W * s))
            arr[l].stride = s
        N += H * W
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%d locations per image (max %d)" % (N, _lib.TARGET_MAX_BOXES))
    return arr, L, N


def _ratio(v, name):
    v = number(v, name)
    if not 0.0 <= v <= 1.0:
        raise ValueError("%s must be in [0, 1], got %r" % (name, v))
    r = (1.0 - v) / 2.0
    return _f32(r), _f32(1.0 - r)


def _level_thresholds(anchor_scale, stride0, L):
    """t_k = m^2 2^(2k-1), k = 1..L-1, m = anchor_scale * strides[0]: formed in float64, rounded once to fp32."""
    m = number(anchor_scale, "anchor_scale", positive=True) * stride0
    thr = [_f32(m * m * 2.0 ** (2 * k - 1)) for k in range(1, L)]
    if not all(math.isfinite(t) and t > 0 for t in thr):
        raise ValueError("anchor_scale %r with stride %d: a level threshold is outside fp32" % (anchor_scale, stride0))
    return thr


def ga_loc_target(featmap_sizes, strides, anchor_scale, gt_bboxes, gt_counts, center_ratio, ignore_ratio):
    """Location targets (tdn_ga_loc_target).  Returns (loc_targets, loc_weights, loc_avg_factor)."""
    arr, L, N = _pyramid(featmap_sizes, strides)
    B, G = _gt(gt_bboxes, gt_counts)
    cfg = _lib.GaLocConfig()
    for k, t in enumerate(_level_thresholds(anchor_scale, arr[0].stride, L)):
        cfg.area_thr[k] = t
    cfg.center_r, cfg.center_c = _ratio(center_ratio, "center_ratio")
    cfg.ignore_r, cfg.ignore_c = _ratio(ignore_ratio, "ignore_ratio")
    on_device([("gt_bboxes", gt_bboxes), ("gt_counts", gt_counts)])
    dev = gt_bboxes.device
    loc_targets = torch.empty(B, N, dtype=torch.int64, device=dev)
    loc_weights = torch.empty(B, N, dtype=F32, device=dev)
    _lib.check(_lib.load().tdn_ga_loc_target(arr, L, B, _ptr(gt_bboxes), _ptr(gt_counts), G, ctypes.byref(cfg),
                                             _ptr(loc_targets), _ptr(loc_weights), _lib.stream_ptr()),
               "tdn_ga_loc_target")
    return loc_targets, loc_weights, B * N / 200.0


def ga_shape_target(approxs, squares, valid_flags, gt_bboxes, gt_counts, img_shapes, pos_iou_thr, neg_iou_thr,
                    min_pos_iou, gt_max_assign_all, num, pos_fraction, neg_pos_ub, allowed_border, keys, seed,
                    sampling):
    """Shape targets (tdn_ga_shape_target).  Returns (bbox_anchors, bbox_gts, bbox_weights, num_pos, num_neg,
    assigned_gt_inds, max_overlaps)."""
    B, G = _gt(gt_bboxes, gt_counts)
    N, A, _ = tensor(approxs, "approxs", F32, ("Nloc", "A", 4))
    if not 1 <= A <= _lib.GA_MAX_APPROX:
        raise ValueError("approxs: A = %d approxs per location (1..%d)" % (A, _lib.GA_MAX_APPROX))
    if not 1 <= N <= _lib.TARGET_MAX_BOXES:
        raise ValueError("approxs: %d locations per image (1..%d)" % (N, _lib.TARGET_MAX_BOXES))
    tensor(squares, "squares", F32, (N, 4))
    vstride = 0
    if valid_flags is not None:
        shared = torch.is_tensor(valid_flags) and valid_flags.dim() == 1
        tensor(valid_flags, "valid_flags", (torch.uint8, torch.bool), (N * A,) if shared else (B, N * A))
        valid_flags, vstride = valid_flags.view(torch.uint8), (0 if shared else N * A)
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    _sampling(cfg, num, pos_fraction, neg_pos_ub, seed)
    cfg.allowed_border = int(allowed_border)
    if cfg.allowed_border >= 0 or img_shapes is not None:
        tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    _keys(keys, (B, N))
    on_device([("approxs", approxs), ("squares", squares), ("valid_flags", valid_flags), ("gt_bboxes", gt_bboxes),
               ("gt_counts", gt_counts), ("img_shapes", img_shapes), ("keys", keys)])
    dev = approxs.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_ga_shape_target_workspace_bytes(B, N, G), "ga_shape_target")
    bbox_anchors = torch.empty(B, N, 4, dtype=F32, device=dev)
    bbox_gts = torch.empty(B, N, 4, dtype=F32, device=dev)
    bbox_weights = torch.empty(B, N, 4, dtype=F32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    assigned = torch.empty(B, N, dtype=torch.int32, device=dev)
    max_overlaps = torch.empty(B, N, dtype=F32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_ga_shape_target(_ptr(approxs), A, _ptr(squares), _ptr(valid_flags), vstride, _ptr(gt_bboxes),
                                       _ptr(gt_counts), _ptr(img_shapes), B, N, G, ctypes.byref(cfg),
                                       1 if sampling else 0, _ptr(keys), _ptr(bbox_anchors), _ptr(bbox_gts),
                                       _ptr(bbox_weights), _ptr(num_pos), _ptr(num_neg), _ptr(assigned),
                                       _ptr(max_overlaps), wp, nbytes, _lib.stream_ptr()), "tdn_ga_shape_target")
    return bbox_anchors, bbox_gts, bbox_weights, num_pos, num_neg, assigned, max_overlaps


def _heads(shape_preds, loc_preds, who):
    """Checks of the head outputs of one call -> (the level table, L, B, N, dtype, (name, tensor) pairs)."""
    shape_preds = list(shape_preds)
    L = len(shape_preds)
    if not 1 <= L <= _lib.LOSS_MAX_LEVELS:
        raise ValueError("%s takes 1..%d levels, got %d" % (who, _lib.LOSS_MAX_LEVELS, L))
    if loc_preds is not None:
        loc_preds = list(loc_preds)
        if len(loc_preds) != L:
            raise ValueError("%s: %d shape_preds but %d loc_preds" % (who, L, len(loc_preds)))
    B = tensor(shape_preds[0], "shape_preds[0]", tuple(CODES), ("B", 2, "H", "W"), contiguous=False)[0]
    batch(B)
    dtype = shape_preds[0].dtype
    sizes, flags, named = [], [], []
    for l, s in enumerate(shape_preds):
        sn = "shape_preds[%d]" % l
        _, _, H, W = tensor(s, sn, dtype, (B, 2, "H", "W"), contiguous=False)
        if H < 1 or W < 1:
            raise ValueError("level %d: empty shape_pred %s" % (l, tuple(s.shape)))
        if B * 2 * H * W >= 1 << 31:
            raise ValueError("level %d holds 2^31 elements or more" % l)
        sizes.append((H, W))
        flags.append(_layout(s, sn))
        named.append((sn, s))
        if loc_preds is not None:
            ln = "loc_preds[%d]" % l
            tensor(loc_preds[l], ln, dtype, (B, 1, H, W), contiguous=False)
            _layout(loc_preds[l], ln)                       # one channel: both layouts are the same memory
            named.append((ln, loc_preds[l]))
    arr, _, N = _pyramid(sizes)
    for l, s in enumerate(shape_preds):
        arr[l].shape, arr[l].shape_nhwc = s.data_ptr(), flags[l]
        if loc_preds is not None:
            arr[l].loc = loc_preds[l].data_ptr()
    return arr, L, B, N, dtype, named


def _loc_threshold(loc_filter_thr):
    """The logit whose sigmoid is ``loc_filter_thr``: log(t / (1 - t)) in float64, rounded once to fp32."""
    t = number(loc_filter_thr, "loc_filter_thr")
    if not 0.0 < t < 1.0:
        raise ValueError("loc_filter_thr must be in (0, 1), got %r" % t)
    return _f32(math.log(t / (1.0 - t)))


def guided_anchors(shape_preds, squares, loc_preds, loc_filter_thr, means, stds):
    """The guided anchors and their mask (tdn_guided_anchors).  Returns (anchors, loc_mask)."""
    if (loc_preds is None) != (loc_filter_thr is None):
        raise ValueError("loc_preds and loc_filter_thr go together")
    arr, L, B, N, dtype, named = _heads(shape_preds, loc_preds, "guided_anchors")
    try:
        tensor(squares, "squares", F32, (N, 4))
    except ValueError as e:
        raise ValueError("%s (the levels hold N = %d locations per image)" % (e, N)) from None
    means, stds = f4(means, "anchoring_means"), f4(stds, "anchoring_stds")
    thr = 0.0 if loc_preds is None else _loc_threshold(loc_filter_thr)
    on_device(named + [("squares", squares)])
    dev = squares.device
    anchors = torch.empty(B, N, 4, dtype=F32, device=dev)
    loc_mask = torch.empty(B, N, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().tdn_guided_anchors(arr, L, B, CODES[dtype], _ptr(squares), means, stds,
                                              0 if loc_preds is None else 1, thr, _ptr(anchors), _ptr(loc_mask),
                                              _lib.stream_ptr()), "tdn_guided_anchors")
    return anchors, loc_mask


def _like(t):
    """An uninitialised tensor of ``t``'s shape, dtype and strides (its memory is one flat array either way)."""
    flat = torch.empty(t.numel(), dtype=t.dtype, device=t.device)
    return flat.as_strided(tuple(t.shape), tuple(t.stride()))


def _loss_setup(loc_preds, shape_preds, loc_targets, loc_weights, bbox_anchors, bbox_gts, bbox_weights, loc_avg_factor,
                gamma, alpha, beta, eps, means, stds):
    arr, L, B, N, dtype, named = _heads(shape_preds, loc_preds, "ga_loss")
    cfg = _lib.GaLossConfig()
    cfg.dtype = CODES[dtype]
    cfg.gamma, cfg.alpha = number(gamma, "gamma"), number(alpha, "alpha")
    if cfg.gamma < 0 or not 0 <= cfg.alpha <= 1:
        raise ValueError("focal loss needs gamma >= 0 and alpha in [0, 1]")
    cfg.beta = number(beta, "beta", positive=True)
    cfg.eps = number(eps, "eps")
    if not 0 < cfg.eps < 1:
        raise ValueError("eps must be in (0, 1), got %r" % eps)
    cfg.loc_avg_factor = number(loc_avg_factor, "loc_avg_factor", positive=True)
    cfg.means, cfg.stds = f4(means, "anchoring_means"), f4(stds, "anchoring_stds")
    what = "(the levels hold N = %d locations per image)" % N
    for t, name, dt, shape in ((loc_targets, "loc_targets", torch.int64, (B, N)),
                               (loc_weights, "loc_weights", F32, (B, N)),
                               (bbox_anchors, "bbox_anchors", F32, (B, N, 4)),
                               (bbox_gts, "bbox_gts", F32, (B, N, 4)),
                               (bbox_weights, "bbox_weights", F32, (B, N, 4))):
        try:
            tensor(t, name, dt, shape)
        except ValueError as e:
            raise ValueError("%s %s" % (e, what)) from None
    named += [("loc_targets", loc_targets), ("loc_weights", loc_weights), ("bbox_anchors", bbox_anchors),
              ("bbox_gts", bbox_gts), ("bbox_weights", bbox_weights)]
    return arr, L, B, cfg, named


def ga_loss_fwd(loc_preds, shape_preds, loc_targets, loc_weights, bbox_anchors, bbox_gts, bbox_weights, loc_avg_factor,
                shape_avg_factor, gamma, alpha, beta, eps, means, stds):
    """-> (losses (2,) float32 = [loss_loc, loss_shape], the divisors (2,) float32 that the backward call takes)."""
    arr, L, B, cfg, named = _loss_setup(loc_preds, shape_preds, loc_targets, loc_weights, bbox_anchors, bbox_gts,
                                        bbox_weights, loc_avg_factor, gamma, alpha, beta, eps, means, stds)
    av, avg_tensors = _avg(shape_avg_factor, False)
    on_device(named + [("shape_avg_factor", t) for t in avg_tensors])
    dev = loc_targets.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_ga_loss_workspace_bytes(arr, L, B, ctypes.byref(cfg)), "ga_loss")
    losses = torch.empty(2, dtype=F32, device=dev)
    norm = torch.empty(2, dtype=F32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_ga_loss_fwd(arr, L, B, ctypes.byref(cfg), _ptr(loc_targets), _ptr(loc_weights),
                                   _ptr(bbox_anchors), _ptr(bbox_gts), _ptr(bbox_weights), ctypes.byref(av),
                                   _ptr(losses), _ptr(norm), wp, nbytes, _lib.stream_ptr()), "tdn_ga_loss_fwd")
    return losses, norm


def ga_loss_bwd(loc_preds, shape_preds, loc_targets, loc_weights, bbox_anchors, bbox_gts, bbox_weights, g, norm,
                gamma, alpha, beta, eps, means, stds):
    """Gradients of ``g . losses``: one tensor per head output with its shape, dtype and strides.  ``g``: (2,) float32;
    ``norm``: what the forward call returned."""
    arr, L, B, cfg, named = _loss_setup(loc_preds, shape_preds, loc_targets, loc_weights, bbox_anchors, bbox_gts,
                                        bbox_weights, 1.0, gamma, alpha, beta, eps, means, stds)
    tensor(g, "g", F32, (2,))
    tensor(norm, "norm", F32, (2,))
    on_device(named + [("g", g), ("norm", norm)])
    dloc = [_like(t) for t in loc_preds]
    dshape = [_like(t) for t in shape_preds]
    for l in range(L):
        arr[l].dloc, arr[l].dshape = dloc[l].data_ptr(), dshape[l].data_ptr()
    _lib.check(_lib.load().tdn_ga_loss_bwd(arr, L, B, ctypes.byref(cfg), _ptr(loc_targets), _ptr(loc_weights),
                                           _ptr(bbox_anchors), _ptr(bbox_gts), _ptr(bbox_weights), _ptr(g), _ptr(norm),
                                           _lib.stream_ptr()), "tdn_ga_loss_bwd")
    return dloc, dshape


def ga_rpn_proposals(cls_scores, bbox_preds, anchors, loc_mask, img_shapes, nms_pre, nms_post, max_num, nms_thr,
                     min_bbox_size, means, stds):
    """RPN proposals from guided anchors (tdn_ga_rpn_proposals): ``rpn_proposals`` with one anchor per location,
    per-image ``anchors`` (B, Nloc, 4) and ``loc_mask`` (B, Nloc).  Returns (proposals (B, max_num, 5) float32,
    anchor_idx (B, max_num) int64, counts (B,) int32)."""
    cls_scores, bbox_preds = list(cls_scores), list(bbox_preds)
    L = len(cls_scores)
    if not (1 <= L <= _lib.RPN_MAX_LEVELS) or len(bbox_preds) != L:
        raise ValueError("ga_rpn_proposals takes 1..%d levels with one cls_score and one bbox_pred each"
                         % _lib.RPN_MAX_LEVELS)
    B = tensor(cls_scores[0], "cls_scores[0]", (F32, BF16), ("B", 1, "H", "W"), contiguous=False)[0]
    batch(B)
    dtype = cls_scores[0].dtype
    cfg = _lib.RpnConfig()
    cfg.nms_pre = nms_pre = integer(nms_pre, "nms_pre", 0, _lib.NMS_SEG_MAX)
    cfg.nms_post = integer(nms_post, "nms_post", 1)
    cfg.max_num = max_num = integer(max_num, "max_num", 1, _lib.RPN_MAX_NUM)
    cfg.nms_thr, cfg.min_bbox_size = number(nms_thr, "nms_thr"), number(min_bbox_size, "min_bbox_size")
    if cfg.min_bbox_size < 0:
        raise ValueError("min_bbox_size must be >= 0")
    cfg.means, cfg.stds = f4(means, "target_means"), f4(stds, "target_stds")
    arr = (_lib.RpnLevel * L)()
    named, N = [], 0
    for l, (c, d) in enumerate(zip(cls_scores, bbox_preds)):
        cn, dn = "cls_scores[%d]" % l, "bbox_preds[%d]" % l
        _, _, H, W = tensor(c, cn, dtype, (B, 1, "H", "W"), contiguous=False)   # one anchor per location
        if H < 1 or W < 1:
            raise ValueError("level %d: empty cls_score %s" % (l, tuple(c.shape)))
        tensor(d, dn, dtype, (B, 4, H, W), contiguous=False)
        if nms_pre == 0 and H * W > _lib.NMS_SEG_MAX:
            raise ValueError("level %d: %d locations enter NMS with nms_pre=0 (max %d)" % (l, H * W, _lib.NMS_SEG_MAX))
        named += [(cn, c), (dn, d)]
        v = arr[l]
        v.logits, v.deltas = c.data_ptr(), d.data_ptr()
        v.logit_strides[:] = list(c.stride())
        v.delta_strides[:] = list(d.stride())
        v.dtype, v.H, v.W, v.A = CODES[dtype], H, W, 1
        N += H * W
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%d locations per image (max %d)" % (N, _lib.TARGET_MAX_BOXES))
    what = "(the levels hold N = %d locations per image)" % N
    for t, name, dt, shape in ((anchors, "anchors", F32, (B, N, 4)), (loc_mask, "loc_mask", (torch.uint8, torch.bool),
                                                                      (B, N))):
        try:
            tensor(t, name, dt, shape)
        except ValueError as e:
            raise ValueError("%s %s" % (e, what)) from None
    loc_mask = loc_mask.view(torch.uint8)
    tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    on_device(named + [("anchors", anchors), ("loc_mask", loc_mask), ("img_shapes", img_shapes)])
    dev = anchors.device
    for l in range(L):
        arr[l].anchors = anchors.data_ptr()
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_ga_rpn_proposals_workspace_bytes(arr, L, B, ctypes.byref(cfg)), "ga_rpn_proposals")
    proposals = torch.empty(B, max_num, 5, dtype=F32, device=dev)
    anchor_idx = torch.empty(B, max_num, dtype=torch.int64, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_ga_rpn_proposals(arr, L, B, _ptr(anchors), _ptr(loc_mask), _ptr(img_shapes), ctypes.byref(cfg),
                                        _ptr(proposals), _ptr(anchor_idx), _ptr(counts), wp, nbytes,
                                        _lib.stream_ptr()), "tdn_ga_rpn_proposals")
    return proposals, anchor_idx, counts
