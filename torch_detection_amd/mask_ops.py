"""Host wrappers of the mask-branch kernels (csrc/mask.hip), written in the vocabulary of ``_args.py``
(DESIGN.md §5e): every shape, dtype, layout and limit is checked here, before any launch (ValueError) — shapes and
limits first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated here, the
library allocates nothing and never synchronises, so every call can be captured in a graph.

Like ``loss_ops.py`` and ``detect_ops.py`` these live beside ``ops.py`` rather than in it (``tests/test_gpu_guarded.py``
takes a census of ``ops.py``); ``tests/test_gpu_mask.py`` puts THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, batch, integer, number, on_device, tensor
from .loss_ops import _avg, _layout
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)


def _like(t):
    """An uninitialised tensor of ``t``'s shape, dtype and strides (its memory is one flat array either way)."""
    flat = torch.empty(t.numel(), dtype=t.dtype, device=t.device)
    return flat.as_strided(tuple(t.shape), tuple(t.stride()))


def _pred(mask_pred, R=None):
    """Checks of a (R, C, M, M) logits tensor -> (R, C, M, layout code)."""
    R, C, M, _ = tensor(mask_pred, "mask_pred", tuple(CODES), ("R" if R is None else R, "C", "M", "M"), contiguous=False)
    if mask_pred.shape[3] != M or not 1 <= M <= _lib.MASK_MAX_SIZE:
        raise ValueError("mask_pred must be (R, C, M, M) with M in 1..%d, got %s"
                         % (_lib.MASK_MAX_SIZE, tuple(mask_pred.shape)))
    if not 1 <= C <= _lib.LOSS_MAX_CLASSES:
        raise ValueError("mask_pred has %d channels (1..%d)" % (C, _lib.LOSS_MAX_CLASSES))
    if R > _lib.LOSS_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (R, _lib.LOSS_MAX_ROWS))
    if R * C * M * M >= 1 << 31:
        raise ValueError("mask_pred holds 2^31 elements or more")
    return R, C, M, _layout(mask_pred, "mask_pred")


def mask_target(rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_size):
    """-> (mask_targets (R, M, M) uint8, mask_weights (R,) float32), one launch (tdn_mask_target)."""
    M = integer(mask_size, "mask_size", 1, _lib.MASK_MAX_SIZE)
    R = tensor(rois, "rois", torch.float32, ("R", 5))[0]
    if R > _lib.LOSS_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (R, _lib.LOSS_MAX_ROWS))
    tensor(pos_assigned_gt_inds, "pos_assigned_gt_inds", torch.int32, (R,))
    P = tensor(poly_xy, "poly_xy", torch.float32, ("P", 2))[0]
    Q = tensor(poly_offsets, "poly_offsets", torch.int32, ("Q+1",))[0] - 1
    B, G = tensor(gt_poly_offsets, "gt_poly_offsets", torch.int32, ("B", "G+1"))
    G -= 1
    if Q < 0 or G < 0:
        raise ValueError("poly_offsets and the rows of gt_poly_offsets hold at least one entry")
    batch(B)
    if G > _lib.TARGET_MAX_GT:
        raise ValueError("gt_poly_offsets describes %d ground truths per image (max %d)" % (G, _lib.TARGET_MAX_GT))
    on_device([("rois", rois), ("pos_assigned_gt_inds", pos_assigned_gt_inds), ("poly_xy", poly_xy),
               ("poly_offsets", poly_offsets), ("gt_poly_offsets", gt_poly_offsets)])
    dev = rois.device
    targets = torch.empty(R, M, M, dtype=torch.uint8, device=dev)
    weights = torch.empty(R, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tdn_mask_target(_ptr(rois), _ptr(pos_assigned_gt_inds), R, _ptr(poly_xy), P,
                                           _ptr(poly_offsets), Q, _ptr(gt_poly_offsets), B, G, M, _ptr(targets),
                                           _ptr(weights), _lib.stream_ptr()), "tdn_mask_target")
    return targets, weights


def _loss_setup(mask_pred, mask_targets, labels, mask_weights):
    R, C, M, nhwc = _pred(mask_pred)
    tensor(mask_targets, "mask_targets", torch.uint8, (R, M, M))
    tensor(labels, "labels", torch.int64, (R,))
    tensor(mask_weights, "mask_weights", torch.float32, (R,))
    named = [("mask_pred", mask_pred), ("mask_targets", mask_targets), ("labels", labels),
             ("mask_weights", mask_weights)]
    return R, C, M, nhwc, named


def mask_head_loss_fwd(mask_pred, mask_targets, labels, mask_weights, avg_factor):
    """-> (loss (1,) float32, the divisor D (1,) float32 that the backward call takes)."""
    R, C, M, nhwc, named = _loss_setup(mask_pred, mask_targets, labels, mask_weights)
    av, avg_ts = _avg(avg_factor, allow_none=True)
    on_device(named + [("avg_factor", t) for t in avg_ts])
    dev = mask_pred.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_mask_loss_workspace_bytes(R), "mask_head_loss")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    avg = torch.empty(1, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_mask_loss_fwd(_ptr(mask_pred), CODES[mask_pred.dtype], nhwc, R, C, M, _ptr(mask_targets),
                                     _ptr(labels), _ptr(mask_weights), ctypes.byref(av), _ptr(loss), _ptr(avg), wp,
                                     nbytes, _lib.stream_ptr()), "tdn_mask_loss_fwd")
    return loss, avg


def mask_head_loss_bwd(mask_pred, mask_targets, labels, mask_weights, g, avg):
    """The gradient of ``g[0] * loss`` with ``mask_pred``'s shape, dtype and strides, written in full."""
    R, C, M, nhwc, named = _loss_setup(mask_pred, mask_targets, labels, mask_weights)
    tensor(g, "g", torch.float32, (1,))
    tensor(avg, "avg", torch.float32, (1,))
    on_device(named + [("g", g), ("avg", avg)])
    dpred = _like(mask_pred)
    _lib.check(_lib.load().tdn_mask_loss_bwd(_ptr(mask_pred), CODES[mask_pred.dtype], nhwc, R, C, M, _ptr(mask_targets),
                                             _ptr(labels), _ptr(mask_weights), _ptr(g), _ptr(avg), _ptr(dpred),
                                             _lib.stream_ptr()), "tdn_mask_loss_bwd")
    return dpred


def _dets(dets, counts):
    B, max_num, _ = tensor(dets, "dets", torch.float32, ("B", "max_num", 5))
    batch(B)
    if not 1 <= max_num <= _lib.RPN_MAX_NUM:
        raise ValueError("dets hold %d rows per image (1..%d)" % (max_num, _lib.RPN_MAX_NUM))
    tensor(counts, "counts", torch.int32, (B,))
    return B, max_num


def rois_from_detections(dets, counts, scale_factors):
    """(B*max_num, 5) rois (b, x1 s, y1 s, x2 s, y2 s) from ``multiclass_nms``' output; rows at or past counts[b] are
    (-1, 0, 0, 0, 0) (tdn_rois_from_detections; no host synchronisation)."""
    B, max_num = _dets(dets, counts)
    scale_t, scale_v = None, 1.0
    if torch.is_tensor(scale_factors):              # or None, or a positive number
        tensor(scale_factors, "scale_factors", torch.float32, (B,))
        scale_t = scale_factors
    elif scale_factors is not None:
        scale_v = number(scale_factors, "scale_factors", positive=True)
    on_device([("dets", dets), ("counts", counts), ("scale_factors", scale_t)])
    rois = torch.empty(B * max_num, 5, dtype=torch.float32, device=dets.device)
    _lib.check(_lib.load().tdn_rois_from_detections(_ptr(dets), _ptr(counts), B, max_num, _ptr(scale_t), scale_v,
                                                    _ptr(rois), _lib.stream_ptr()), "tdn_rois_from_detections")
    return rois


def mask_head_masks(mask_pred, dets, labels, counts, out_shape, img_shapes, thr, packed):
    """-> (B*max_num, H, W) uint8 masks, or (B*max_num, H, 8*ceil(W/64)) packed bits (tdn_mask_paste, one launch)."""
    B, max_num = _dets(dets, counts)
    R, C, M, nhwc = _pred(mask_pred, B * max_num)
    tensor(labels, "labels", torch.int64, (B, max_num))
    try:
        H, W = out_shape
    except (TypeError, ValueError):
        raise ValueError("out_shape must be (H, W)") from None
    H, W = integer(H, "out_shape[0]", 1, 1 << 16), integer(W, "out_shape[1]", 1, 1 << 16)
    if img_shapes is not None:
        tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    thr = number(thr, "thr")
    if R * ((H + 15) // 16) >= 1 << 31:
        raise ValueError("out_shape: %d masks of %d rows are more than one launch takes" % (R, H))
    on_device([("mask_pred", mask_pred), ("dets", dets), ("labels", labels), ("counts", counts),
               ("img_shapes", img_shapes)])
    out = torch.empty(R, H, 8 * ((W + 63) // 64) if packed else W, dtype=torch.uint8, device=mask_pred.device)
    _lib.check(_lib.load().tdn_mask_paste(_ptr(mask_pred), CODES[mask_pred.dtype], nhwc, B, max_num, C, M, _ptr(dets),
                                          _ptr(labels), _ptr(counts), _ptr(img_shapes), H, W, thr, 1 if packed else 0,
                                          _ptr(out), _lib.stream_ptr()), "tdn_mask_paste")
    return out
