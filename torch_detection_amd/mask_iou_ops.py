"""Host wrappers of the Mask Scoring R-CNN kernels (csrc/mask_iou.hip), written in the vocabulary of
``_args.py``: every shape, dtype, layout and limit is checked here, before any launch (ValueError) —
shapes and limits first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated
here, the library allocates nothing and never synchronises, so every call can be captured in a graph.

These live beside ``mask_ops.py`` rather than in it (``tests/test_gpu_mask.py`` takes a census of that module);
``tests/test_gpu_ms_rcnn.py`` puts THIS module under the guard of ``tests/guard_util.py``.
"""
import torch

from . import _lib
from ._args import CODES, batch, integer, number, on_device, tensor
from .loss_ops import _layout
from .ops import _aligned_ws, _ptr, _workspace, dtype_code  # noqa: F401  (_workspace: swapped by the guard)


def _pred4(mask_pred, R=None):
    """Checks of a (R, C, M, M) logits tensor, or (R, M, M) for C = 1 -> (the 4-D view, C, M, layout code)."""
    if isinstance(mask_pred, torch.Tensor) and mask_pred.dim() == 3:
        tensor(mask_pred, "mask_pred", tuple(CODES), ("R" if R is None else R, "M", "M"))
        mask_pred = mask_pred.unsqueeze(1)
    R, C, M, _ = tensor(mask_pred, "mask_pred", tuple(CODES), ("R" if R is None else R, "C", "M", "M"), contiguous=False)
    if mask_pred.shape[3] != M or not 1 <= M <= _lib.MASK_MAX_SIZE:
        raise ValueError("mask_pred must be (R, C, M, M) with M in 1..%d, got %s"
                         % (_lib.MASK_MAX_SIZE, tuple(mask_pred.shape)))
    if not 1 <= C <= _lib.LOSS_MAX_CLASSES:
        raise ValueError("mask_pred has %d channels (1..%d)" % (C, _lib.LOSS_MAX_CLASSES))
    if R * C * M * M >= 1 << 31:
        raise ValueError("mask_pred holds 2^31 elements or more")
    return mask_pred, C, M, _layout(mask_pred, "mask_pred")


def mask_iou_target(rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_pred, labels, mask_targets,
                    img_shapes, thr):
    """-> mask_iou_targets (R,) float32, one launch (tdn_mask_iou_target)."""
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
    pred, C, M, nhwc = _pred4(mask_pred, R)
    tensor(labels, "labels", torch.int64, (R,))
    tensor(mask_targets, "mask_targets", torch.uint8, (R, M, M))
    tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    thr = number(thr, "thr")
    on_device([("rois", rois), ("pos_assigned_gt_inds", pos_assigned_gt_inds), ("poly_xy", poly_xy),
               ("poly_offsets", poly_offsets), ("gt_poly_offsets", gt_poly_offsets), ("mask_pred", mask_pred),
               ("labels", labels), ("mask_targets", mask_targets), ("img_shapes", img_shapes)])
    iou = torch.empty(R, dtype=torch.float32, device=rois.device)
    _lib.check(_lib.load().tdn_mask_iou_target(_ptr(rois), _ptr(pos_assigned_gt_inds), R, _ptr(poly_xy), P,
                                               _ptr(poly_offsets), Q, _ptr(gt_poly_offsets), B, G, _ptr(pred),
                                               CODES[pred.dtype], nhwc, C, M, _ptr(labels), _ptr(mask_targets),
                                               _ptr(img_shapes), thr, _ptr(iou), _lib.stream_ptr()),
               "tdn_mask_iou_target")
    return iou


def _loss_setup(mask_iou_pred, labels, mask_iou_targets, loss_weight):
    R, C = tensor(mask_iou_pred, "mask_iou_pred", tuple(CODES), ("R", "C"))
    if R > _lib.LOSS_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (R, _lib.LOSS_MAX_ROWS))
    if not 1 <= C <= _lib.LOSS_MAX_CLASSES:
        raise ValueError("mask_iou_pred has %d columns (1..%d)" % (C, _lib.LOSS_MAX_CLASSES))
    tensor(labels, "labels", torch.int64, (R,))
    tensor(mask_iou_targets, "mask_iou_targets", torch.float32, (R,))
    named = [("mask_iou_pred", mask_iou_pred), ("labels", labels), ("mask_iou_targets", mask_iou_targets)]
    return R, C, number(loss_weight, "loss_weight"), named


def mask_iou_loss_fwd(mask_iou_pred, labels, mask_iou_targets, loss_weight):
    """-> (loss (1,) float32, the divisor D (1,) float32 that the backward call takes); two launches."""
    R, C, lw, named = _loss_setup(mask_iou_pred, labels, mask_iou_targets, loss_weight)
    on_device(named)
    dev = mask_iou_pred.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_mask_iou_loss_workspace_bytes(R), "mask_iou_loss")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    avg = torch.empty(1, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_mask_iou_loss_fwd(_ptr(mask_iou_pred), CODES[mask_iou_pred.dtype], R, C, _ptr(labels),
                                         _ptr(mask_iou_targets), lw, _ptr(loss), _ptr(avg), wp, nbytes,
                                         _lib.stream_ptr()), "tdn_mask_iou_loss_fwd")
    return loss, avg


def mask_iou_loss_bwd(mask_iou_pred, labels, mask_iou_targets, loss_weight, g, avg):
    """The gradient of ``g[0] * loss``: (R, C) in ``mask_iou_pred``'s dtype, written in full; one launch."""
    R, C, lw, named = _loss_setup(mask_iou_pred, labels, mask_iou_targets, loss_weight)
    tensor(g, "g", torch.float32, (1,))
    tensor(avg, "avg", torch.float32, (1,))
    on_device(named + [("g", g), ("avg", avg)])
    dpred = torch.empty(R, C, dtype=mask_iou_pred.dtype, device=mask_iou_pred.device)
    _lib.check(_lib.load().tdn_mask_iou_loss_bwd(_ptr(mask_iou_pred), CODES[mask_iou_pred.dtype], R, C, _ptr(labels),
                                                 _ptr(mask_iou_targets), lw, _ptr(g), _ptr(avg), _ptr(dpred),
                                                 _lib.stream_ptr()), "tdn_mask_iou_loss_bwd")
    return dpred


def mask_scores(mask_iou_pred, dets, labels, counts):
    """-> (B, max_num) float32, one launch (tdn_mask_scores)."""
    B, max_num, _ = tensor(dets, "dets", torch.float32, ("B", "max_num", 5))
    batch(B)
    if not 1 <= max_num <= _lib.RPN_MAX_NUM:
        raise ValueError("dets hold %d rows per image (1..%d)" % (max_num, _lib.RPN_MAX_NUM))
    C = tensor(mask_iou_pred, "mask_iou_pred", tuple(CODES), (B * max_num, "C"))[1]
    if not 1 <= C <= _lib.LOSS_MAX_CLASSES:
        raise ValueError("mask_iou_pred has %d columns (1..%d)" % (C, _lib.LOSS_MAX_CLASSES))
    tensor(labels, "labels", torch.int64, (B, max_num))
    tensor(counts, "counts", torch.int32, (B,))
    on_device([("mask_iou_pred", mask_iou_pred), ("dets", dets), ("labels", labels), ("counts", counts)])
    scores = torch.empty(B, max_num, dtype=torch.float32, device=dets.device)
    _lib.check(_lib.load().tdn_mask_scores(_ptr(mask_iou_pred), CODES[mask_iou_pred.dtype], B, max_num, C, _ptr(dets),
                                           _ptr(labels), _ptr(counts), _ptr(scores), _lib.stream_ptr()),
               "tdn_mask_scores")
    return scores


def _stem_setup(mask_pred, labels, weight, label_offset):
    pred, C, M, nhwc = _pred4(mask_pred)
    R = pred.shape[0]
    if M % 2:
        raise ValueError("mask_pred must be (R, C, 2S, 2S), got M = %d" % M)
    if not 1 <= R <= _lib.LOSS_MAX_ROWS:
        raise ValueError("%d rows (1..%d)" % (R, _lib.LOSS_MAX_ROWS))
    tensor(labels, "labels", torch.int64, (R,))
    Cout, Cin, _, _ = tensor(weight, "weight", torch.float32, ("Cout", "Cf+1", 3, 3))
    Cf = Cin - 1
    if Cf < 64 or Cf % 64:
        raise ValueError("weight: Cf = %d input feature channels must be a positive multiple of 64" % Cf)
    if Cout % 64 or not 64 <= Cout <= _lib.MASK_IOU_MAX_COUT:
        raise ValueError("weight: Cout must be a multiple of 64 in 64..%d, got %d" % (_lib.MASK_IOU_MAX_COUT, Cout))
    S = M // 2
    if R * S * S * Cout >= 1 << 31:
        raise ValueError("the layer's output holds 2^31 elements or more")
    off = integer(label_offset, "label_offset", -1, 1)
    return pred, R, C, S, nhwc, Cf, Cout, off


def mask_iou_stem_fwd(mask_pred, labels, weight, label_offset, dtype):
    """-> (a (R, S, S, Cout) ``dtype``: the conv epilogue's addend, P (R, S, S) float32, idx (R, S, S) uint8); one
    launch (tdn_mask_iou_stem_fwd)."""
    pred, R, C, S, nhwc, Cf, Cout, off = _stem_setup(mask_pred, labels, weight, label_offset)
    code = dtype_code(dtype)
    on_device([("mask_pred", mask_pred), ("labels", labels), ("weight", weight)])
    dev = pred.device
    a = torch.empty(R, S, S, Cout, dtype=dtype, device=dev)
    P = torch.empty(R, S, S, dtype=torch.float32, device=dev)
    idx = torch.empty(R, S, S, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().tdn_mask_iou_stem_fwd(_ptr(pred), CODES[pred.dtype], nhwc, R, C, S, _ptr(labels), off,
                                                 _ptr(weight), Cf, Cout, _ptr(a), code, _ptr(P), _ptr(idx),
                                                 _lib.stream_ptr()), "tdn_mask_iou_stem_fwd")
    return a, P, idx


def mask_iou_stem_bwd(gz, P, idx, mask_pred, labels, weight, label_offset):
    """From ``gz`` (R, S, S, Cout), the layer's cotangent behind its ReLU -> (dmask_pred with ``mask_pred``'s shape, dtype
    and strides, written in full, dw1 (Cout, 3, 3) float32: the gradient of ``weight[:, Cf]``, dP (R, S, S) float32); two
    launches (tdn_mask_iou_stem_bwd)."""
    pred, R, C, S, nhwc, Cf, Cout, off = _stem_setup(mask_pred, labels, weight, label_offset)
    tensor(gz, "gz", (torch.bfloat16, torch.float16), (R, S, S, Cout))
    tensor(P, "P", torch.float32, (R, S, S))
    tensor(idx, "idx", torch.uint8, (R, S, S))
    on_device([("gz", gz), ("P", P), ("idx", idx), ("mask_pred", mask_pred), ("labels", labels), ("weight", weight)])
    dev = pred.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_mask_iou_stem_bwd_workspace_bytes(R, S, Cout), "mask_iou_stem_bwd")
    flat = torch.empty(pred.numel(), dtype=pred.dtype, device=dev)
    dpred = flat.as_strided(tuple(mask_pred.shape), tuple(mask_pred.stride()))
    dw1 = torch.empty(Cout, 3, 3, dtype=torch.float32, device=dev)
    dP = torch.empty(R, S, S, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_mask_iou_stem_bwd(_ptr(gz), dtype_code(gz.dtype), _ptr(P), _ptr(idx), _ptr(weight), Cf, Cout,
                                         _ptr(pred), CODES[pred.dtype], nhwc, R, C, S, _ptr(labels), off, _ptr(dP),
                                         _ptr(flat), _ptr(dw1), wp, nbytes, _lib.stream_ptr()),
               "tdn_mask_iou_stem_bwd")
    return dpred, dw1, dP
