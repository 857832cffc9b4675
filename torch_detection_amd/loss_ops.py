"""Host wrappers of the loss kernels (csrc/loss.hip), written in the vocabulary of ``_args.py``
(DESIGN.md §5e): every shape, dtype, layout and limit is checked here, before any launch (ValueError) — shapes and
limits first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated here, the
library allocates nothing and never synchronises, so every call can be captured in a graph.

Like ``target_ops.py`` these live beside ``ops.py`` rather than in it (``tests/test_gpu_guarded.py`` takes a census of
``ops.py``); ``tests/test_gpu_losses.py`` puts THIS module under the same guard.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, batch, integer, number, on_device, tensor
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)


def _layout(t, name):
    """0: NCHW-contiguous memory, 1: channels_last memory; anything else is refused."""
    if t.is_contiguous():
        return 0
    if t.is_contiguous(memory_format=torch.channels_last):
        return 1
    raise ValueError("%s must be NCHW-contiguous or channels_last, got strides %s for shape %s" %
                     (name, tuple(t.stride()), tuple(t.shape)))


def _avg(avg_factor, allow_none):
    """-> (tdn_loss_avg, the tensors it points to)."""
    av = _lib.LossAvg()
    if avg_factor is None:
        if not allow_none:
            raise ValueError("avg_factor must be a number, an int32 tensor or a tuple of up to two")
        av.mode = 2
        return av, ()
    if torch.is_tensor(avg_factor):
        avg_factor = (avg_factor,)
    if isinstance(avg_factor, (tuple, list)):
        ts = tuple(avg_factor)
        if not 1 <= len(ts) <= 2:
            raise ValueError("avg_factor: a tuple of one or two int32 tensors, got %d entries" % len(ts))
        for t in ts:                                    # of any shape
            tensor(t, "avg_factor", torch.int32, (None,) * (t.dim() if torch.is_tensor(t) else 1))
            if t.numel() > _lib.LOSS_MAX_AVG:
                raise ValueError("avg_factor tensors hold at most %d elements" % _lib.LOSS_MAX_AVG)
        av.mode = 1
        av.a, av.na = ts[0].data_ptr() if ts[0].numel() else None, ts[0].numel()
        if len(ts) == 2:
            av.b, av.nb = ts[1].data_ptr() if ts[1].numel() else None, ts[1].numel()
        return av, ts
    av.mode = 0
    av.value = number(avg_factor, "avg_factor", positive=True)
    return av, ()


def _head_levels(who, cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, num_classes):
    """The head outputs of 1..8 levels and ``anchor_target``'s tensors for them, as ``who`` (this module's dense loss,
    ``ghm_ops.py``) takes them -> (levels array, L, B, A, C, dtype, tensors to check for their device)."""
    cls_scores, bbox_preds = list(cls_scores), list(bbox_preds)
    L = len(cls_scores)
    if not 1 <= L <= _lib.LOSS_MAX_LEVELS or len(bbox_preds) != L:
        raise ValueError("%s takes 1..%d levels with one cls_score and one bbox_pred each" % (who, _lib.LOSS_MAX_LEVELS))
    C = integer(num_classes, "num_classes", 1, _lib.LOSS_MAX_CLASSES)
    B, ch, _, _ = tensor(cls_scores[0], "cls_scores[0]", tuple(CODES), ("B", "A*C", "H", "W"), contiguous=False)
    batch(B)
    if ch % C or ch == 0:
        raise ValueError("cls_scores have %d channels, no multiple of num_classes = %d" % (ch, C))
    A, dtype = ch // C, cls_scores[0].dtype
    levels = (_lib.LossLevel * L)()
    N = 0
    for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
        _, _, H, W = tensor(c, "cls_scores[%d]" % l, dtype, (B, A * C, "H", "W"), contiguous=False)
        if H < 1 or W < 1:
            raise ValueError("level %d: empty cls_score %s" % (l, tuple(c.shape)))
        tensor(r, "bbox_preds[%d]" % l, dtype, (B, 4 * A, H, W), contiguous=False)
        if B * A * max(C, 4) * H * W >= 1 << 31:
            raise ValueError("level %d holds 2^31 elements or more" % l)
        lv = levels[l]
        lv.cls, lv.reg, lv.H, lv.W = c.data_ptr(), r.data_ptr(), H, W
        lv.cls_nhwc, lv.reg_nhwc = _layout(c, "cls_scores[%d]" % l), _layout(r, "bbox_preds[%d]" % l)
        N += H * W * A
    if N > _lib.LOSS_MAX_ROWS:
        raise ValueError("%d anchors per image (max %d)" % (N, _lib.LOSS_MAX_ROWS))
    what = "(the levels hold N = %d anchors per image)" % N
    for t, name, dt, shape in ((labels, "labels", torch.int64, (B, N)),
                               (label_weights, "label_weights", torch.float32, (B, N)),
                               (bbox_targets, "bbox_targets", torch.float32, (B, N, 4)),
                               (bbox_weights, "bbox_weights", torch.float32, (B, N, 4))):
        try:
            tensor(t, name, dt, shape)
        except ValueError as e:
            raise ValueError("%s %s" % (e, what)) from None
    named = [("cls_scores[%d]" % l, t) for l, t in enumerate(cls_scores)] + \
            [("bbox_preds[%d]" % l, t) for l, t in enumerate(bbox_preds)] + \
            [("labels", labels), ("label_weights", label_weights), ("bbox_targets", bbox_targets),
             ("bbox_weights", bbox_weights)]
    return levels, L, B, A, C, dtype, named


def _dense_setup(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, num_classes, beta, gamma,
                 alpha):
    """Checks of a dense-head call -> (levels array, L, B, config, tensors to check for their device)."""
    levels, L, B, A, C, dtype, named = _head_levels("anchor_head_loss", cls_scores, bbox_preds, labels, label_weights,
                                                    bbox_targets, bbox_weights, num_classes)
    cfg = _lib.LossConfig()
    cfg.dtype, cfg.num_anchors, cfg.num_classes = CODES[dtype], A, C
    cfg.beta = number(beta, "beta", positive=True)
    if gamma is not None:
        cfg.focal = 1
        cfg.gamma, cfg.alpha = number(gamma, "gamma"), number(alpha, "alpha")
        if cfg.gamma < 0 or not 0 <= cfg.alpha <= 1:
            raise ValueError("focal loss needs gamma >= 0 and alpha in [0, 1]")
    return levels, L, B, cfg, named


def _like(t):
    """An uninitialised tensor of ``t``'s shape, dtype and strides (its memory is one flat array either way)."""
    flat = torch.empty(t.numel(), dtype=t.dtype, device=t.device)
    return flat.as_strided(tuple(t.shape), tuple(t.stride()))


def anchor_head_loss_fwd(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor,
                         num_classes, beta, gamma, alpha):
    """-> (losses (2,) float32 = [loss_cls, loss_bbox], the divisor (1,) float32 that the backward call takes)."""
    levels, L, B, cfg, named = _dense_setup(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights,
                                            num_classes, beta, gamma, alpha)
    av, avg_ts = _avg(avg_factor, allow_none=False)
    on_device(named + [("avg_factor", t) for t in avg_ts])
    dev = labels.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_loss_dense_workspace_bytes(levels, L, B, ctypes.byref(cfg)), "anchor_head_loss")
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    avg = torch.empty(1, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_loss_dense_fwd(levels, L, B, ctypes.byref(cfg), _ptr(labels), _ptr(label_weights),
                                      _ptr(bbox_targets), _ptr(bbox_weights), ctypes.byref(av), _ptr(losses),
                                      _ptr(avg), wp, nbytes, _lib.stream_ptr()), "tdn_loss_dense_fwd")
    return losses, avg


def anchor_head_loss_bwd(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, g, avg,
                         num_classes, beta, gamma, alpha):
    """Gradients of ``g[0] * loss_cls + g[1] * loss_bbox``: one tensor per head output, with its shape, dtype and
    strides.  ``g``: (2,) float32, ``avg``: what the forward call returned."""
    levels, L, B, cfg, named = _dense_setup(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights,
                                            num_classes, beta, gamma, alpha)
    tensor(g, "g", torch.float32, (2,))
    tensor(avg, "avg", torch.float32, (1,))
    on_device(named + [("g", g), ("avg", avg)])
    dcls = [_like(t) for t in cls_scores]
    dreg = [_like(t) for t in bbox_preds]
    for l in range(L):
        levels[l].dcls, levels[l].dreg = dcls[l].data_ptr(), dreg[l].data_ptr()
    _lib.check(_lib.load().tdn_loss_dense_bwd(levels, L, B, ctypes.byref(cfg), _ptr(labels), _ptr(label_weights),
                                              _ptr(bbox_targets), _ptr(bbox_weights), _ptr(g), _ptr(avg),
                                              _lib.stream_ptr()), "tdn_loss_dense_bwd")
    return dcls, dreg


def _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta):
    beta = number(beta, "beta", positive=True)
    R, C = tensor(cls_score, "cls_score", tuple(CODES), ("R", "C"))
    if not 1 <= C <= _lib.LOSS_MAX_CLASSES:
        raise ValueError("cls_score has %d classes (1..%d)" % (C, _lib.LOSS_MAX_CLASSES))
    if R > _lib.LOSS_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (R, _lib.LOSS_MAX_ROWS))
    cols = tensor(bbox_pred, "bbox_pred", cls_score.dtype, (R, (4 * C, 4)))[1]
    tensor(labels, "labels", torch.int64, (R,))
    tensor(label_weights, "label_weights", torch.float32, (R,))
    tensor(bbox_targets, "bbox_targets", torch.float32, (R, 4))
    tensor(bbox_weights, "bbox_weights", torch.float32, (R, 4))
    if not labels.is_cuda and not label_weights.is_cuda and R:          # only a host tensor can be looked at for free
        bad = ((labels < 0) | (labels >= C)) & (label_weights != 0)
        if bool(bad.any()):
            raise ValueError("labels outside [0, %d) on rows with non-zero weight" % C)
    named = [("cls_score", cls_score), ("bbox_pred", bbox_pred), ("labels", labels), ("label_weights", label_weights),
             ("bbox_targets", bbox_targets), ("bbox_weights", bbox_weights)]
    return R, C, cols, beta, named


def bbox_head_loss_fwd(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, avg_factor, beta):
    R, C, cols, beta, named = _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta)
    av, avg_ts = _avg(avg_factor, allow_none=True)
    on_device(named + [("avg_factor", t) for t in avg_ts])
    dev = cls_score.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_loss_roi_workspace_bytes(R), "bbox_head_loss")
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    avg = torch.empty(1, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_loss_roi_fwd(_ptr(cls_score), _ptr(bbox_pred), CODES[cls_score.dtype], R, C, cols,
                                    _ptr(labels), _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights), beta,
                                    ctypes.byref(av), _ptr(losses), _ptr(avg), wp, nbytes, _lib.stream_ptr()),
               "tdn_loss_roi_fwd")
    return losses, avg


def bbox_head_loss_bwd(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, g, avg, beta):
    R, C, cols, beta, named = _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta)
    tensor(g, "g", torch.float32, (2,))
    tensor(avg, "avg", torch.float32, (1,))
    on_device(named + [("g", g), ("avg", avg)])
    dcls = torch.empty(R, C, dtype=cls_score.dtype, device=cls_score.device)
    dreg = torch.empty(R, cols, dtype=cls_score.dtype, device=cls_score.device)
    _lib.check(_lib.load().tdn_loss_roi_bwd(_ptr(cls_score), _ptr(bbox_pred), CODES[cls_score.dtype], R, C, cols,
                                            _ptr(labels), _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights),
                                            beta, _ptr(g), _ptr(avg), _ptr(dcls), _ptr(dreg), _lib.stream_ptr()),
               "tdn_loss_roi_bwd")
    return dcls, dreg
