"""Host wrappers of the loss kernels (csrc/loss.hip): every shape, dtype, layout and limit is checked
here, before any launch (ValueError) — shapes and limits first, so that those refusals need no GPU, the device last;
outputs and the workspace are allocated here, the library allocates nothing and never synchronises, so every call can
be captured in a graph.

Like ``target_ops.py`` these live beside ``ops.py`` rather than in it (``tests/test_gpu_guarded.py`` takes a census of
``ops.py``); ``tests/test_gpu_losses.py`` puts THIS module under the same guard.
"""
import ctypes
import math

import torch

from . import _lib
from .ops import _aligned_ws, _chk_dev, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)

_CODES = {torch.bfloat16: _lib.TDN_BF16, torch.float16: _lib.TDN_F16, torch.float32: _lib.TDN_F32}


def _number(v, name, positive=False):
    if torch.is_tensor(v) or isinstance(v, (tuple, list)):
        raise ValueError("%s must be a number" % name)
    v = float(v)
    if not math.isfinite(v) or (positive and v <= 0):
        raise ValueError("%s must be finite%s, got %r" % (name, " and > 0" if positive else "", v))
    return v


def _layout(t, name):
    """0: NCHW-contiguous memory, 1: channels_last memory; anything else is refused."""
    if t.is_contiguous():
        return 0
    if t.is_contiguous(memory_format=torch.channels_last):
        return 1
    raise ValueError("%s must be NCHW-contiguous or channels_last, got strides %s for shape %s" %
                     (name, tuple(t.stride()), tuple(t.shape)))


def _chk_target(t, name, dtype, shape):
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s must be a contiguous %s tensor of shape %s, got %s" % (
            name, str(dtype).replace("torch.", ""), tuple(shape),
            (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)))


def _chk_cuda(tensors):
    for name, t in tensors:
        if t is not None:
            if not t.is_cuda:
                raise ValueError("%s must be a CUDA tensor" % name)
            _chk_dev(t, name)


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
        for t in ts:
            if not torch.is_tensor(t) or t.dtype != torch.int32 or not t.is_contiguous() or \
                    t.numel() > _lib.LOSS_MAX_AVG:
                raise ValueError("avg_factor tensors must be contiguous int32 with at most %d elements"
                                 % _lib.LOSS_MAX_AVG)
        av.mode = 1
        av.a, av.na = ts[0].data_ptr() if ts[0].numel() else None, ts[0].numel()
        if len(ts) == 2:
            av.b, av.nb = ts[1].data_ptr() if ts[1].numel() else None, ts[1].numel()
        return av, ts
    av.mode = 0
    av.value = _number(avg_factor, "avg_factor", positive=True)
    return av, ()


def _dense_setup(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, num_classes, beta, gamma,
                 alpha):
    """Checks of a dense-head call -> (levels array, L, B, config, tensors to check for their device)."""
    cls_scores, bbox_preds = list(cls_scores), list(bbox_preds)
    L = len(cls_scores)
    if not 1 <= L <= _lib.LOSS_MAX_LEVELS or len(bbox_preds) != L:
        raise ValueError("anchor_head_loss takes 1..%d levels with one cls_score and one bbox_pred each"
                         % _lib.LOSS_MAX_LEVELS)
    C = int(num_classes)
    if not 1 <= C <= _lib.LOSS_MAX_CLASSES:
        raise ValueError("num_classes must be in 1..%d, got %d" % (_lib.LOSS_MAX_CLASSES, C))
    beta = _number(beta, "beta", positive=True)
    cfg = _lib.LossConfig()
    cfg.num_classes, cfg.beta = C, beta
    if gamma is not None:
        cfg.focal = 1
        cfg.gamma, cfg.alpha = _number(gamma, "gamma"), _number(alpha, "alpha")
        if cfg.gamma < 0 or not 0 <= cfg.alpha <= 1:
            raise ValueError("focal loss needs gamma >= 0 and alpha in [0, 1]")
    first = cls_scores[0]
    if not torch.is_tensor(first) or first.dim() != 4 or first.dtype not in _CODES:
        raise ValueError("cls_scores must be (B, A*C, H, W) float32 / bfloat16 / float16 tensors")
    B, dtype = first.shape[0], first.dtype
    if not 1 <= B <= 64:
        raise ValueError("batch size must be 1..64, got %d" % B)
    if first.shape[1] % C or first.shape[1] == 0:
        raise ValueError("cls_scores have %d channels, no multiple of num_classes = %d" % (first.shape[1], C))
    A = first.shape[1] // C
    cfg.dtype, cfg.num_anchors = _CODES[dtype], A
    levels = (_lib.LossLevel * L)()
    N = 0
    for l, (c, r) in enumerate(zip(cls_scores, bbox_preds)):
        for t, name, ch in ((c, "cls_scores[%d]" % l, A * C), (r, "bbox_preds[%d]" % l, 4 * A)):
            if not torch.is_tensor(t) or t.dim() != 4 or t.dtype != dtype or t.shape[0] != B or t.shape[1] != ch:
                raise ValueError("%s must be a (%d, %d, H, W) %s tensor, got %s" % (
                    name, B, ch, str(dtype).replace("torch.", ""),
                    (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t)))
        H, W = c.shape[2], c.shape[3]
        if H < 1 or W < 1 or tuple(r.shape[2:]) != (H, W):
            raise ValueError("level %d: cls_score is %s, bbox_pred is %s" % (l, tuple(c.shape), tuple(r.shape)))
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
            _chk_target(t, name, dt, shape)
        except ValueError as e:
            raise ValueError("%s %s" % (e, what)) from None
    named = [("cls_scores[%d]" % l, t) for l, t in enumerate(cls_scores)] + \
            [("bbox_preds[%d]" % l, t) for l, t in enumerate(bbox_preds)] + \
            [("labels", labels), ("label_weights", label_weights), ("bbox_targets", bbox_targets),
             ("bbox_weights", bbox_weights)]
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
    _chk_cuda(named + [("avg_factor", t) for t in avg_ts])
    dev = labels.device
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    avg = torch.empty(1, dtype=torch.float32, device=dev)
    lib = _lib.load()
    nbytes = lib.tdn_loss_dense_workspace_bytes(levels, L, B, ctypes.byref(cfg))
    if nbytes < 0:
        raise ValueError("tdn_loss_dense_workspace_bytes refused the shapes")
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
    _chk_target(g, "g", torch.float32, (2,))
    _chk_target(avg, "avg", torch.float32, (1,))
    _chk_cuda(named + [("g", g), ("avg", avg)])
    dcls = [_like(t) for t in cls_scores]
    dreg = [_like(t) for t in bbox_preds]
    for l in range(L):
        levels[l].dcls, levels[l].dreg = dcls[l].data_ptr(), dreg[l].data_ptr()
    _lib.check(_lib.load().tdn_loss_dense_bwd(levels, L, B, ctypes.byref(cfg), _ptr(labels), _ptr(label_weights),
                                              _ptr(bbox_targets), _ptr(bbox_weights), _ptr(g), _ptr(avg),
                                              _lib.stream_ptr()), "tdn_loss_dense_bwd")
    return dcls, dreg


def _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta):
    beta = _number(beta, "beta", positive=True)
    if not torch.is_tensor(cls_score) or cls_score.dim() != 2 or cls_score.dtype not in _CODES or \
            not cls_score.is_contiguous():
        raise ValueError("cls_score must be a contiguous (R, C) float32 / bfloat16 / float16 tensor")
    R, C = cls_score.shape
    if not 1 <= C <= _lib.LOSS_MAX_CLASSES:
        raise ValueError("cls_score has %d classes (1..%d)" % (C, _lib.LOSS_MAX_CLASSES))
    if R > _lib.LOSS_MAX_ROWS:
        raise ValueError("%d rows (max %d)" % (R, _lib.LOSS_MAX_ROWS))
    if not torch.is_tensor(bbox_pred) or bbox_pred.dim() != 2 or bbox_pred.dtype != cls_score.dtype or \
            not bbox_pred.is_contiguous() or bbox_pred.shape[0] != R or bbox_pred.shape[1] not in (4, 4 * C):
        raise ValueError("bbox_pred must be a contiguous (%d, %d) or (%d, 4) tensor of cls_score's dtype" %
                         (R, 4 * C, R))
    _chk_target(labels, "labels", torch.int64, (R,))
    _chk_target(label_weights, "label_weights", torch.float32, (R,))
    _chk_target(bbox_targets, "bbox_targets", torch.float32, (R, 4))
    _chk_target(bbox_weights, "bbox_weights", torch.float32, (R, 4))
    if not labels.is_cuda and not label_weights.is_cuda and R:          # only a host tensor can be looked at for free
        bad = ((labels < 0) | (labels >= C)) & (label_weights != 0)
        if bool(bad.any()):
            raise ValueError("labels outside [0, %d) on rows with non-zero weight" % C)
    named = [("cls_score", cls_score), ("bbox_pred", bbox_pred), ("labels", labels), ("label_weights", label_weights),
             ("bbox_targets", bbox_targets), ("bbox_weights", bbox_weights)]
    return R, C, bbox_pred.shape[1], beta, named


def bbox_head_loss_fwd(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, avg_factor, beta):
    R, C, cols, beta, named = _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta)
    av, avg_ts = _avg(avg_factor, allow_none=True)
    _chk_cuda(named + [("avg_factor", t) for t in avg_ts])
    dev = cls_score.device
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    avg = torch.empty(1, dtype=torch.float32, device=dev)
    lib = _lib.load()
    nbytes = lib.tdn_loss_roi_workspace_bytes(R)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_loss_roi_fwd(_ptr(cls_score), _ptr(bbox_pred), _CODES[cls_score.dtype], R, C, cols,
                                    _ptr(labels), _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights), beta,
                                    ctypes.byref(av), _ptr(losses), _ptr(avg), wp, nbytes, _lib.stream_ptr()),
               "tdn_loss_roi_fwd")
    return losses, avg


def bbox_head_loss_bwd(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, g, avg, beta):
    R, C, cols, beta, named = _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta)
    _chk_target(g, "g", torch.float32, (2,))
    _chk_target(avg, "avg", torch.float32, (1,))
    _chk_cuda(named + [("g", g), ("avg", avg)])
    dcls = torch.empty(R, C, dtype=cls_score.dtype, device=cls_score.device)
    dreg = torch.empty(R, cols, dtype=cls_score.dtype, device=cls_score.device)
    _lib.check(_lib.load().tdn_loss_roi_bwd(_ptr(cls_score), _ptr(bbox_pred), _CODES[cls_score.dtype], R, C, cols,
                                            _ptr(labels), _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights),
                                            beta, _ptr(g), _ptr(avg), _ptr(dcls), _ptr(dreg), _lib.stream_ptr()),
               "tdn_loss_roi_bwd")
    return dcls, dreg
