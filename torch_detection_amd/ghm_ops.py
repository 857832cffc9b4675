"""Host wrappers of the gradient-harmonised loss kernels (csrc/ghm.hip), written in the vocabulary of
``_args.py``: every shape, dtype, layout and limit is checked here, before any launch (ValueError) —
shapes and limits first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated
here, the library allocates nothing and never synchronises, so every call can be captured in a graph.

``tests/test_gpu_ghm.py`` puts THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, integer, number, on_device, tensor
from .loss_ops import _head_levels
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)

SCOPES = {"level": _lib.GHM_SCOPE_LEVEL, "batch": _lib.GHM_SCOPE_BATCH}
TABLE_SHAPE = (2, _lib.LOSS_MAX_LEVELS, _lib.GHM_TABLE_STRIDE)


def _momentum(v, name):
    v = number(v, name)
    if not 0 <= v < 1 or not 0 <= ctypes.c_float(v).value < 1:
        raise ValueError("%s must lie in [0, 1), got %r" % (name, v))
    return v


def _setup(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, acc_cls, acc_reg, num_classes,
           bins_cls, bins_reg, momentum_cls, momentum_reg, mu, scope):
    """Checks of a GHM call (heads and targets: ``loss_ops._head_levels``) -> (levels array, L, B, config, tensors to
    check for their device)."""
    levels, L, B, A, C, dtype, named = _head_levels("ghm_head_loss", cls_scores, bbox_preds, labels, label_weights,
                                                    bbox_targets, bbox_weights, num_classes)
    cfg = _lib.GhmConfig()
    cfg.dtype, cfg.num_anchors, cfg.num_classes = CODES[dtype], A, C
    cfg.bins_cls = integer(bins_cls, "bins_cls", 1, _lib.GHM_MAX_BINS)
    cfg.bins_reg = integer(bins_reg, "bins_reg", 1, _lib.GHM_MAX_BINS)
    cfg.momentum_cls = _momentum(momentum_cls, "momentum_cls")
    cfg.momentum_reg = _momentum(momentum_reg, "momentum_reg")
    cfg.mu = number(mu, "mu", positive=True)
    if not cfg.mu > 0:
        raise ValueError("mu must be > 0 as a float32, got %r" % (mu,))
    if not isinstance(scope, str) or scope not in SCOPES:
        raise ValueError("scope must be 'level' or 'batch', got %r" % (scope,))
    cfg.scope = SCOPES[scope]
    for acc, name, mmt, bins in ((acc_cls, "acc_cls", cfg.momentum_cls, cfg.bins_cls),
                                 (acc_reg, "acc_reg", cfg.momentum_reg, cfg.bins_reg)):
        if acc is None:
            if mmt > 0:
                raise ValueError("%s may be None only when its momentum is 0 (it is %r)" % (name, mmt))
        else:
            tensor(acc, name, torch.float32, (bins,))
    named = named + [("acc_cls", acc_cls), ("acc_reg", acc_reg)]
    return levels, L, B, cfg, named


def _like(t):
    """An uninitialised tensor of ``t``'s shape, dtype and strides (its memory is one flat array either way)."""
    flat = torch.empty(t.numel(), dtype=t.dtype, device=t.device)
    return flat.as_strided(tuple(t.shape), tuple(t.stride()))


def ghm_head_loss_fwd(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, acc_cls, acc_reg,
                      num_classes, bins_cls, bins_reg, momentum_cls, momentum_reg, mu, scope):
    """-> (losses (2,) float32 = [loss_cls, loss_bbox], table (2, 8, 136) float32: per (kind, row) beta [64], the bin
    counts [64], tot, the number of non-empty bins, the number of valid elements in no bin — what the backward call
    takes).  ``acc_cls`` / ``acc_reg`` are advanced in place."""
    levels, L, B, cfg, named = _setup(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights,
                                      acc_cls, acc_reg, num_classes, bins_cls, bins_reg, momentum_cls, momentum_reg,
                                      mu, scope)
    on_device(named)
    dev = labels.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_ghm_workspace_bytes(levels, L, B, ctypes.byref(cfg)), "ghm_head_loss")
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    table = torch.empty(TABLE_SHAPE, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_ghm_fwd(levels, L, B, ctypes.byref(cfg), _ptr(labels), _ptr(label_weights), _ptr(bbox_targets),
                               _ptr(bbox_weights), _ptr(acc_cls), _ptr(acc_reg), _ptr(losses), _ptr(table), wp, nbytes,
                               _lib.stream_ptr()), "tdn_ghm_fwd")
    return losses, table


def ghm_head_loss_bwd(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, g, table,
                      num_classes, bins_cls, bins_reg, momentum_cls, momentum_reg, mu, scope):
    """Gradients of ``g[0] * loss_cls + g[1] * loss_bbox``: one tensor per head output, with its shape, dtype and
    strides.  ``g``: (2,) float32, ``table``: what the forward call returned.  Neither running average is read."""
    levels, L, B, cfg, named = _setup(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights,
                                      None, None, num_classes, bins_cls, bins_reg, 0.0, 0.0, mu, scope)
    tensor(g, "g", torch.float32, (2,))
    tensor(table, "table", torch.float32, TABLE_SHAPE)
    on_device(named + [("g", g), ("table", table)])
    dcls = [_like(t) for t in cls_scores]
    dreg = [_like(t) for t in bbox_preds]
    for l in range(L):
        levels[l].dcls, levels[l].dreg = dcls[l].data_ptr(), dreg[l].data_ptr()
    _lib.check(_lib.load().tdn_ghm_bwd(levels, L, B, ctypes.byref(cfg), _ptr(labels), _ptr(label_weights),
                                       _ptr(bbox_targets), _ptr(bbox_weights), _ptr(g), _ptr(table),
                                       _lib.stream_ptr()), "tdn_ghm_bwd")
    return dcls, dreg
