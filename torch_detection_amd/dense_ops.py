"""Host wrappers of the dense head predictors (csrc/dense_head.hip), written in the vocabulary of
``_args.py``: every dtype, layout and limit is checked here, before any launch (ValueError that names
the argument) — dtypes, layouts and sizes first, so that those refusals need no GPU, the device last.

A pyramid is a list of 1..8 levels.  The hidden maps ``hs[l]`` are logical (B, C, H_l, W_l) 16-bit tensors in
channels_last MEMORY (``t.permute(0, 2, 3, 1)`` is contiguous) — what the conv units hand on; so are the outputs
``cls[l]`` (B, A, H_l, W_l) and ``reg[l]`` (B, 4A, H_l, W_l), channel order ``a`` and ``4a + j``, and the gradient
``dh[l]``.  A cotangent that is not channels_last memory of the compute dtype — an NCHW tensor handed to ``.backward``,
another float dtype — is brought there by ONE copy (``cotangents``); a 1-channel map, whose strides say nothing, is
taken as it is when its memory is dense.  The packed weights are ``w_fwd`` (Op, C) and ``w_dgrad`` (C, Kp) of
``pack_pred_weight``: the stacked weight, first the A cls rows, then the 4A reg rows, zero padded to Op = 5A rounded up
to 16 and Kp = 5A rounded up to 32.  Parameters, biases and their gradients are float32.

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_dense_head.py`` puts
THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import integer, on_device, tensor
from .deconv_ops import _nhwc
from .ops import BF16, F16, _aligned_ws, _ptr, _workspace, dtype_code  # noqa: F401  (_workspace: swapped by the guard)

F32 = torch.float32
_16 = (BF16, F16)
FWD, DGRAD, WGRAD = 0, 1, 2
MAX_LEVELS, MAX_A, MAX_C, MAX_ROWS = _lib.PRED_MAX_LEVELS, 12, 512, (1 << 31) - 1


def _pad(n, to):
    return (n + to - 1) // to * to


def _channels(C):
    C = integer(C, "C", 64, MAX_C)
    if C % 64:
        raise ValueError("C must be a multiple of 64 in 64..%d, got %d" % (MAX_C, C))
    return C


def _anchors(A):
    return integer(A, "A", 1, MAX_A)


def _levels(ts, name):
    if not isinstance(ts, (list, tuple)) or not 1 <= len(ts) <= MAX_LEVELS:
        raise ValueError("%s must be a list of 1..%d levels, got %s" % (
            name, MAX_LEVELS, len(ts) if isinstance(ts, (list, tuple)) else type(ts).__name__))
    return list(ts)


def _hidden(hs, name="hs"):
    """The hidden maps: -> (list, dtype, B, C, [(H, W)]).  One dtype, one batch size, one channel count."""
    hs = _levels(hs, name)
    B, C, H, W = _nhwc(hs[0], "%s[0]" % name, _16, ("B", "C", "H", "W"))
    C = _channels(C)
    dtype = hs[0].dtype
    sizes = []
    for l, h in enumerate(hs):
        _, _, H, W = _nhwc(h, "%s[%d]" % (name, l), dtype, (B, C, "H", "W"))
        integer(B * H * W, "%s[%d]: B*H*W" % (name, l), 0, MAX_ROWS)
        sizes.append((H, W))
    return hs, dtype, B, C, sizes


def _same_count(ts, name, n):
    ts = _levels(ts, name)
    if len(ts) != n:
        raise ValueError("%s must have one entry per level (%d), got %d" % (name, n, len(ts)))
    return ts


def cotangents(gs, name, dtype, B, ch, sizes):
    """Every ``gs[l]`` as a (B, ch, H_l, W_l) tensor of ``dtype`` in channels_last memory: itself where it already is
    one, else one copy.  Shapes are checked, layouts and float dtypes are free."""
    gs = _same_count(gs, name, len(sizes))
    out = []
    for l, (g, (H, W)) in enumerate(zip(gs, sizes)):
        if not isinstance(g, torch.Tensor) or tuple(g.shape) != (B, ch, H, W) or not g.is_floating_point():
            raise ValueError("%s[%d] must be a floating (%d, %d, %d, %d) tensor, got %s" % (
                name, l, B, ch, H, W, "%s %s" % (g.dtype, tuple(g.shape)) if torch.is_tensor(g) else type(g).__name__))
        if g.dtype != dtype or not g.permute(0, 2, 3, 1).is_contiguous():
            c = torch.empty((B, H, W, ch), dtype=dtype, device=g.device).permute(0, 3, 1, 2)
            c.copy_(g)
            g = c
        out.append(g)
    return out


def _table(hs, cls, reg, dhs, rows):
    n = len(hs)
    arr = (_lib.PredLevel * n)()
    for l in range(n):
        arr[l].h = hs[l].data_ptr()
        arr[l].cls = cls[l].data_ptr()
        arr[l].reg = reg[l].data_ptr()
        arr[l].dh = dhs[l].data_ptr() if dhs is not None else None
        arr[l].rows = rows[l]
    return arr


def _rows(rows):
    rows = [integer(r, "rows[%d]" % l, 0, MAX_ROWS) for l, r in enumerate(_levels(rows, "rows"))]
    return rows, (ctypes.c_int64 * len(rows))(*rows)


class PredPlan(object):
    """What ``tdn_pred_plan`` answered (host side)."""
    __slots__ = ("rows_per_workgroup", "workgroups", "slices", "rows_per_slice", "launches", "Op", "Kp", "channel_tiles",
                 "lds_bytes", "slab_bytes", "workspace_bytes")


def pred_plan(kind, rows, C, A):
    """Host only: the decomposition of one product (kind FWD / DGRAD / WGRAD) over levels of ``rows[l]`` = B * H_l * W_l
    rows.  Refusals of the library are ValueErrors."""
    rows, arr = _rows(rows)
    out = (ctypes.c_int32 * 16)()
    if _lib.load().tdn_pred_plan(int(kind), arr, len(rows), int(C), int(A), out) != 0:
        _lib.ws_bytes(-1, "pred_plan")
    pl = PredPlan()
    (pl.rows_per_workgroup, pl.workgroups, pl.slices, pl.rows_per_slice, pl.launches, pl.Op, pl.Kp, pl.channel_tiles,
     pl.lds_bytes) = list(out)[:9]
    pl.slab_bytes, pl.workspace_bytes = _lib.size_word(out, 12), _lib.size_word(out, 14)
    return pl


def _weight(w, name, ch, C):
    """A (ch, C) or (ch, C, 1, 1) float32 parameter of any strides -> (stride of a row, stride of a channel)."""
    if isinstance(w, torch.Tensor) and w.dim() == 4:
        tensor(w, name, F32, (ch, C, 1, 1), contiguous=False)
    else:
        tensor(w, name, F32, (ch, C), contiguous=False)
    return w.stride(0), w.stride(1)


def pack_pred_weight(w_cls, w_reg, want_dgrad=True, dtype=BF16, out=None):
    """float32 ``w_cls`` (A, C[, 1, 1]) and ``w_reg`` (4A, C[, 1, 1]), any strides -> (w_fwd (Op, C), w_dgrad (C, Kp) or
    None) in ``dtype``, by one launch.  ``out``: the pair of an earlier call, overwritten in place."""
    if not isinstance(w_cls, torch.Tensor) or w_cls.dim() not in (2, 4):
        tensor(w_cls, "w_cls", F32, ("A", "C"), contiguous=False)
    A, C = _anchors(w_cls.shape[0]), _channels(w_cls.shape[1])
    cs = _weight(w_cls, "w_cls", A, C)
    rs = _weight(w_reg, "w_reg", 4 * A, C)
    code = dtype_code(dtype)
    Op, Kp = _pad(5 * A, 16), _pad(5 * A, 32)
    if out is not None:
        w_fwd, w_dgrad = out
        tensor(w_fwd, "out[0]", dtype, (Op, C))
        if want_dgrad:
            tensor(w_dgrad, "out[1]", dtype, (C, Kp))
    on_device([("w_cls", w_cls), ("w_reg", w_reg)] +
              ([("out[0]", out[0]), ("out[1]", out[1] if want_dgrad else None)] if out else []))
    if out is None:
        w_fwd = torch.empty((Op, C), dtype=dtype, device=w_cls.device)
        w_dgrad = torch.empty((C, Kp), dtype=dtype, device=w_cls.device) if want_dgrad else None
    if not want_dgrad:
        w_dgrad = None
    _lib.check(_lib.load().tdn_pack_pred_weight(_ptr(w_cls), cs[0], cs[1], _ptr(w_reg), rs[0], rs[1], A, C, _ptr(w_fwd),
                                                _ptr(w_dgrad), code, _lib.stream_ptr()), "tdn_pack_pred_weight")
    return w_fwd, w_dgrad


def _rows_of(B, sizes):
    return [B * H * W for H, W in sizes]


def pred_fwd(hs, w_fwd, bias_cls, bias_reg):
    """-> (cls, reg): lists of (B, A, H_l, W_l) and (B, 4A, H_l, W_l) tensors in ``hs``'s dtype, channels_last memory,
    ``cls_l = h_l . w_cls^T + bias_cls`` and ``reg_l = h_l . w_reg^T + bias_reg`` for all levels in one launch.
    ``bias_cls`` (A,) and ``bias_reg`` (4A,) float32."""
    hs, dtype, B, C, sizes = _hidden(hs)
    A = _anchors(tensor(bias_cls, "bias_cls", F32, ("A",))[0])
    tensor(bias_reg, "bias_reg", F32, (4 * A,))
    tensor(w_fwd, "w_fwd", dtype, (_pad(5 * A, 16), C))
    on_device([("hs[%d]" % l, h) for l, h in enumerate(hs)] + [("w_fwd", w_fwd), ("bias_cls", bias_cls),
                                                               ("bias_reg", bias_reg)])
    dev = hs[0].device
    cls = [torch.empty((B, H, W, A), dtype=dtype, device=dev) for H, W in sizes]
    reg = [torch.empty((B, H, W, 4 * A), dtype=dtype, device=dev) for H, W in sizes]
    arr = _table(hs, cls, reg, None, _rows_of(B, sizes))
    _lib.check(_lib.load().tdn_pred_fwd(arr, len(hs), _ptr(w_fwd), _ptr(bias_cls), _ptr(bias_reg), C, A,
                                        dtype_code(dtype), _lib.stream_ptr()), "tdn_pred_fwd")
    return [t.permute(0, 3, 1, 2) for t in cls], [t.permute(0, 3, 1, 2) for t in reg]


def _grads(hs, g_cls, g_reg):
    hs, dtype, B, C, sizes = _hidden(hs)
    g_cls = _same_count(g_cls, "g_cls", len(hs))
    A = _anchors(g_cls[0].shape[1] if torch.is_tensor(g_cls[0]) and g_cls[0].dim() == 4 else 0)
    g_cls = cotangents(g_cls, "g_cls", dtype, B, A, sizes)
    g_reg = cotangents(g_reg, "g_reg", dtype, B, 4 * A, sizes)
    return hs, dtype, B, C, sizes, A, g_cls, g_reg


def pred_dgrad(g_cls, g_reg, w_dgrad, hs):
    """-> dh: list of (B, C, H_l, W_l) tensors, channels_last memory: ``g_cls_l . w_cls + g_reg_l . w_reg`` summed in
    fp32 and rounded once, zero where ``hs[l] <= 0`` (the hidden maps are the ReLU's own output), all levels in one
    launch.  The cotangents are read where they lie."""
    hs, dtype, B, C, sizes, A, g_cls, g_reg = _grads(hs, g_cls, g_reg)
    tensor(w_dgrad, "w_dgrad", dtype, (C, _pad(5 * A, 32)))
    on_device([("hs[%d]" % l, h) for l, h in enumerate(hs)] + [("g_cls[%d]" % l, g) for l, g in enumerate(g_cls)] +
              [("g_reg[%d]" % l, g) for l, g in enumerate(g_reg)] + [("w_dgrad", w_dgrad)])
    dhs = [torch.empty((B, H, W, C), dtype=dtype, device=hs[0].device) for H, W in sizes]
    arr = _table(hs, g_cls, g_reg, dhs, _rows_of(B, sizes))
    _lib.check(_lib.load().tdn_pred_dgrad(arr, len(hs), _ptr(w_dgrad), C, A, dtype_code(dtype), _lib.stream_ptr()),
               "tdn_pred_dgrad")
    return [t.permute(0, 3, 1, 2) for t in dhs]


def pred_wgrad(hs, g_cls, g_reg):
    """-> (dw_cls (A, C, 1, 1), dbias_cls (A,), dw_reg (4A, C, 1, 1), dbias_reg (4A,)), float32: the sums over the rows
    of all levels of ``g^T h`` and of ``g``, cut into slices that depend on the shapes alone and added in slice order
    (two launches; the same bits on every run).  An empty batch gives zeros."""
    hs, dtype, B, C, sizes, A, g_cls, g_reg = _grads(hs, g_cls, g_reg)
    on_device([("hs[%d]" % l, h) for l, h in enumerate(hs)] + [("g_cls[%d]" % l, g) for l, g in enumerate(g_cls)] +
              [("g_reg[%d]" % l, g) for l, g in enumerate(g_reg)])
    dev = hs[0].device
    dwc = torch.empty((A, C, 1, 1), dtype=F32, device=dev)
    dwr = torch.empty((4 * A, C, 1, 1), dtype=F32, device=dev)
    dbc = torch.empty((A,), dtype=F32, device=dev)
    dbr = torch.empty((4 * A,), dtype=F32, device=dev)
    rows = _rows_of(B, sizes)
    nbytes = _lib.ws_bytes(_lib.load().tdn_pred_workspace_bytes(WGRAD, (ctypes.c_int64 * len(rows))(*rows), len(rows), C,
                                                                A), "pred workspace")
    ws, wp = _aligned_ws(nbytes, dev) if nbytes else (None, None)
    arr = _table(hs, g_cls, g_reg, None, rows)
    _lib.check(_lib.load().tdn_pred_wgrad(arr, len(hs), _ptr(dwc), _ptr(dbc), _ptr(dwr), _ptr(dbr), C, A, wp, nbytes,
                                          dtype_code(dtype), _lib.stream_ptr()), "tdn_pred_wgrad")
    return dwc, dbc, dwr, dbr
