"""Host wrappers of the fully connected layers (csrc/linear.hip), written in the vocabulary of
``_args.py``: every dtype, layout and limit is checked here, before any launch (ValueError that names
the argument) — dtypes, layouts and sizes first, so that those refusals need no GPU, the device last.

Operands are 2-D: ``x`` (M, K) and the cotangent ``g`` (M, O) contiguous 16-bit tensors of one dtype, the packed weights
``w_fwd`` (Op, K) and ``w_dgrad`` (K, Op) of ``pack_linear_weight`` (Op = O rounded up to 64), bias and gradients
float32.  A channels_last RoI feature buffer is such an ``x`` through the pack's column permutation (``C``).

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_linear.py`` puts THIS
module under the guard of ``tests/guard_util.py``.
"""

import torch

from . import _lib
from ._args import integer, number, on_device, tensor
from .ops import BF16, F16, _aligned_ws, _ptr, _workspace, dtype_code  # noqa: F401  (_workspace: swapped by the guard)

F32 = torch.float32
_16 = (BF16, F16)
FWD, DGRAD, WGRAD = 0, 1, 2
MAX_M, MAX_O, MAX_K = 1 << 18, 65536, 1 << 20


def _pad64(n):
    return (n + 63) // 64 * 64


def _dims(M, O, K):
    M = integer(M, "M", 0, MAX_M)
    O = integer(O, "O", 1, MAX_O)
    K = integer(K, "K", 64, MAX_K)
    if K % 64:
        raise ValueError("K must be a multiple of 64, got %d" % K)
    return M, O, K


def _splits(splits, kind, M, K):
    hi = max(1, (M + 63) // 64 if kind == WGRAD else K // 64)
    return integer(splits, "splits", 0, hi)


def _perm(C, K):
    C = K if C is None else integer(C, "C", 1, K)
    if K % C or (C != K and C % 8):
        raise ValueError("C must divide K=%d and be a multiple of 8 (or equal K), got %d" % (K, C))
    return C


class LinearPlan(object):
    """What ``tdn_linear_plan`` answered (host side)."""
    __slots__ = ("bm", "bn", "bk", "tiles_r", "tiles_c", "tiles", "slices", "chunks_per_slice", "chunks", "workgroups",
                 "launches", "pad", "conv", "slab_bytes", "workspace_bytes")


def linear_plan(kind, M, O, K, splits=0):
    """Host only: the decomposition of one product (kind FWD / DGRAD / WGRAD).  Refusals of the library are ValueErrors."""
    pl = LinearPlan()
    flags = _lib.gemm128_plan(pl, _lib.load().tdn_linear_plan, (kind, M, O, K, splits), "linear_plan")
    pl.pad, pl.conv = flags & 1, flags >> 1
    return pl


def _ws(kind, M, O, K, splits, dev):
    nbytes = _lib.ws_bytes(_lib.load().tdn_linear_workspace_bytes(kind, M, O, K, splits), "linear workspace")
    if nbytes == 0:
        return None, None, 0
    ws, wp = _aligned_ws(nbytes, dev)
    return ws, wp, nbytes


def pack_linear_weight(w, C=None, want_dgrad=True, dtype=BF16, out=None):
    """float32 (O, K) weight (any strides) -> (w_fwd (Op, K), w_dgrad (K, Op) or None) in ``dtype``; ``C``: the channel
    count of a channels_last (R, S, S, C) input whose logical flattening the weight's columns follow (None: as they
    are).  ``out``: the pair of an earlier call, overwritten in place."""
    O, K = tensor(w, "weight", F32, ("O", "K"), contiguous=False)
    _, O, K = _dims(0, O, K)
    C = _perm(C, K)
    code = dtype_code(dtype)
    Op = _pad64(O)
    if out is not None:
        w_fwd, w_dgrad = out
        tensor(w_fwd, "out[0]", dtype, (Op, K))
        if want_dgrad:
            tensor(w_dgrad, "out[1]", dtype, (K, Op))
    on_device([("weight", w)] + ([("out[0]", out[0]), ("out[1]", out[1] if want_dgrad else None)] if out else []))
    if out is None:
        w_fwd = torch.empty((Op, K), dtype=dtype, device=w.device)
        w_dgrad = torch.empty((K, Op), dtype=dtype, device=w.device) if want_dgrad else None
    if not want_dgrad:
        w_dgrad = None
    _lib.check(_lib.load().tdn_pack_linear_weight(_ptr(w), w.stride(0), w.stride(1), O, K, C, _ptr(w_fwd), _ptr(w_dgrad),
                                                  code, _lib.stream_ptr()), "tdn_pack_linear_weight")
    return w_fwd, w_dgrad


def linear_fwd(x, w_fwd, O, bias=None, relu=False, out_f32=False, splits=0):
    """y (M, O) = act(x @ w^T + bias): ``x`` (M, K), ``w_fwd`` (Op, K) packed, ``bias`` float32 (O,) or None; y in
    ``x``'s dtype, float32 with ``out_f32``."""
    M, K = tensor(x, "x", _16, ("M", "K"))
    M, O, K = _dims(M, O, K)
    tensor(w_fwd, "w_fwd", x.dtype, (_pad64(O), K))
    if bias is not None:
        tensor(bias, "bias", F32, (O,))
    splits = _splits(splits, FWD, M, K)
    on_device([("x", x), ("w_fwd", w_fwd), ("bias", bias)])
    y = torch.empty((M, O), dtype=F32 if out_f32 else x.dtype, device=x.device)
    ws, wp, nbytes = _ws(FWD, M, O, K, splits, x.device)
    _lib.check(_lib.load().tdn_linear_fwd(_ptr(x), K, _ptr(w_fwd), _ptr(bias), _ptr(y), O, M, O, K, 1 if relu else 0,
                                          1 if out_f32 else 0, splits, wp, nbytes, dtype_code(x.dtype),
                                          _lib.stream_ptr()), "tdn_linear_fwd")
    return y


def linear_dgrad(g, w_dgrad, mask_src=None, splits=0):
    """dx (M, K) = g @ w, zero where ``mask_src`` (M, K) <= 0: ``g`` (M, O), ``w_dgrad`` (K, Op) packed."""
    M, O = tensor(g, "g", _16, ("M", "O"))
    K = tensor(w_dgrad, "w_dgrad", g.dtype, ("K", _pad64(max(O, 1))))[0]
    M, O, K = _dims(M, O, K)
    if mask_src is not None:
        tensor(mask_src, "mask_src", g.dtype, (M, K))
    splits = _splits(splits, DGRAD, M, K)
    on_device([("g", g), ("w_dgrad", w_dgrad), ("mask_src", mask_src)])
    dx = torch.empty((M, K), dtype=g.dtype, device=g.device)
    ws, wp, nbytes = _ws(DGRAD, M, O, K, splits, g.device)
    _lib.check(_lib.load().tdn_linear_dgrad(_ptr(g), O, _ptr(w_dgrad), _ptr(mask_src), K, _ptr(dx), K, M, O, K, splits,
                                            wp, nbytes, dtype_code(g.dtype), _lib.stream_ptr()), "tdn_linear_dgrad")
    return dx


def linear_wgrad(x, g, C=None, dw=None, dbias=None, beta=0.0, want_dbias=True, splits=0):
    """-> (dw float32 (O, K) in the weight's logical column order, dbias float32 (O,) or None): beta * old + g^T @ x and
    beta * old + column sums of g.  ``dw`` / ``dbias``: buffers to write (and, with beta != 0, to accumulate into);
    ``want_dbias=False`` skips the bias gradient."""
    M, K = tensor(x, "x", _16, ("M", "K"))
    O = tensor(g, "g", x.dtype, (M, "O"))[1]
    M, O, K = _dims(M, O, K)
    C = _perm(C, K)
    beta = number(beta, "beta")
    if dw is not None:
        tensor(dw, "dw", F32, (O, K))
    elif beta != 0.0:
        raise ValueError("dw must be given when beta != 0")
    if not want_dbias:
        dbias = None
    elif dbias is not None:
        tensor(dbias, "dbias", F32, (O,))
    elif beta != 0.0:
        raise ValueError("dbias must be given when beta != 0 (or want_dbias=False)")
    splits = _splits(splits, WGRAD, M, K)
    on_device([("x", x), ("g", g), ("dw", dw), ("dbias", dbias)])
    if dw is None:
        dw = torch.empty((O, K), dtype=F32, device=x.device)
    if want_dbias and dbias is None:
        dbias = torch.empty((O,), dtype=F32, device=x.device)
    ws, wp, nbytes = _ws(WGRAD, M, O, K, splits, x.device)
    _lib.check(_lib.load().tdn_linear_wgrad(_ptr(x), K, _ptr(g), O, _ptr(dw), _ptr(dbias), beta, M, O, K, C, splits, wp,
                                            nbytes, dtype_code(x.dtype), _lib.stream_ptr()), "tdn_linear_wgrad")
    return dw, dbias


def linear_relu_bwd(g, y):
    """g where y > 0 else 0: the cotangent behind a layer's own ReLU.  ``g`` (M, O) 16-bit, ``y`` the stored output, in
    ``g``'s dtype or float32."""
    M, O = tensor(g, "g", _16, ("M", "O"))
    tensor(y, "y", (g.dtype, F32), (M, O))
    integer(M, "M", 0, MAX_M)
    integer(O, "O", 1, MAX_O)
    on_device([("g", g), ("y", y)])
    out = torch.empty((M, O), dtype=g.dtype, device=g.device)
    _lib.check(_lib.load().tdn_linear_relu_bwd(_ptr(g), _ptr(y), 1 if y.dtype == F32 else 0, _ptr(out), M, O,
                                               dtype_code(g.dtype), _lib.stream_ptr()), "tdn_linear_relu_bwd")
    return out
