"""Host wrappers of the 2x2 stride-2 transposed convolution (csrc/deconv.hip), written in the vocabulary
of ``_args.py``: every dtype, layout and limit is checked here, before any launch (ValueError that names
the argument) — dtypes, layouts and sizes first, so that those refusals need no GPU, the device last.

Activations are logical (R, C, H, W) 16-bit tensors in channels_last MEMORY — what ``roi_align`` and the conv modules
hand on — i.e. ``t.permute(0, 2, 3, 1)`` is contiguous: ``x`` (R, Cin, H, W), ``y`` and its cotangent ``g``
(R, Cout, 2H, 2W).  The packed weights are ``w_fwd`` (4 Cout, Cin), row (a * 2 + b) * Cout + o, and ``w_dgrad``
(Cin, 4 Cout) of ``pack_deconv_weight``; weight (Cin, Cout, 2, 2), bias and the gradients are float32.

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_deconv.py`` puts THIS
module under the guard of ``tests/guard_util.py``.
"""

import torch

from . import _lib
from ._args import integer, number, on_device, tensor
from .ops import BF16, F16, _aligned_ws, _ptr, _workspace, dtype_code  # noqa: F401  (_workspace: swapped by the guard)

F32 = torch.float32
_16 = (BF16, F16)
FWD, DGRAD, WGRAD = 0, 1, 2
MAX_C, MAX_PIX, MAX_OUT = 1 << 16, 1 << 29, 1 << 31


def _channels(n, name):
    n = integer(n, name, 64, MAX_C)
    if n % 64:
        raise ValueError("%s must be a multiple of 64, got %d" % (name, n))
    return n


def _nhwc(t, name, dtype, shape):
    """``t`` is a logical (R, C, H, W) tensor of ``dtype`` in channels_last memory; ``shape`` = (R, C, H, W) with None /
    a string for a free size.  Returns its logical shape."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        tensor(t, name, dtype, shape)            # raises with the usual message
    R, C, H, W = shape
    try:
        R, H, W, C = tensor(t.permute(0, 2, 3, 1), name, dtype, (R, H, W, C))
    except ValueError:
        want = ", ".join(str(s) if isinstance(s, int) else "*" for s in shape)
        names = " / ".join(str(d).replace("torch.", "") for d in (dtype if isinstance(dtype, tuple) else (dtype,)))
        raise ValueError("%s must be a %s (%s) tensor in channels_last memory (NHWC), got %s %s with strides %s" % (
            name, names, want, str(t.dtype).replace("torch.", ""), tuple(t.shape), tuple(t.stride())))
    return R, C, H, W


def _geometry(R, H, W, Cin, Cout):
    R = integer(R, "R", 0)
    H = integer(H, "H", 1)
    W = integer(W, "W", 1)
    Cin, Cout = _channels(Cin, "Cin"), _channels(Cout, "Cout")
    M = R * H * W
    if M >= MAX_PIX or 4 * M * Cout >= MAX_OUT or M * Cin >= MAX_OUT:
        raise ValueError("x is too large: R*H*W=%d must be below 2^29, R*2H*2W*Cout and R*H*W*Cin below 2^31" % M)
    return R, H, W, Cin, Cout


def _splits(splits, kind, M):
    return integer(splits, "splits", 0, max(1, (M + 63) // 64) if kind == WGRAD else 1)


class DeconvPlan(object):
    """What ``tdn_deconv2x2_plan`` answered (host side)."""
    __slots__ = ("bm", "bn", "bk", "tiles_r", "tiles_c", "tiles", "slices", "chunks_per_slice", "chunks", "workgroups",
                 "launches", "slab_bytes", "workspace_bytes")


def deconv2x2_plan(kind, R, H, W, Cin, Cout, splits=0):
    """Host only: the decomposition of one product (kind FWD / DGRAD / WGRAD).  Refusals of the library are ValueErrors."""
    pl = DeconvPlan()
    _lib.gemm128_plan(pl, _lib.load().tdn_deconv2x2_plan, (kind, R, H, W, Cin, Cout, splits), "deconv2x2_plan")
    return pl


def pack_deconv_weight(w, want_dgrad=True, dtype=BF16, out=None):
    """float32 (Cin, Cout, 2, 2) weight (any strides) -> (w_fwd (4 Cout, Cin), w_dgrad (Cin, 4 Cout) or None) in
    ``dtype``.  ``out``: the pair of an earlier call, overwritten in place."""
    Cin, Cout = tensor(w, "weight", F32, ("Cin", "Cout", 2, 2), contiguous=False)[:2]
    Cin, Cout = _channels(Cin, "Cin"), _channels(Cout, "Cout")
    code = dtype_code(dtype)
    if out is not None:
        w_fwd, w_dgrad = out
        tensor(w_fwd, "out[0]", dtype, (4 * Cout, Cin))
        if want_dgrad:
            tensor(w_dgrad, "out[1]", dtype, (Cin, 4 * Cout))
    on_device([("weight", w)] + ([("out[0]", out[0]), ("out[1]", out[1] if want_dgrad else None)] if out else []))
    if out is None:
        w_fwd = torch.empty((4 * Cout, Cin), dtype=dtype, device=w.device)
        w_dgrad = torch.empty((Cin, 4 * Cout), dtype=dtype, device=w.device) if want_dgrad else None
    if not want_dgrad:
        w_dgrad = None
    s = w.stride()
    _lib.check(_lib.load().tdn_pack_deconv2x2_weight(_ptr(w), s[0], s[1], s[2], s[3], Cin, Cout, _ptr(w_fwd),
                                                     _ptr(w_dgrad), code, _lib.stream_ptr()), "tdn_pack_deconv2x2_weight")
    return w_fwd, w_dgrad


def deconv2x2_fwd(x, w_fwd, bias=None, relu=False):
    """y (R, Cout, 2H, 2W) = act(conv_transpose2d(x, weight, bias, stride=2)), channels_last memory, in ``x``'s dtype:
    ``x`` (R, Cin, H, W) channels_last, ``w_fwd`` (4 Cout, Cin) packed, ``bias`` float32 (Cout,) or None."""
    R, Cin, H, W = _nhwc(x, "x", _16, ("R", "Cin", "H", "W"))
    N4 = tensor(w_fwd, "w_fwd", x.dtype, ("4*Cout", Cin))[0]
    if N4 % 4:
        raise ValueError("w_fwd must have 4 * Cout rows, got %d" % N4)
    R, H, W, Cin, Cout = _geometry(R, H, W, Cin, N4 // 4)
    if bias is not None:
        tensor(bias, "bias", F32, (Cout,))
    on_device([("x", x), ("w_fwd", w_fwd), ("bias", bias)])
    y = torch.empty((R, 2 * H, 2 * W, Cout), dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().tdn_deconv2x2_fwd(_ptr(x), _ptr(w_fwd), _ptr(bias), _ptr(y), R, H, W, Cin, Cout,
                                             1 if relu else 0, dtype_code(x.dtype), _lib.stream_ptr()), "tdn_deconv2x2_fwd")
    return y.permute(0, 3, 1, 2)


def deconv2x2_dgrad(g, w_dgrad):
    """dx (R, Cin, H, W), channels_last memory: ``g`` (R, Cout, 2H, 2W) channels_last — already masked by the layer's
    ReLU, if it has one —, ``w_dgrad`` (Cin, 4 Cout) packed."""
    R, Cout, H2, W2 = _nhwc(g, "g", _16, ("R", "Cout", "2H", "2W"))
    if H2 % 2 or W2 % 2 or not H2 or not W2:
        raise ValueError("g must be a (R, Cout, 2H, 2W) tensor with even, positive height and width, got %s" % (tuple(g.shape),))
    Cin = tensor(w_dgrad, "w_dgrad", g.dtype, ("Cin", 4 * Cout))[0]
    R, H, W, Cin, Cout = _geometry(R, H2 // 2, W2 // 2, Cin, Cout)
    on_device([("g", g), ("w_dgrad", w_dgrad)])
    dx = torch.empty((R, H, W, Cin), dtype=g.dtype, device=g.device)
    _lib.check(_lib.load().tdn_deconv2x2_dgrad(_ptr(g), _ptr(w_dgrad), _ptr(dx), R, H, W, Cin, Cout, dtype_code(g.dtype),
                                               _lib.stream_ptr()), "tdn_deconv2x2_dgrad")
    return dx.permute(0, 3, 1, 2)


def deconv2x2_wgrad(x, g, dw=None, dbias=None, beta=0.0, want_dbias=True, splits=0):
    """-> (dw float32 (Cin, Cout, 2, 2), dbias float32 (Cout,) or None): beta * old + the weight gradient and beta * old
    + the sum of ``g`` over its pixels.  ``x`` (R, Cin, H, W) and ``g`` (R, Cout, 2H, 2W) channels_last; ``dw`` /
    ``dbias``: buffers to write (and, with beta != 0, to accumulate into); ``want_dbias=False`` skips the bias gradient."""
    R, Cin, H, W = _nhwc(x, "x", _16, ("R", "Cin", "H", "W"))
    Cout = _nhwc(g, "g", x.dtype, (R, "Cout", 2 * H, 2 * W))[1]
    R, H, W, Cin, Cout = _geometry(R, H, W, Cin, Cout)
    beta = number(beta, "beta")
    if dw is not None:
        tensor(dw, "dw", F32, (Cin, Cout, 2, 2))
    elif beta != 0.0:
        raise ValueError("dw must be given when beta != 0")
    if not want_dbias:
        dbias = None
    elif dbias is not None:
        tensor(dbias, "dbias", F32, (Cout,))
    elif beta != 0.0:
        raise ValueError("dbias must be given when beta != 0 (or want_dbias=False)")
    splits = _splits(splits, WGRAD, R * H * W)
    on_device([("x", x), ("g", g), ("dw", dw), ("dbias", dbias)])
    if dw is None:
        dw = torch.empty((Cin, Cout, 2, 2), dtype=F32, device=x.device)
    if want_dbias and dbias is None:
        dbias = torch.empty((Cout,), dtype=F32, device=x.device)
    nbytes = _lib.ws_bytes(_lib.load().tdn_deconv2x2_workspace_bytes(WGRAD, R, H, W, Cin, Cout, splits),
                           "deconv2x2 workspace")
    ws, wp = _aligned_ws(nbytes, x.device) if nbytes else (None, None)
    _lib.check(_lib.load().tdn_deconv2x2_wgrad(_ptr(x), _ptr(g), _ptr(dw), _ptr(dbias), beta, R, H, W, Cin, Cout, splits,
                                               wp, nbytes, dtype_code(x.dtype), _lib.stream_ptr()), "tdn_deconv2x2_wgrad")
    return dw, dbias
