"""Host wrappers of the deformable-convolution kernels (csrc/deform.hip), written in the vocabulary of
``_args.py``: every dtype, layout and limit is checked here, before any launch (ValueError that names the
argument) — dtypes, layouts and sizes first, so that those refusals need no GPU, the device last.

``x`` is a logical (N, C, H, W) 16-bit tensor in channels_last MEMORY, read in place.  ``offset`` (N, 18 dg, Ho, Wo) and
``mask`` (N, 9 dg, Ho, Wo) are float32 or the compute dtype, NHWC memory with a PIXEL PITCH: channel stride 1 and any
number >= their channel count of elements between neighbouring pixels, so a channel slice of a wider channels_last buffer
(the one output of a ``conv_offset_mask``) is read where it lies.  ``cols`` and its cotangent ``dcol`` are (N, Ho, Wo, 9 C)
contiguous tensors of the compute dtype, K index ``tap * C + channel`` — what ``ops.conv2d_fwd`` takes as a 1x1 conv's
input.  The packed weights are ``w_fwd`` (Cout, 1, 1, 9 C) and ``w_dgrad`` (9 C, 1, 1, Cout) of ``pack_deform_weight``.

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_deform.py`` puts THIS
module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, integer, on_device, tensor
from .deconv_ops import _nhwc
from .ops import BF16, F16, _aligned_ws, _ptr, _workspace, conv_out_size, dtype_code  # noqa: F401  (_workspace: swapped by the guard)

F32 = torch.float32
_16 = (BF16, F16)
MAX_HW, MAX_SAMPLES = 32766, 1 << 30


class Geometry(object):
    """One deformable 3x3 conv's checked shape: N, C, H, W, Ho, Wo, stride, pad (= dilation), dg."""
    __slots__ = ("N", "C", "H", "W", "Ho", "Wo", "stride", "pad", "dg")


def geometry(N, C, H, W, kernel_size=3, stride=1, padding=1, dilation=1, deformable_groups=1, groups=1):
    """The supported geometry or a ValueError: 3x3, groups 1, stride 1 or 2, padding == dilation in 1..32, C a multiple
    of 64 that ``deformable_groups`` divides into multiples of 8.  Needs no device."""
    ks = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
    if ks != (3, 3):
        raise ValueError("kernel_size must be 3, got %r" % (kernel_size,))
    if integer(groups, "groups", 1) != 1:
        raise ValueError("groups must be 1, got %d" % groups)
    stride = integer(stride, "stride", 1, 2)
    padding, dilation = integer(padding, "padding", 0), integer(dilation, "dilation", 1, 32)
    if padding != dilation:
        raise ValueError("padding must equal dilation (a 'same' 3x3 conv), got padding %d, dilation %d" % (
            padding, dilation))
    g = Geometry()
    g.N, g.H, g.W = integer(N, "N", 1), integer(H, "H", 1, MAX_HW), integer(W, "W", 1, MAX_HW)
    g.C = integer(C, "C", 1)
    g.dg = integer(deformable_groups, "deformable_groups", 1)
    if g.C % 64:
        raise ValueError("C must be a multiple of 64, got %d" % g.C)
    if g.C % g.dg or (g.C // g.dg) % 8:
        raise ValueError("deformable_groups must divide C = %d into multiples of 8 channels, got %d" % (g.C, g.dg))
    g.stride, g.pad = stride, padding
    g.Ho, g.Wo = conv_out_size(g.H, 3, stride, padding), conv_out_size(g.W, 3, stride, padding)
    if g.Ho < 1 or g.Wo < 1:
        raise ValueError("the output is empty for a %d x %d input with dilation %d" % (g.H, g.W, dilation))
    integer(g.N * g.Ho * g.Wo * 9 * g.dg, "N*Ho*Wo*9*deformable_groups", 1, MAX_SAMPLES - 1)
    integer(g.N * g.H * g.W, "N*H*W", 1, MAX_SAMPLES - 1)
    return g


def _pitched(t, name, dtypes, N, ch, Ho, Wo):
    """``t``: logical (N, ch, Ho, Wo), channel stride 1, pixels ``pitch >= ch`` elements apart in NHWC order -> pitch"""
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype not in dtypes or tuple(t.shape) != (N, ch, Ho, Wo):
        tensor(t, name, dtypes, (N, ch, Ho, Wo), contiguous=False)
    sn, sc, sh, sw = t.stride()
    pitch = sw if Wo > 1 else (sh // Wo if Ho > 1 else (sn // (Ho * Wo) if N > 1 else ch))
    if pitch < ch or (ch > 1 and sc != 1) or (Wo > 1 and sw != pitch) or (Ho > 1 and sh != Wo * pitch) or \
            (N > 1 and sn != Ho * Wo * pitch):
        raise ValueError("%s must be (%d, %d, %d, %d) in NHWC memory (channel stride 1, one pitch between pixels), got "
                         "strides %s" % (name, N, ch, Ho, Wo, tuple(t.stride())))
    return pitch


def _operands(g, x_dtype, offset, mask):
    dts = (F32, x_dtype)
    op = _pitched(offset, "offset", dts, g.N, 18 * g.dg, g.Ho, g.Wo)
    mp = _pitched(mask, "mask", dts, g.N, 9 * g.dg, g.Ho, g.Wo) if mask is not None else 0
    return op, mp


def _desc(g, dtype, x, offset, op, mask, mp, mask_is_logit):
    d = _lib.DeformDesc()
    d.x = x.data_ptr() if x is not None else None
    d.offset, d.offset_pitch, d.offset_dtype = offset.data_ptr(), op, CODES[offset.dtype]
    if mask is not None:
        d.mask, d.mask_pitch, d.mask_dtype = mask.data_ptr(), mp, CODES[mask.dtype]
    else:
        d.mask_dtype = dtype_code(dtype)
    d.N, d.H, d.W, d.C, d.stride, d.pad, d.deformable_groups = g.N, g.H, g.W, g.C, g.stride, g.pad, g.dg
    d.dtype = dtype_code(dtype)
    d.mask_is_logit = 1 if (mask is not None and mask_is_logit) else 0
    return d


def _x(x):
    return _nhwc(x, "x", _16, ("N", "C", "H", "W"))


def _dcol(dcol, g, dtype):
    tensor(dcol, "dcol", dtype, (g.N, g.Ho, g.Wo, 9 * g.C))


def deform_workspace_bytes(N, H, W, stride=1, padding=1, deformable_groups=1):
    """Host only: the bytes ``deform_input_grad`` needs — records [N][chunks][256] of 16 bytes, then boxes [N][chunks] of
    16 bytes, chunks = ceil(Ho Wo dg 9 / 256), each region rounded up to 256 bytes."""
    return _lib.ws_bytes(_lib.load().tdn_deform_workspace_bytes(int(N), int(H), int(W), int(stride), int(padding),
                                                                int(deformable_groups)), "deform workspace")


def pack_deform_weight(w, want_dgrad=True, dtype=BF16, out=None):
    """float32 ``w`` (Cout, C, 3, 3) of any strides -> (w_fwd (Cout, 1, 1, 9 C), w_dgrad (9 C, 1, 1, Cout) or None) in
    ``dtype`` by one launch, K index ``(3 kh + kw) * C + c``, each element rounded once.  ``out``: the pair of an earlier
    call, overwritten in place."""
    Cout, C = tensor(w, "weight", F32, ("Cout", "C", 3, 3), contiguous=False)[:2]
    if Cout % 64 or C % 64 or not Cout or not C:
        raise ValueError("weight: Cout and C must be multiples of 64, got %d and %d" % (Cout, C))
    code = dtype_code(dtype)
    if out is not None:
        w_fwd, w_dgrad = out
        tensor(w_fwd, "out[0]", dtype, (Cout, 1, 1, 9 * C))
        if want_dgrad:
            tensor(w_dgrad, "out[1]", dtype, (9 * C, 1, 1, Cout))
    on_device([("weight", w)] + ([("out[0]", out[0]), ("out[1]", out[1] if want_dgrad else None)] if out else []))
    if out is None:
        w_fwd = torch.empty((Cout, 1, 1, 9 * C), dtype=dtype, device=w.device)
        w_dgrad = torch.empty((9 * C, 1, 1, Cout), dtype=dtype, device=w.device) if want_dgrad else None
    if not want_dgrad:
        w_dgrad = None
    s = w.stride()
    _lib.check(_lib.load().tdn_pack_deform_weight(_ptr(w), s[0], s[1], s[2], s[3], Cout, C, _ptr(w_fwd), _ptr(w_dgrad),
                                                  code, _lib.stream_ptr()), "tdn_pack_deform_weight")
    return w_fwd, w_dgrad


def deform_sample(x, offset, mask=None, stride=1, padding=1, dilation=1, deformable_groups=1, mask_is_logit=False):
    """-> cols (N, Ho, Wo, 9 C) in ``x``'s dtype: the bilinear samples of every (output pixel, tap, channel), times the
    mask (or its sigmoid with ``mask_is_logit``), rounded once."""
    N, C, H, W = _x(x)
    g = geometry(N, C, H, W, 3, stride, padding, dilation, deformable_groups)
    op, mp = _operands(g, x.dtype, offset, mask)
    on_device([("x", x), ("offset", offset), ("mask", mask)])
    cols = torch.empty((N, g.Ho, g.Wo, 9 * C), dtype=x.dtype, device=x.device)
    d = _desc(g, x.dtype, x, offset, op, mask, mp, mask_is_logit)
    _lib.check(_lib.load().tdn_deform_sample(ctypes.byref(d), _ptr(cols), _lib.stream_ptr()), "tdn_deform_sample")
    return cols


def _like_pitched(t, pitch):
    """An uninitialised tensor of ``t``'s logical shape and pitch; the channels of a pixel past ``t``'s are zero."""
    N, ch, Ho, Wo = t.shape
    if pitch == ch:
        return torch.empty((N, Ho, Wo, ch), dtype=t.dtype, device=t.device).permute(0, 3, 1, 2)
    return torch.zeros((N, Ho, Wo, pitch), dtype=t.dtype, device=t.device).permute(0, 3, 1, 2)[:, :ch]


def deform_coord_grad(dcol, x, offset, mask=None, stride=1, padding=1, dilation=1, deformable_groups=1,
                      mask_is_logit=False, out=None):
    """-> (doffset, dmask or None) from ``dcol`` (N, Ho, Wo, 9 C): the gradients of the offsets and of the mask (of its
    logit with ``mask_is_logit``), in the operands' own dtype, layout and pitch; exact zeros for invalid samples.  ``out``:
    (doffset, dmask) to write into — tensors of the operands' shape, dtype and strides (views of one wider buffer)."""
    N, C, H, W = _x(x)
    g = geometry(N, C, H, W, 3, stride, padding, dilation, deformable_groups)
    op, mp = _operands(g, x.dtype, offset, mask)
    _dcol(dcol, g, x.dtype)
    if out is not None:
        doff, dmsk = out
        if _pitched(doff, "out[0]", (offset.dtype,), N, 18 * g.dg, g.Ho, g.Wo) != op or (
                mask is not None and _pitched(dmsk, "out[1]", (mask.dtype,), N, 9 * g.dg, g.Ho, g.Wo) != mp):
            raise ValueError("out must have the pitch of offset / mask")
    on_device([("x", x), ("offset", offset), ("mask", mask), ("dcol", dcol)] +
              ([("out[0]", out[0]), ("out[1]", out[1] if mask is not None else None)] if out else []))
    if out is None:
        doff = _like_pitched(offset, op)
        dmsk = _like_pitched(mask, mp) if mask is not None else None
    if mask is None:
        dmsk = None
    d = _desc(g, x.dtype, x, offset, op, mask, mp, mask_is_logit)
    _lib.check(_lib.load().tdn_deform_coord_grad(ctypes.byref(d), _ptr(dcol), _ptr(doff), _ptr(dmsk),
                                                 _lib.stream_ptr()), "tdn_deform_coord_grad")
    return doff, dmsk


def deform_input_grad(dcol, offset, mask, in_shape, stride=1, padding=1, dilation=1, deformable_groups=1,
                      mask_is_logit=False):
    """-> dx, logical ``in_shape`` = (N, C, H, W) in channels_last memory and ``dcol``'s dtype: every pixel the fp32 sum
    of ``dcol * mask * corner weight`` over the valid samples' corners that land on it, in sample order, rounded once
    (two launches, no atomics; the same bits on every run)."""
    if not isinstance(in_shape, (tuple, list, torch.Size)) or len(in_shape) != 4:
        raise ValueError("in_shape must be (N, C, H, W), got %r" % (in_shape,))
    N, C, H, W = (int(v) for v in in_shape)
    g = geometry(N, C, H, W, 3, stride, padding, dilation, deformable_groups)
    dtype = dcol.dtype if isinstance(dcol, torch.Tensor) and dcol.dtype in _16 else BF16
    _dcol(dcol, g, _16 if not isinstance(dcol, torch.Tensor) or dcol.dtype not in _16 else dtype)
    op, mp = _operands(g, dtype, offset, mask)
    on_device([("dcol", dcol), ("offset", offset), ("mask", mask)])
    dx = torch.empty((N, H, W, C), dtype=dtype, device=dcol.device)
    nbytes = deform_workspace_bytes(N, H, W, g.stride, g.pad, g.dg)
    ws, wp = _aligned_ws(nbytes, dcol.device)
    d = _desc(g, dtype, None, offset, op, mask, mp, mask_is_logit)
    _lib.check(_lib.load().tdn_deform_input_grad(ctypes.byref(d), _ptr(dcol), _ptr(dx), wp, nbytes, _lib.stream_ptr()),
               "tdn_deform_input_grad")
    return dx.permute(0, 3, 1, 2)
