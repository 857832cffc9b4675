"""Host wrappers of the CARAFE kernels (csrc/carafe.hip), written in the vocabulary of ``_args.py``
(DESIGN.md §5e): every dtype, layout and limit is checked here, before any launch (ValueError that names the argument) —
dtypes, layouts and sizes first, so that those refusals need no GPU, the device last.

``x`` is a logical (N, C, H, W) 16-bit tensor in channels_last MEMORY, read in place; so are ``out``, its cotangent ``gout``,
``addend`` — all (N, C, Ho, Wo) with ``out_size`` = (Ho, Wo) — and ``dx``.  The reassembly weights come as exactly one of

  ``masks``   (N, g k^2, sH, sW): the normalised weights, float32 or the compute dtype;
  ``logits``  (N, g k^2 s^2, H, W): the content encoder's output, channel ``(gi k^2 + t) s^2 + dy s + dx``
              (``F.pixel_shuffle``'s rule); the kernels apply the softmax over the k^2 taps themselves,

in NHWC memory with a PIXEL PITCH (``deform_ops._pitched``): channel stride 1 and any number >= their channel count of
elements between neighbouring pixels.  Their gradient comes back in the same dtype, layout and pitch.  No kernel needs
a workspace.

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_carafe.py`` puts THIS
module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from ._args import CODES, integer, on_device
from .deconv_ops import _nhwc
from .deform_ops import _pitched
from .ops import BF16, F16, _aligned_ws, _ptr, _workspace, dtype_code  # noqa: F401  (_workspace: swapped by the guard)

F32 = torch.float32
_16 = (BF16, F16)
MAX_HW, MAX_PIXELS, MAX_WEIGHT_CHANNELS = 32766, 1 << 30, 1024


class Geometry(object):
    """One checked CARAFE shape: N, C, H, W, k, g, s, sH, sW and the cropped output size Ho, Wo."""
    __slots__ = ("N", "C", "H", "W", "k", "g", "s", "sH", "sW", "Ho", "Wo")

    def channels(self, logits):
        return self.g * self.k * self.k * (self.s * self.s if logits else 1)


def geometry(N, C, H, W, kernel_size, group_size, scale_factor, out_size=None):
    """The supported geometry or a ValueError: kernel_size odd in 1..7, scale_factor in 1..4, group_size dividing C (a
    multiple of 64) into multiples of 8, group_size * kernel_size^2 * scale_factor^2 <= 1024, ``out_size`` within
    (sH - s + 1 .. sH, sW - s + 1 .. sW).  Needs no device."""
    q = Geometry()
    q.k = integer(kernel_size, "kernel_size", 1, 7)
    if q.k % 2 == 0:
        raise ValueError("kernel_size must be odd, got %d" % q.k)
    q.s = integer(scale_factor, "scale_factor", 1, 4)
    q.g = integer(group_size, "group_size", 1)
    if q.g * q.k * q.k * q.s * q.s > MAX_WEIGHT_CHANNELS:
        raise ValueError("group_size * kernel_size^2 * scale_factor^2 must be at most %d, got %d" % (
            MAX_WEIGHT_CHANNELS, q.g * q.k * q.k * q.s * q.s))
    q.N, q.H, q.W = integer(N, "N", 1), integer(H, "H", 1, MAX_HW), integer(W, "W", 1, MAX_HW)
    q.C = integer(C, "C", 1)
    if q.C % 64:
        raise ValueError("C must be a multiple of 64, got %d" % q.C)
    if q.C % q.g or (q.C // q.g) % 8:
        raise ValueError("group_size must divide C = %d into multiples of 8 channels, got %d" % (q.C, q.g))
    q.sH, q.sW = q.H * q.s, q.W * q.s
    integer(q.N * q.sH * q.sW, "N*sH*sW", 1, MAX_PIXELS - 1)
    if out_size is None:
        q.Ho, q.Wo = q.sH, q.sW
    else:
        if not isinstance(out_size, (tuple, list, torch.Size)) or len(out_size) != 2:
            raise ValueError("out_size must be (Ho, Wo), got %r" % (out_size,))
        q.Ho = integer(out_size[0], "out_size[0]", q.sH - q.s + 1, q.sH)
        q.Wo = integer(out_size[1], "out_size[1]", q.sW - q.s + 1, q.sW)
    return q


def _weights(q, dtype, masks, logits):
    """Exactly one of ``masks`` / ``logits`` -> (tensor, pitch, is_logits)."""
    if (masks is None) == (logits is None):
        raise ValueError("exactly one of masks and logits must be given")
    if logits is not None:
        return logits, _pitched(logits, "logits", (F32, dtype), q.N, q.channels(True), q.H, q.W), True
    return masks, _pitched(masks, "masks", (F32, dtype), q.N, q.channels(False), q.sH, q.sW), False


def _desc(q, dtype, x, w, pitch, is_logits, addend=None):
    d = _lib.CarafeDesc()
    d.x = x.data_ptr() if x is not None else None
    d.weights, d.weight_pitch, d.weight_dtype = w.data_ptr(), pitch, CODES[w.dtype]
    d.addend = addend.data_ptr() if addend is not None else None
    d.N, d.H, d.W, d.C = q.N, q.H, q.W, q.C
    d.kernel_size, d.group_size, d.scale_factor = q.k, q.g, q.s
    d.out_h, d.out_w = q.Ho, q.Wo
    d.dtype = dtype_code(dtype)
    d.weights_are_logits = 1 if is_logits else 0
    return d


def _x(x):
    return _nhwc(x, "x", _16, ("N", "C", "H", "W"))


def carafe_forward(x, kernel_size, group_size, scale_factor, masks=None, logits=None, out_size=None, addend=None):
    """-> out, logical (N, C, Ho, Wo) in ``x``'s dtype and channels_last memory: ``addend +`` the reassembly of ``x`` by
    the weights, fp32 sums in tap order, rounded once; only the ``out_size`` crop is computed (one launch)."""
    N, C, H, W = _x(x)
    q = geometry(N, C, H, W, kernel_size, group_size, scale_factor, out_size)
    w, pitch, is_logits = _weights(q, x.dtype, masks, logits)
    if addend is not None:
        _nhwc(addend, "addend", x.dtype, (N, C, q.Ho, q.Wo))
    on_device([("x", x), ("logits" if is_logits else "masks", w), ("addend", addend)])
    out = torch.empty((N, q.Ho, q.Wo, C), dtype=x.dtype, device=x.device)
    d = _desc(q, x.dtype, x, w, pitch, is_logits, addend)
    _lib.check(_lib.load().tdn_carafe_forward(ctypes.byref(d), _ptr(out), _lib.stream_ptr()), "tdn_carafe_forward")
    return out.permute(0, 3, 1, 2)


def _gout(gout, in_shape):
    if not isinstance(in_shape, (tuple, list, torch.Size)) or len(in_shape) != 4:
        raise ValueError("in_shape must be (N, C, H, W), got %r" % (in_shape,))
    N, C, H, W = (int(v) for v in in_shape)
    gN, gC, Ho, Wo = _nhwc(gout, "gout", _16, (N, C, "Ho", "Wo"))
    return N, C, H, W, (Ho, Wo)


def carafe_feature_grad(gout, in_shape, kernel_size, group_size, scale_factor, masks=None, logits=None):
    """-> dx, logical ``in_shape`` = (N, C, H, W) in channels_last memory and ``gout``'s dtype; ``gout`` (N, C, Ho, Wo) is
    the cotangent of the (cropped) output.  Gather form: every element one thread's fp32 sum in a fixed order, rounded
    once (one launch, no atomics; the same bits on every run)."""
    N, C, H, W, out_size = _gout(gout, in_shape)
    q = geometry(N, C, H, W, kernel_size, group_size, scale_factor, out_size)
    w, pitch, is_logits = _weights(q, gout.dtype, masks, logits)
    on_device([("gout", gout), ("logits" if is_logits else "masks", w)])
    dx = torch.empty((N, H, W, C), dtype=gout.dtype, device=gout.device)
    d = _desc(q, gout.dtype, None, w, pitch, is_logits)
    _lib.check(_lib.load().tdn_carafe_feature_grad(ctypes.byref(d), _ptr(gout), _ptr(dx), _lib.stream_ptr()),
               "tdn_carafe_feature_grad")
    return dx.permute(0, 3, 1, 2)


def _like_pitched(t, pitch):
    """An uninitialised tensor of ``t``'s logical shape and pitch; the channels of a pixel past ``t``'s are zero."""
    N, ch, Ho, Wo = t.shape
    if pitch == ch:
        return torch.empty((N, Ho, Wo, ch), dtype=t.dtype, device=t.device).permute(0, 3, 1, 2)
    return torch.zeros((N, Ho, Wo, pitch), dtype=t.dtype, device=t.device).permute(0, 3, 1, 2)[:, :ch]


def carafe_mask_grad(gout, x, kernel_size, group_size, scale_factor, masks=None, logits=None, out=None):
    """-> the gradient of ``masks`` (or, through the softmax, of ``logits``) in the operand's own dtype, layout and pitch
    (one launch).  ``out``: a tensor of the operand's shape, dtype and strides to write into."""
    N, C, H, W = _x(x)
    gN, gC, Ho, Wo = _nhwc(gout, "gout", x.dtype, (N, C, "Ho", "Wo"))
    q = geometry(N, C, H, W, kernel_size, group_size, scale_factor, (Ho, Wo))
    w, pitch, is_logits = _weights(q, x.dtype, masks, logits)
    name = "logits" if is_logits else "masks"
    if out is not None and _pitched(out, "out", (w.dtype,), *w.shape) != pitch:
        raise ValueError("out must have the pitch of %s" % name)
    on_device([("x", x), ("gout", gout), (name, w), ("out", out)])
    dw = _like_pitched(w, pitch) if out is None else out
    d = _desc(q, x.dtype, x, w, pitch, is_logits)
    _lib.check(_lib.load().tdn_carafe_mask_grad(ctypes.byref(d), _ptr(gout), _ptr(dw), _lib.stream_ptr()),
               "tdn_carafe_mask_grad")
    return dw
