"""2x2 stride-2 transposed convolution on the HIP path (csrc/deconv.hip): ``conv_transpose2x2`` is
``F.conv_transpose2d(x, weight, bias, stride=2)`` (+ ReLU) with fp32 parameters, 16-bit operands and fp32 accumulation,
one autograd node per call.

The 16-bit packed copies of a weight are cached exactly as ``linear.LinearUnit`` caches its own: under a version key
(data pointer, ``_version``, device, dtype); ``invalidate_packed`` reaches them; inside a graph capture they are
re-packed in place when ``functional.REPACK_IN_CAPTURE`` is set, so that a replay after an optimizer update computes with
the updated weights.
"""
import weakref

import torch

from . import deconv_ops, linear_ops, ops
from . import functional as _F
from ._args import tensor

__all__ = ["conv_transpose2x2", "ConvTranspose2x2Function", "DeconvUnit"]

_16 = (torch.bfloat16, torch.float16)


class DeconvUnit(object):
    """Packed 16-bit operands of one (Cin, Cout, 2, 2) weight for one compute dtype."""

    def __init__(self, weight, dtype):
        self.weight = weight
        self.dtype = dtype
        self.key = None
        self.w_fwd = self.w_dgrad = None
        self._layout = None

    def _version_key(self):
        w = self.weight
        return (self.dtype, w.data_ptr(), w._version, w.device)

    def refresh(self):
        w = self.weight
        if not w.is_cuda:
            raise RuntimeError('torch_detection_amd modules run on the MI355X HIP path only: move the module to '
                               'a CUDA/HIP device (no CPU fallback)')
        key = self._version_key()
        capturing = _F.REPACK_IN_CAPTURE and torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        layout = (w.device, self.dtype, tuple(w.shape))
        reuse = self.w_fwd is not None and layout == self._layout
        self._layout = layout
        with torch.no_grad():
            self.w_fwd, self.w_dgrad = deconv_ops.pack_deconv_weight(
                w.detach(), True, self.dtype, out=(self.w_fwd, self.w_dgrad) if reuse else None)
        self.key = key
        return self


_units = {}   # id(weight) -> (weak reference to the weight, {dtype: DeconvUnit})


def _unit_for(weight, dtype):
    k = id(weight)
    ent = _units.get(k)
    if ent is None or ent[0]() is not weight:
        ent = (weakref.ref(weight, lambda _, k=k: _units.pop(k, None)), {})
        _units[k] = ent
    u = ent[1].get(dtype)
    if u is None:
        u = ent[1][dtype] = DeconvUnit(weight, dtype)
    return u


def forget(weight):
    """``invalidate_packed``'s hook: drop the version key of every packed copy of ``weight``."""
    ent = _units.get(id(weight))
    if ent is not None and ent[0]() is weight:
        for u in ent[1].values():
            u.key = None


def check_params(weight, bias, Cin):
    """float32 (Cin, Cout, 2, 2) weight and (Cout,) bias or None; returns Cout.  Needs no device."""
    Cout = tensor(weight, "weight", torch.float32, (Cin, "Cout", 2, 2), contiguous=False)[1]
    if bias is not None:
        tensor(bias, "bias", torch.float32, (Cout,))
    return Cout


def _dtype_of(x):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("x must be a 4-D (R, Cin, H, W) tensor, got %s" % (
            tuple(x.shape) if torch.is_tensor(x) else type(x).__name__,))
    return x.dtype if x.dtype in _16 else torch.bfloat16


class ConvTranspose2x2Function(torch.autograd.Function):
    """``apply(x, weight, bias, relu)``.  Saves the 16-bit channels_last input (and the output when ``relu``); backward
    returns ``dx`` in ``x``'s dtype, channels_last, and float32 ``dw`` / ``dbias``."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        dtype = _dtype_of(x)
        xh = ops.to_nhwc_bf16(x, dtype).permute(0, 3, 1, 2)     # zero-copy for a channels_last 16-bit input
        check_params(weight, bias, xh.shape[1])
        unit = _unit_for(weight, dtype).refresh()
        y = deconv_ops.deconv2x2_fwd(xh, unit.w_fwd, bias.detach() if bias is not None else None, relu)
        ctx.save_for_backward(xh, y if relu else None)
        ctx.meta = (unit, relu, bias is not None, x.dtype, x.dim() == 4 and x.is_contiguous() and not xh.is_contiguous())
        return y

    @staticmethod
    def backward(ctx, g):
        xh, y = ctx.saved_tensors
        unit, relu, has_bias, in_dtype, nchw = ctx.meta
        g = ops.to_nhwc_bf16(g, xh.dtype)                        # (R, 2H, 2W, Cout) memory
        R, H2, W2, Cout = g.shape
        if relu:      # y is a contiguous (R * 2H * 2W, Cout) matrix in memory
            g = linear_ops.linear_relu_bwd(g.view(-1, Cout), y.permute(0, 2, 3, 1).reshape(-1, Cout)).view(R, H2, W2, Cout)
        g = g.permute(0, 3, 1, 2)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = deconv_ops.deconv2x2_dgrad(g, unit.w_dgrad)
            if dx.dtype != in_dtype:
                dx = dx.to(in_dtype)
            if nchw:                                             # the input's own layout
                dx = dx.contiguous()
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            dw, db = deconv_ops.deconv2x2_wgrad(xh, g, want_dbias=has_bias)
        return dx, dw, db, None


def conv_transpose2x2(x, weight, bias=None, relu=False):
    """``relu?(F.conv_transpose2d(x, weight, bias, stride=2))``: ``x`` a (R, Cin, H, W) CUDA tensor (a 16-bit
    channels_last one — what ``roi_align`` and the conv modules return — is read in place; anything else is converted
    as ``ConvModule`` converts its input), ``weight`` (Cin, Cout, 2, 2) and ``bias`` (Cout,) float32.  Returns a
    channels_last (R, Cout, 2H, 2W) tensor in the compute dtype.  Differentiable in all three."""
    _dtype_of(x)
    check_params(weight, bias, x.shape[1])
    return ConvTranspose2x2Function.apply(x, weight, bias, bool(relu))
