"""Fully connected layer on the HIP path (csrc/linear.hip): ``linear`` is ``F.linear`` (+ ReLU) with fp32
parameters, 16-bit operands and fp32 accumulation, one autograd node per call.

The 16-bit packed copies of a weight are cached under a version key, exactly as the conv units' are
(``functional.ConvUnit``): data pointer, ``_version``, device and dtype; ``invalidate_packed`` reaches them; inside a
graph capture they are re-packed in place when ``functional.REPACK_IN_CAPTURE`` is set, so that a replay after an
optimizer update computes with the updated weights.
"""
import weakref

import torch

from . import functional as _F
from . import linear_ops
from ._args import tensor

__all__ = ["linear", "LinearFunction", "LinearUnit"]

_16 = (torch.bfloat16, torch.float16)


class LinearUnit(object):
    """Packed 16-bit operands of one weight — or of several weights stacked along the output dimension (the box head's
    two predictors share one input-gradient GEMM) — for one compute dtype and one column permutation ``C``."""

    def __init__(self, sources, dtype, C=None):
        self.sources = tuple(sources)
        self.dtype = dtype
        self.C = C
        self.key = None
        self.w_fwd = self.w_dgrad = None
        self._layout = None

    def _version_key(self):
        key = [self.dtype, self.C]
        for w in self.sources:
            key += [w.data_ptr(), w._version, w.device]
        return tuple(key)

    def refresh(self):
        w0 = self.sources[0]
        if not w0.is_cuda:
            raise RuntimeError('torch_detection_amd modules run on the MI355X HIP path only: move the module to '
                               'a CUDA/HIP device (no CPU fallback)')
        key = self._version_key()
        capturing = _F.REPACK_IN_CAPTURE and torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        layout = (w0.device, self.dtype, tuple(tuple(w.shape) for w in self.sources))
        reuse = self.w_fwd is not None and layout == self._layout
        self._layout = layout
        with torch.no_grad():
            w = w0.detach() if len(self.sources) == 1 else torch.cat([s.detach() for s in self.sources], 0)
            self.w_fwd, self.w_dgrad = linear_ops.pack_linear_weight(
                w, self.C, True, self.dtype, out=(self.w_fwd, self.w_dgrad) if reuse else None)
        self.key = key
        return self


_units = {}   # id(weight) -> (weak reference to the weight, {(dtype, C): LinearUnit})


def _unit_for(weight, dtype, C):
    k = id(weight)
    ent = _units.get(k)
    if ent is None or ent[0]() is not weight:
        ent = (weakref.ref(weight, lambda _, k=k: _units.pop(k, None)), {})
        _units[k] = ent
    u = ent[1].get((dtype, C))
    if u is None:
        u = ent[1][(dtype, C)] = LinearUnit((weight,), dtype, C)
    return u


def forget(weight):
    """``invalidate_packed``'s hook: drop the version key of every packed copy of ``weight``."""
    ent = _units.get(id(weight))
    if ent is not None and ent[0]() is weight:
        for u in ent[1].values():
            u.key = None


def flatten_input(x):
    """-> (x as an (M, K) view in memory order, C or None, restore): the reference flattening ``x.view(R, -1)`` of a
    logical (R, C, S, S) tensor.  A channels_last buffer is taken in place with the packed column permutation ``C``; a
    contiguous one as it is.  ``restore(dx2d)`` gives a gradient the layout of ``x``.  Needs no device."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _16 or x.dim() not in (2, 4):
        raise ValueError("x must be a 2-D (M, K) or 4-D (R, C, S, S) bfloat16 / float16 tensor, got %s" % (
            "%s %s" % (str(x.dtype).replace("torch.", ""), tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__))
    if x.dim() == 2:
        tensor(x, "x", _16, ("M", "K"))
        return x, None, lambda d: d
    R, C, S1, S2 = x.shape
    K = C * S1 * S2
    if x.is_contiguous():
        return x.view(R, K), None, lambda d: d.view(R, C, S1, S2)
    xl = x.permute(0, 2, 3, 1)
    if xl.is_contiguous():
        return xl.reshape(R, K), C, lambda d: d.view(R, S1, S2, C).permute(0, 3, 1, 2)
    raise ValueError("x must be a contiguous or channels_last (R, C, S, S) tensor, got strides %s" % (tuple(x.stride()),))


def check_params(weight, bias, K):
    O = tensor(weight, "weight", torch.float32, ("O", K), contiguous=False)[0]
    if bias is not None:
        tensor(bias, "bias", torch.float32, (O,))
    return O


class LinearFunction(torch.autograd.Function):
    """``apply(x, weight, bias, relu, out_f32)``.  Saves the 16-bit input (and the output when ``relu``); backward
    returns ``dx`` in ``x``'s dtype and layout and float32 ``dw`` / ``dbias``."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, out_f32):
        x2, C, restore = flatten_input(x)
        O = check_params(weight, bias, x2.shape[1])
        unit = _unit_for(weight, x.dtype, C).refresh()
        y = linear_ops.linear_fwd(x2, unit.w_fwd, O, bias.detach() if bias is not None else None, relu, out_f32)
        ctx.save_for_backward(x2, y if relu else None)
        ctx.meta = (unit, C, restore, relu, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        x2, y = ctx.saved_tensors
        unit, C, restore, relu, has_bias = ctx.meta
        g = g.to(x2.dtype).contiguous()
        if relu:
            g = linear_ops.linear_relu_bwd(g, y)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = restore(linear_ops.linear_dgrad(g, unit.w_dgrad))
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            dw, db = linear_ops.linear_wgrad(x2, g, C, want_dbias=has_bias)
        return dx, dw, db, None, None


def linear(x, weight, bias=None, relu=False, out_f32=False):
    """``relu?(x.view(R, -1) @ weight.T + bias)``: ``x`` a contiguous (M, K) or a (R, C, S, S) 16-bit CUDA tensor (a
    channels_last one — what ``roi_align`` returns — is read in place), ``weight`` (O, K) and ``bias`` (O,) float32.
    Returns (M, O) in ``x``'s dtype, float32 with ``out_f32``.  Differentiable in all three."""
    x2, _, _ = flatten_input(x)
    check_params(weight, bias, x2.shape[1])
    return LinearFunction.apply(x, weight, bias, bool(relu), bool(out_f32))
