"""Deformable convolution, DCN v1 / v2, on the HIP path (csrc/deform.hip).

``deform_conv2d`` is one autograd node: the bilinear gather ``deform_ops.deform_sample`` writes ``cols`` (N, Ho, Wo, 9 C),
the existing 1x1 conv GEMM multiplies it by the packed weight (bias and ReLU in its epilogue).  The backward recomputes
``cols`` instead of keeping 9x the activation alive: ``dcol`` by the 1x1 input-gradient GEMM, ``dW`` / ``db`` by the 1x1
weight-gradient launch over ``cols``, the offset / mask gradients by ``deform_coord_grad`` and ``dx`` by
``deform_input_grad`` — no atomics anywhere, the same bits on every run, eager or replayed.

The 16-bit packed copies of a weight are cached as ``deconv.DeconvUnit`` caches its own: under a version key (data pointer,
``_version``, device, dtype); ``invalidate_packed`` reaches them; inside a graph capture they are re-packed in place when
``functional.REPACK_IN_CAPTURE`` is set, so that a replay after an optimizer update computes with the updated weights.

The modules take mmdetection v1's constructor and state-dict keys (``weight``, ``bias``, ``conv_offset.*`` /
``conv_offset_mask.*``).  The offset conv of the Pack modules runs on routes the library already has — the one-level
pyramid conv where its geometry allows, else the conv GEMM with the weight zero padded to 64 outputs — and its output
buffer is read in place by the sampling kernels through the pixel pitch; the node's offset / mask gradient is written into
one buffer of that layout, which is the offset conv's cotangent.
"""
import math
import weakref

import torch
from torch import nn

from . import deform_ops, ops, pyramid_ops
from . import functional as _F
from ._args import on_device, tensor

__all__ = ["deform_conv2d", "DeformConvFunction", "DeformUnit", "DeformConv", "ModulatedDeformConv", "DeformConvPack",
           "ModulatedDeformConvPack"]

_16 = (torch.bfloat16, torch.float16)
_NO_CPU = ('torch_detection_amd modules run on the MI355X HIP path only: move the module to a CUDA/HIP device (no CPU '
           'fallback)')


class DeformUnit(object):
    """Packed 16-bit operands of one (Cout, C, 3, 3) weight for one compute dtype: ``w_fwd`` (Cout, 1, 1, 9 C) and
    ``w_dgrad`` (9 C, 1, 1, Cout), the 1x1 GEMM operands over ``cols``."""

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
            raise RuntimeError(_NO_CPU)
        key = self._version_key()
        capturing = _F.REPACK_IN_CAPTURE and torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        layout = (w.device, self.dtype, tuple(w.shape))
        reuse = self.w_fwd is not None and layout == self._layout
        self._layout = layout
        with torch.no_grad():
            self.w_fwd, self.w_dgrad = deform_ops.pack_deform_weight(
                w.detach(), True, self.dtype, out=(self.w_fwd, self.w_dgrad) if reuse else None)
        self.key = key
        return self


_units = {}   # id(weight) -> (weak reference to the weight, {dtype: DeformUnit})


def _unit_for(weight, dtype):
    k = id(weight)
    ent = _units.get(k)
    if ent is None or ent[0]() is not weight:
        ent = (weakref.ref(weight, lambda _, k=k: _units.pop(k, None)), {})
        _units[k] = ent
    u = ent[1].get(dtype)
    if u is None:
        u = ent[1][dtype] = DeformUnit(weight, dtype)
    return u


def forget(weight):
    """``invalidate_packed``'s hook: drop the version key of every packed copy of ``weight``."""
    ent = _units.get(id(weight))
    if ent is not None and ent[0]() is weight:
        for u in ent[1].values():
            u.key = None


def check_args(x, offset, weight, bias=None, stride=1, padding=1, dilation=1, deformable_groups=1, mask=None, packed=0):
    """Every refusal of ``deform_conv2d`` as a ValueError, before any launch: shapes, dtypes, layouts and limits first (no
    device needed), the device last.  ``packed``: ``offset`` is the offset conv's whole output buffer (see the module
    docstring).  Returns the checked ``deform_ops.Geometry``."""
    N, C, H, W = deform_ops._x(x)
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4:
        tensor(weight, "weight", torch.float32, ("Cout", C, 3, 3), contiguous=False)
    g = deform_ops.geometry(N, C, H, W, tuple(weight.shape[2:]), stride, padding, dilation, deformable_groups)
    Cout = tensor(weight, "weight", torch.float32, ("Cout", C, 3, 3), contiguous=False)[0]
    if Cout % 64 or not Cout:
        raise ValueError("weight: Cout must be a multiple of 64, got %d" % Cout)
    if bias is not None:
        tensor(bias, "bias", torch.float32, (Cout,))
    if packed:
        used = (18 if packed == 1 else 27) * g.dg
        P = deform_ops._nhwc(offset, "offset buffer", x.dtype, (N, "P", g.Ho, g.Wo))[1]
        if P < used or mask is not None:
            raise ValueError("a packed offset buffer holds %d channels and comes without a separate mask" % used)
    else:
        deform_ops._operands(g, x.dtype, offset, mask)
    on_device([("x", x), ("offset", offset), ("mask", mask), ("weight", weight), ("bias", bias)])
    return g


class DeformConvFunction(torch.autograd.Function):
    """``apply(x, offset, mask, weight, bias, stride, pad, deformable_groups, relu, mask_is_logit, packed)``.  Saves ``x``,
    the offsets and the mask (and the output when ``relu``), not ``cols``.  ``packed`` 1 / 2: ``offset`` is a channels_last
    (N, P, Ho, Wo) buffer whose first 18 dg channels are the offsets and (2) next 9 dg the mask logits; its gradient is
    one buffer of that shape, the channels past those zero."""

    @staticmethod
    def forward(ctx, x, offset, mask, weight, bias, stride, pad, dg, relu, mask_is_logit, packed):
        g = check_args(x, offset, weight, bias, stride, pad, pad, dg, mask, packed)
        unit = _unit_for(weight, x.dtype).refresh()
        off, msk = _split(offset, mask, g.dg, packed)
        cols = deform_ops.deform_sample(x, off, msk, stride, pad, pad, dg, mask_is_logit)
        y = ops.conv2d_fwd(cols, unit.w_fwd, 1, 1, 0, None, bias.detach() if bias is not None else None, relu=relu)
        ctx.save_for_backward(x, offset, mask, y if relu else None)
        ctx.meta = (unit, stride, pad, dg, relu, mask_is_logit, packed, bias is not None)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        x, offset, mask, y = ctx.saved_tensors
        unit, stride, pad, dg, relu, logit, packed, has_bias = ctx.meta
        gy = ops.to_nhwc_bf16(gy, x.dtype)                                   # (N, Ho, Wo, Cout) memory
        if relu:
            gy = ops.act_mask(gy, y)
        N, Ho, Wo, _ = gy.shape
        off, msk = _split(offset, mask, dg, packed)
        need = ctx.needs_input_grad
        dx = doff = dmsk = dw = db = None
        if need[3] or (has_bias and need[4]):
            cols = deform_ops.deform_sample(x, off, msk, stride, pad, pad, dg, logit)
            dw, _, db = ops.conv2d_wgrad(cols, gy, unit.w_fwd, 1, 1, 0, want_dbeta=has_bias)
            dw = dw.view(dw.shape[0], 3, 3, x.shape[1]).permute(0, 3, 1, 2)  # [O][3][3][I] seen as OIHW
            del cols
        if need[0] or need[1] or (msk is not None and (need[2] or packed)):
            dcol = ops.conv2d_dgrad(gy, unit.w_dgrad, (Ho, Wo), 1, 1, 0)
            if need[1] or (msk is not None and (need[2] or packed)):
                if packed:
                    P, used = offset.shape[1], (18 if packed == 1 else 27) * dg
                    buf = (torch.empty if P == used else torch.zeros)((N, Ho, Wo, P), dtype=offset.dtype,
                                                                      device=offset.device).permute(0, 3, 1, 2)
                    deform_ops.deform_coord_grad(dcol, x, off, msk, stride, pad, pad, dg, logit,
                                                 out=_split(buf, None, dg, packed))
                    doff = buf
                else:
                    doff, dmsk = deform_ops.deform_coord_grad(dcol, x, off, msk, stride, pad, pad, dg, logit)
            if need[0]:
                dx = deform_ops.deform_input_grad(dcol, off, msk, tuple(x.shape), stride, pad, pad, dg, logit)
        return dx, doff, dmsk, dw, db, None, None, None, None, None, None


def _split(offset, mask, dg, packed):
    if not packed:
        return offset, mask
    return offset[:, :18 * dg], (offset[:, 18 * dg:27 * dg] if packed == 2 else None)


def deform_conv2d(x, offset, weight, bias=None, stride=1, padding=1, dilation=1, deformable_groups=1, mask=None,
                  relu=False, mask_is_logit=False):
    """``relu?(sum_{k, c} W[:, c, k] * sample(x, c, k) (+ bias))`` — DCN v1, or v2 with ``mask`` — as DESIGN.md §4p
    specifies it.  ``x``: (N, C, H, W) bf16 / fp16 CUDA tensor in channels_last memory; ``weight`` (Cout, C, 3, 3) and
    ``bias`` float32; ``offset`` (N, 18 dg, Ho, Wo) and ``mask`` (N, 9 dg, Ho, Wo) float32 or ``x``'s dtype, NHWC memory
    with any pixel pitch; ``mask_is_logit``: the kernels apply the sigmoid, and the mask gradient is the logit's.
    3x3 only, stride 1 or 2, padding == dilation in 1..32.  Returns (N, Cout, Ho, Wo) in ``x``'s dtype, channels_last.
    Differentiable in ``x``, ``offset``, ``mask``, ``weight`` and ``bias``."""
    check_args(x, offset, weight, bias, stride, padding, dilation, deformable_groups, mask)
    return DeformConvFunction.apply(x, offset, mask, weight, bias, int(stride), int(padding), int(deformable_groups),
                                    bool(relu), bool(mask_is_logit), 0)


# ---- the offset conv of the Pack modules -----------------------------------------------------------------------------
class OffsetConvUnit(object):
    """Packed operands of a Pack module's 3x3 offset conv.  Route 'pyramid': the one-level pyramid conv (stride 1,
    dilation 1, 64..512 input channels), exactly Cout channels per pixel.  Route 'padded': the conv GEMM over the weight
    and bias zero padded to Cp = 64-multiple outputs.  Cached like ``DeformUnit``."""

    def __init__(self, conv, dtype):
        self.conv, self.dtype = conv, dtype
        self.Cout, self.Cin = conv.weight.shape[:2]
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        self.route = 'pyramid' if self.stride == 1 and self.pad == 1 and 64 <= self.Cin <= pyramid_ops.MAX_CIN else 'padded'
        self.Cp = self.Cout if self.route == 'pyramid' else -(-self.Cout // 64) * 64
        self.key = None
        self.w_fwd = self.w_dgrad = self.w_pad = self.b_pad = None
        self._layout = None

    def refresh(self):
        w, b = self.conv.weight, self.conv.bias
        if not w.is_cuda:
            raise RuntimeError(_NO_CPU)
        key = (self.dtype, w.data_ptr(), w._version, w.device, b.data_ptr(), b._version)
        capturing = _F.REPACK_IN_CAPTURE and torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        layout = (w.device, self.dtype, tuple(w.shape))
        reuse = self.w_fwd is not None and layout == self._layout
        self._layout = layout
        out = (self.w_fwd, self.w_dgrad) if reuse else None
        with torch.no_grad():
            if self.route == 'pyramid':
                self.w_fwd, self.w_dgrad = pyramid_ops.pack_pyramid_weight(w.detach(), True, self.dtype, out=out)
            else:
                if not reuse:
                    self.w_pad = torch.zeros((self.Cp, self.Cin, 3, 3), dtype=torch.float32, device=w.device)
                    self.b_pad = torch.zeros((self.Cp,), dtype=torch.float32, device=w.device)
                self.w_pad[:self.Cout].copy_(w)
                self.b_pad[:self.Cout].copy_(b)
                self.w_fwd, self.w_dgrad = ops.pack_conv_weight(self.w_pad, None, True, self.dtype, out=out)
        self.key = key
        return self


class OffsetConvFunction(torch.autograd.Function):
    """``apply(x, weight, bias, unit)`` -> the offset conv's output buffer, logical (N, Cp, Ho, Wo) in channels_last
    memory (Cp: see ``OffsetConvUnit``; the channels past the conv's own are zero)."""

    @staticmethod
    def forward(ctx, x, weight, bias, unit):
        if unit.route == 'pyramid':
            y = pyramid_ops.pyramid_conv_fwd([x], unit.w_fwd, bias.detach(), unit.Cout)[0]
        else:
            y = ops.conv2d_fwd(x.permute(0, 2, 3, 1), unit.w_fwd, 3, unit.stride, unit.pad, None,
                               unit.b_pad).permute(0, 3, 1, 2)
        ctx.save_for_backward(x)
        ctx.unit = unit
        return y

    @staticmethod
    def backward(ctx, g):
        (x,), unit = ctx.saved_tensors, ctx.unit
        need = ctx.needs_input_grad
        dx = dw = db = None
        if unit.route == 'pyramid':
            if need[0]:
                dx = pyramid_ops.pyramid_conv_dgrad([g], unit.w_dgrad)[0]
            if need[1] or need[2]:
                dw, db = pyramid_ops.pyramid_conv_wgrad([x], [g], unit.conv.weight.permute(0, 2, 3, 1).is_contiguous())
        else:
            g = ops.to_nhwc_bf16(g, x.dtype)
            xn = x.permute(0, 2, 3, 1)
            if need[0]:
                dx = ops.conv2d_dgrad(g, unit.w_dgrad, tuple(xn.shape[1:3]), 3, unit.stride, unit.pad).permute(0, 3, 1, 2)
            if need[1] or need[2]:
                dw, _, db = ops.conv2d_wgrad(xn, g, unit.w_fwd, 3, unit.stride, unit.pad)
                dw, db = dw[:unit.Cout].permute(0, 3, 1, 2), db[:unit.Cout]
        return dx, dw, db, None


# ---- modules -----------------------------------------------------------------------------------------------------------
def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class DeformConv(nn.Module):
    """mmdetection v1's ``DeformConv`` (DCN v1): ``forward(x, offset)``.  Constructor and state-dict keys are
    mmdetection's; ``relu=True`` fuses a ReLU into the GEMM's epilogue.  The sampling rule is the modulated kernel's
    (DESIGN.md §4p).  What the HIP path does not cover — kernels other than 3x3, ``groups > 1``, strides above 2,
    ``padding != dilation``, channel counts that are no multiples of 64 — constructs and raises ``NotImplementedError``
    in ``forward``."""
    modulated = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, bias=False, relu=False):
        super().__init__()
        if in_channels % groups or out_channels % groups:
            raise ValueError("in_channels %d and out_channels %d must be divisible by groups %d" % (
                in_channels, out_channels, groups))
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.groups, self.deformable_groups = int(groups), int(deformable_groups)
        self.with_bias, self.relu = bool(bias), bool(relu)
        self.weight = nn.Parameter(torch.empty(self.out_channels, self.in_channels // self.groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        n = self.in_channels * self.kernel_size[0] * self.kernel_size[1]
        stdv = 1.0 / math.sqrt(n)
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.zero_()

    def _geometry(self):
        """(stride, padding, dilation) of the HIP path, or NotImplementedError"""
        k, s, p, d = self.kernel_size, self.stride, self.padding, self.dilation
        C, dg = self.in_channels, self.deformable_groups
        if k != (3, 3) or self.groups != 1 or s[0] != s[1] or s[0] not in (1, 2) or p[0] != p[1] or d[0] != d[1] or \
                p[0] != d[0] or not 1 <= d[0] <= 32 or C % 64 or self.out_channels % 64 or dg < 1 or C % dg or \
                (C // dg) % 8:
            raise NotImplementedError(
                "%s(%d, %d, kernel_size=%s, stride=%s, padding=%s, dilation=%s, groups=%d, deformable_groups=%d) is not "
                "on the HIP path: 3x3, groups 1, stride 1 or 2, padding == dilation in 1..32, channels multiples of 64, "
                "deformable_groups dividing in_channels into multiples of 8" % (
                    type(self).__name__, C, self.out_channels, k, s, p, d, self.groups, dg))
        return s[0], p[0], d[0]

    def forward(self, x, offset, mask=None):
        s, p, d = self._geometry()
        if (mask is not None) != self.modulated:
            raise ValueError("%s takes %s" % (type(self).__name__, "x, offset and mask" if self.modulated else
                                              "x and offset"))
        return deform_conv2d(x, offset, self.weight, self.bias, s, p, d, self.deformable_groups, mask, self.relu)

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, stride=%s, padding=%s, dilation=%s, groups=%d, deformable_groups=%d, bias=%s" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation, self.groups,
            self.deformable_groups, self.with_bias)


class ModulatedDeformConv(DeformConv):
    """mmdetection v1's ``ModulatedDeformConv`` (DCN v2): ``forward(x, offset, mask)``, the mask already a weight (in v1:
    ``torch.sigmoid`` of the mask conv's output)."""
    modulated = True


class _Pack(object):
    """What the two Pack modules share: the zero-initialised 3x3 offset conv with bias — the main conv's stride, padding =
    dilation = the main conv's (mmdetection v1 builds it without the dilation) — and the forward through the two nodes."""

    def _make_offset_conv(self, name, per_tap):
        conv = nn.Conv2d(self.in_channels, self.deformable_groups * per_tap * self.kernel_size[0] * self.kernel_size[1],
                         kernel_size=self.kernel_size, stride=self.stride, padding=self.padding, dilation=self.dilation,
                         bias=True)
        with torch.no_grad():
            conv.weight.zero_()
            conv.bias.zero_()
        setattr(self, name, conv)

    def _forward(self, x, conv, packed):
        s, p, _ = self._geometry()
        deform_ops._x(x)
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
        cache = self.__dict__.setdefault('_hip_units', {})
        u = cache.get(('offset', x.dtype))
        if u is None or u.conv is not conv:
            u = cache[('offset', x.dtype)] = OffsetConvUnit(conv, x.dtype)
        buf = OffsetConvFunction.apply(x, conv.weight, conv.bias, u.refresh())
        return DeformConvFunction.apply(x, buf, None, self.weight, self.bias, s, p, self.deformable_groups, self.relu,
                                        packed == 2, packed)


class DeformConvPack(_Pack, DeformConv):
    """mmdetection v1's ``DeformConvPack``: ``forward(x)``, the offsets from ``conv_offset`` (18 dg outputs)."""

    def __init__(self, *args, **kwargs):
        DeformConv.__init__(self, *args, **kwargs)
        self._make_offset_conv('conv_offset', 2)

    def forward(self, x):
        return self._forward(x, self.conv_offset, 1)


class ModulatedDeformConvPack(_Pack, ModulatedDeformConv):
    """mmdetection v1's ``ModulatedDeformConvPack``: ``forward(x)``; ``conv_offset_mask`` has 27 dg outputs, the first
    18 dg the offsets, the last 9 dg the mask logits, whose sigmoid the sampling kernels apply."""

    def __init__(self, *args, **kwargs):
        ModulatedDeformConv.__init__(self, *args, **kwargs)
        self._make_offset_conv('conv_offset_mask', 3)

    def forward(self, x):
        return self._forward(x, self.conv_offset_mask, 2)
