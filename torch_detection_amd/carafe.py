"""CARAFE content-aware upsampling (Wang et al., ICCV 2019) on the HIP path (csrc/carafe.hip).

``carafe`` is mmdetection's op: the reassembly of a feature map by given, already normalised masks, differentiable in
both operands.  ``CARAFEPack`` is mmdetection's module — a 1x1 ``channel_compressor``, a 3x3 ``content_encoder``, the
pixel-shuffle / softmax ``kernel_normalizer`` and the reassembly — as ONE autograd node: the compressor runs on the conv
GEMM, the encoder on the one-level pyramid conv (its ragged ``k^2 g s^2`` output channels written exactly), and the
normaliser is part of the reassembly launch, which reads the encoder's output buffer where it lies.  The backward recomputes
the softmax from those logits (nothing but ``x``, the compressed map and the logits is kept): feature gradient, logit
gradient, then the two convs' adjoints; the compressor's input gradient takes the reassembly's feature gradient as its
epilogue addend, so ``dx`` is rounded once.  No atomics anywhere: the same bits on every run, eager or replayed.

``forward(x, out_size=None, addend=None)`` exposes the kernels' crop / add, which is what ``FPN_CARAFE``'s
``tensor_add`` needs: ``addend + upsampled[:, :, :Ho, :Wo]`` in one launch.

The 16-bit packed copies of the two weights are cached on the module as the heads cache theirs: under a version key
(data pointers, ``_version``s, device, dtype); ``invalidate_packed`` drops the key; inside a graph capture they are re-packed
in place when ``functional.REPACK_IN_CAPTURE`` is set.
"""
import torch
from torch import nn

from . import carafe_ops, ops, pyramid_ops
from . import functional as _F
from ._args import integer
from .inits import normal_init, xavier_init

__all__ = ["carafe", "CarafeFunction", "CARAFEPack", "CARAFEPackFunction"]

_16 = (torch.bfloat16, torch.float16)
_NO_CPU = ('torch_detection_amd modules run on the MI355X HIP path only: move the module to a CUDA/HIP device (no CPU '
           'fallback)')


def _nchw(t):
    return t.permute(0, 3, 1, 2)


class CarafeFunction(torch.autograd.Function):
    """``apply(features, masks, kernel_size, group_size, scale_factor)``; saves both operands."""

    @staticmethod
    def forward(ctx, features, masks, k, g, s):
        out = carafe_ops.carafe_forward(features, k, g, s, masks=masks)
        ctx.save_for_backward(features, masks)
        ctx.meta = (k, g, s)
        return out

    @staticmethod
    def backward(ctx, gout):
        features, masks = ctx.saved_tensors
        k, g, s = ctx.meta
        gout = _nchw(ops.to_nhwc_bf16(gout, features.dtype))
        dx = dm = None
        if ctx.needs_input_grad[0]:
            dx = carafe_ops.carafe_feature_grad(gout, tuple(features.shape), k, g, s, masks=masks)
        if ctx.needs_input_grad[1]:
            dm = carafe_ops.carafe_mask_grad(gout, features, k, g, s, masks=masks)
        return dx, dm, None, None, None


def carafe(features, masks, kernel_size, group_size, scale_factor):
    """mmdetection's ``carafe`` op.  ``features``: (N, C, H, W) bf16 / fp16 CUDA tensor (channels_last memory is read in
    place); ``masks``: (N, group_size * kernel_size^2, sH, sW), float32 or ``features``' dtype, normalised by the caller.
    Returns (N, C, sH, sW) in ``features``' dtype, channels_last.  Differentiable in both operands."""
    if not isinstance(features, torch.Tensor) or features.dim() != 4 or features.dtype not in _16:
        carafe_ops._x(features)
    if not isinstance(masks, torch.Tensor) or masks.dim() != 4:
        raise ValueError("masks must be a 4-D tensor")
    N, C, H, W = features.shape
    q = carafe_ops.geometry(N, C, H, W, kernel_size, group_size, scale_factor)
    if not features.is_cuda or not masks.is_cuda:
        raise ValueError("features and masks must be CUDA tensors")
    features = _nchw(ops.to_nhwc_bf16(features, features.dtype))
    if masks.dtype not in (torch.float32, features.dtype):
        masks = masks.to(features.dtype)
    if not masks.permute(0, 2, 3, 1).is_contiguous():
        try:
            carafe_ops._weights(q, features.dtype, masks, None)
        except ValueError:
            masks = masks.contiguous(memory_format=torch.channels_last)
    return CarafeFunction.apply(features, masks, q.k, q.g, q.s)


class CarafeUnit(object):
    """Packed 16-bit operands of one ``CARAFEPack`` for one compute dtype: the compressor's conv-GEMM pair and the
    encoder's pyramid-conv pair."""

    def __init__(self, module, dtype):
        self.module, self.dtype = module, dtype
        self.key = None
        self.wc_fwd = self.wc_dgrad = self.we_fwd = self.we_dgrad = None
        self._layout = None

    def refresh(self):
        m = self.module
        ps = (m.channel_compressor.weight, m.channel_compressor.bias, m.content_encoder.weight, m.content_encoder.bias)
        if not ps[0].is_cuda:
            raise RuntimeError(_NO_CPU)
        key = (self.dtype,) + tuple((p.data_ptr(), p._version, p.device) for p in ps)
        capturing = _F.REPACK_IN_CAPTURE and torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        layout = (ps[0].device, self.dtype, tuple(ps[0].shape), tuple(ps[2].shape))
        reuse = self.wc_fwd is not None and layout == self._layout
        self._layout = layout
        with torch.no_grad():
            self.wc_fwd, self.wc_dgrad = ops.pack_conv_weight(
                ps[0].detach(), None, True, self.dtype, out=(self.wc_fwd, self.wc_dgrad) if reuse else None)
            self.we_fwd, self.we_dgrad = pyramid_ops.pack_pyramid_weight(
                ps[2].detach(), True, self.dtype, out=(self.we_fwd, self.we_dgrad) if reuse else None)
        self.key = key
        return self


class CARAFEPackFunction(torch.autograd.Function):
    """``apply(x, addend, wc, bc, we, be, unit, out_size)`` -> (N, C, Ho, Wo).  Saves ``x``, the compressed map and the
    encoder's logits."""

    @staticmethod
    def forward(ctx, x, addend, wc, bc, we, be, unit, out_size):
        m = unit.module
        xh = x.permute(0, 2, 3, 1)
        comp = ops.conv2d_fwd(xh, unit.wc_fwd, 1, 1, 0, None, bc.detach())                     # (N, H, W, Cm)
        logits = pyramid_ops.pyramid_conv_fwd([_nchw(comp)], unit.we_fwd, be.detach(), we.shape[0])[0]
        out = carafe_ops.carafe_forward(x, m.up_kernel, m.up_group, m.scale_factor, logits=logits, out_size=out_size,
                                        addend=addend)
        ctx.save_for_backward(x, comp, logits)
        ctx.unit = unit
        ctx.we_cl = we.permute(0, 2, 3, 1).is_contiguous()
        return out

    @staticmethod
    def backward(ctx, gout):
        x, comp, logits = ctx.saved_tensors
        unit, m = ctx.unit, ctx.unit.module
        k, g, s = m.up_kernel, m.up_group, m.scale_factor
        need = ctx.needs_input_grad
        gout = _nchw(ops.to_nhwc_bf16(gout, x.dtype))
        dx = dwc = dbc = dwe = dbe = None
        if any(need[i] for i in (0, 2, 3, 4, 5)):
            dlogits = carafe_ops.carafe_mask_grad(gout, x, k, g, s, logits=logits)
            if need[4] or need[5]:
                dwe, dbe = pyramid_ops.pyramid_conv_wgrad([_nchw(comp)], [dlogits], ctx.we_cl)
            if need[0] or need[2] or need[3]:
                dcomp = pyramid_ops.pyramid_conv_dgrad([dlogits], unit.we_dgrad)[0].permute(0, 2, 3, 1)
                if need[2] or need[3]:
                    dwc, _, dbc = ops.conv2d_wgrad(x.permute(0, 2, 3, 1), dcomp, unit.wc_fwd, 1, 1, 0)
                    dwc = dwc.view(dwc.shape[0], dwc.shape[3], 1, 1)
                if need[0]:
                    dfeat = carafe_ops.carafe_feature_grad(gout, tuple(x.shape), k, g, s, logits=logits)
                    dx = _nchw(ops.conv2d_dgrad(dcomp, unit.wc_dgrad, tuple(x.shape[2:]), 1, 1, 0,
                                                dfeat.permute(0, 2, 3, 1), ops.ADD_SAME))
        return dx, (gout if need[1] else None), dwc, dbc, dwe, dbe, None, None


class CARAFEPack(nn.Module):
    """mmdetection's ``CARAFEPack``: ``forward(x)`` upsamples (N, channels, H, W) by ``scale_factor`` with reassembly
    kernels predicted from the content.  Constructor and state-dict keys (``channel_compressor.*``,
    ``content_encoder.*``) are mmdetection's.  ``forward(x, out_size=(Ho, Wo), addend=t)`` crops the result top-left
    and adds ``t`` in the same launch.  ``x``: bf16 / fp16 CUDA tensor; ``channels`` a multiple of 64 that ``up_group``
    divides into multiples of 8; ``compressed_channels`` a multiple of 64 in 64..512; ``up_kernel`` odd in 1..7,
    ``scale_factor`` in 1..4; ``encoder_kernel`` 3 and ``encoder_dilation`` 1 only (NotImplementedError otherwise: the
    pyramid conv is 3x3, pad 1)."""

    def __init__(self, channels, scale_factor, up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1,
                 compressed_channels=64):
        super(CARAFEPack, self).__init__()
        if encoder_kernel != 3 or encoder_dilation != 1:
            raise NotImplementedError("CARAFEPack(encoder_kernel=%r, encoder_dilation=%r): the content encoder runs on the "
                                      "pyramid conv, which is 3x3 with padding 1 and dilation 1" % (
                                          encoder_kernel, encoder_dilation))
        q = carafe_ops.geometry(1, channels, 1, 1, up_kernel, up_group, scale_factor)
        cm = integer(compressed_channels, "compressed_channels", 64, pyramid_ops.MAX_CIN)
        if cm % 64:
            raise ValueError("compressed_channels must be a multiple of 64 in 64..%d, got %d" % (pyramid_ops.MAX_CIN, cm))
        self.channels, self.scale_factor = q.C, q.s
        self.up_kernel, self.up_group = q.k, q.g
        self.encoder_kernel, self.encoder_dilation = 3, 1
        self.compressed_channels = cm
        self.channel_compressor = nn.Conv2d(q.C, cm, 1)
        self.content_encoder = nn.Conv2d(cm, q.channels(True), 3, padding=1)
        self.content_encoder.weight.data = self.content_encoder.weight.data.contiguous(memory_format=torch.channels_last)
        self.init_weights()

    def init_weights(self):
        """xavier-uniform for both convs (bias 0), then normal std 0.001 on the encoder (mmdetection's)."""
        for m in (self.channel_compressor, self.content_encoder):
            xavier_init(m, distribution='uniform')
        normal_init(self.content_encoder, std=0.001)

    def _unit(self, dtype):
        cache = self.__dict__.setdefault('_hip_units', {})
        u = cache.get(('carafe', dtype))
        if u is None:
            u = cache[('carafe', dtype)] = CarafeUnit(self, dtype)
        return u.refresh()

    def forward(self, x, out_size=None, addend=None):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype not in _16:
            carafe_ops._x(x)                               # raises with the usual message
        N, C, H, W = x.shape
        if C != self.channels:
            raise ValueError("x must have %d channels, got %d" % (self.channels, C))
        q = carafe_ops.geometry(N, C, H, W, self.up_kernel, self.up_group, self.scale_factor, out_size)
        if addend is not None and (not isinstance(addend, torch.Tensor) or tuple(addend.shape) != (N, C, q.Ho, q.Wo) or
                                   addend.dtype != x.dtype):
            raise ValueError("addend must be a %s (%d, %d, %d, %d) tensor" % (
                str(x.dtype).replace("torch.", ""), N, C, q.Ho, q.Wo))
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
        x = _nchw(ops.to_nhwc_bf16(x, x.dtype))
        if addend is not None:
            addend = _nchw(ops.to_nhwc_bf16(addend, x.dtype))
        unit = self._unit(x.dtype)
        cc, ce = self.channel_compressor, self.content_encoder
        return CARAFEPackFunction.apply(x, addend, cc.weight, cc.bias, ce.weight, ce.bias, unit, (q.Ho, q.Wo))

    def extra_repr(self):
        return "%d, scale_factor=%d, up_kernel=%d, up_group=%d, compressed_channels=%d" % (
            self.channels, self.scale_factor, self.up_kernel, self.up_group, self.compressed_channels)
