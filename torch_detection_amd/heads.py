"""The RoI heads' learnable parts.

``BBoxHead`` — mmdetection v1's ``SharedFCBBoxHead`` with ``num_shared_fcs`` fully connected layers and
the two predictors ``fc_cls`` / ``fc_reg`` — between ``roi_align`` and ``bbox_head_loss`` / ``bbox_head_detections``.
Every product runs through csrc/linear.hip; the whole head is one autograd node.

``FCNMaskHead`` — mmdetection v1's mask head: ``num_convs`` 3x3 ``ConvModule``s, the 2x2 stride-2
transposed conv + ReLU (csrc/deconv.hip) and the 1x1 ``conv_logits``, run as a linear layer over the pixels
(csrc/linear.hip) — between ``roi_align`` and ``mask_head_loss`` / ``mask_head_masks``.  The convs are the existing conv
modules; the tail (upsampling + logits) is one autograd node."""
import torch
import torch.nn as nn

from . import deconv_ops, linear_ops, ops
from .deconv import DeconvUnit
from .deconv import check_params as check_deconv_params
from .functional import pick_dtype
from .layers import ConvModule
from .linear import LinearUnit, check_params, flatten_input
from .registry import HEADS

__all__ = ["BBoxHead", "BBoxHeadFunction", "FCNMaskHead", "MaskTailFunction"]


class BBoxHeadFunction(torch.autograd.Function):
    """``apply(head, x, w_0, b_0, ..., w_cls, b_cls, w_reg, b_reg)`` -> (cls_score, bbox_pred).

    Saves each layer's 16-bit input; a layer's ReLU mask is read from the next layer's saved input (``mask_src`` of the
    input-gradient launch).  The two predictors are ONE product over their stacked weights, forward and backward: their
    two input gradients are summed in the fp32 accumulator and rounded once."""

    @staticmethod
    def forward(ctx, head, x, *params):
        x2, C, restore = flatten_input(x)
        dtype = x.dtype
        acts, units = [x2], []
        n = len(params) // 2 - 2
        for i in range(n):
            w, b = params[2 * i], params[2 * i + 1]
            O = check_params(w, b, acts[-1].shape[1])
            u = head._unit("fc%d" % i, (w,), dtype, C if i == 0 else None)
            units.append(u)
            acts.append(linear_ops.linear_fwd(acts[-1], u.w_fwd, O, b.detach(), relu=True))
        wc, bc, wr, br = params[2 * n:]
        nc = check_params(wc, bc, acts[-1].shape[1])
        nr = check_params(wr, br, acts[-1].shape[1])
        up = head._unit("pred", (wc, wr), dtype, C if n == 0 else None)
        y = linear_ops.linear_fwd(acts[-1], up.w_fwd, nc + nr, torch.cat([bc.detach(), br.detach()]))
        ctx.save_for_backward(*acts)
        ctx.meta = (units, up, C, restore, nc)
        return y[:, :nc].contiguous(), y[:, nc:].contiguous()

    @staticmethod
    def backward(ctx, g_cls, g_reg):
        acts = ctx.saved_tensors
        units, up, C, restore, nc = ctx.meta
        n = len(units)
        g = torch.cat([g_cls.to(acts[0].dtype), g_reg.to(acts[0].dtype)], 1)
        dwp, dbp = linear_ops.linear_wgrad(acts[n], g, C if n == 0 else None)
        grads = [dwp[:nc], dbp[:nc], dwp[nc:], dbp[nc:]]
        need_dx = ctx.needs_input_grad[1]
        gx = None
        if n or need_dx:
            gx = linear_ops.linear_dgrad(g, up.w_dgrad, mask_src=acts[n] if n else None)
        for i in reversed(range(n)):
            dw, db = linear_ops.linear_wgrad(acts[i], gx, C if i == 0 else None)
            grads = [dw, db] + grads
            if i or need_dx:
                gx = linear_ops.linear_dgrad(gx, units[i].w_dgrad, mask_src=acts[i] if i else None)
        return (None, restore(gx) if need_dx else None) + tuple(grads)


@HEADS.register_module
class BBoxHead(nn.Module):
    """``SharedFCBBoxHead`` of mmdetection v1: ``num_fcs`` shared ``Linear + ReLU`` layers on the flattened
    (R, in_channels, roi_feat_size, roi_feat_size) RoI features, then ``fc_cls`` (num_classes) and ``fc_reg``
    (4 * num_classes, or 4 when ``reg_class_agnostic``).  The parameters live in ``nn.Linear`` containers, so the
    state-dict keys are mmdetection's (``shared_fcs.0.weight`` ... ``fc_reg.bias``); the containers' own forward is never
    called."""

    def __init__(self, num_fcs=2, in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=81,
                 reg_class_agnostic=False):
        super().__init__()
        if num_fcs < 0 or min(in_channels, fc_out_channels, roi_feat_size, num_classes) < 1:
            raise ValueError("BBoxHead: sizes must be positive")
        self.num_fcs = int(num_fcs)
        self.in_channels = int(in_channels)
        self.fc_out_channels = int(fc_out_channels)
        self.roi_feat_size = int(roi_feat_size)
        self.num_classes = int(num_classes)
        self.reg_class_agnostic = bool(reg_class_agnostic)
        last = self.in_channels * self.roi_feat_size ** 2
        self.shared_fcs = nn.ModuleList()
        for _ in range(self.num_fcs):
            self.shared_fcs.append(nn.Linear(last, self.fc_out_channels))
            last = self.fc_out_channels
        self.fc_cls = nn.Linear(last, self.num_classes)
        self.fc_reg = nn.Linear(last, 4 if self.reg_class_agnostic else 4 * self.num_classes)
        self.init_weights()

    def init_weights(self):
        for fc in self.shared_fcs:
            nn.init.xavier_uniform_(fc.weight)
            nn.init.constant_(fc.bias, 0)
        nn.init.normal_(self.fc_cls.weight, 0, 0.01)
        nn.init.constant_(self.fc_cls.bias, 0)
        nn.init.normal_(self.fc_reg.weight, 0, 0.001)
        nn.init.constant_(self.fc_reg.bias, 0)

    def _unit(self, name, sources, dtype, C):
        cache = self.__dict__.setdefault('_hip_units', {})
        u = cache.get((name, dtype, C))
        if u is None or any(a is not b for a, b in zip(u.sources, sources)):
            u = cache[(name, dtype, C)] = LinearUnit(sources, dtype, C)
        return u.refresh()

    def forward(self, x):
        """x: (R, in_channels, S, S) 16-bit RoI features (channels_last is read in place) or their (R, K) flattening ->
        (cls_score (R, num_classes), bbox_pred (R, 4 * num_classes or 4)), contiguous, in the compute dtype."""
        if torch.is_tensor(x) and x.dtype == torch.float32:
            x = x.to(pick_dtype(self, x))
        params = []
        for fc in list(self.shared_fcs) + [self.fc_cls, self.fc_reg]:
            params += [fc.weight, fc.bias]
        return BBoxHeadFunction.apply(self, x, *params)


# ---- the mask head ------------------------------------------------------------------------------------------------------
ROW_CHUNK = 1 << 18        # csrc/linear.hip's row limit (a multiple of its 128-row tile)


def row_chunks(M):
    """[(begin, end)] runs of at most ROW_CHUNK rows covering 0..M; one empty run for M == 0."""
    return [(s, min(M, s + ROW_CHUNK)) for s in range(0, M, ROW_CHUNK)] or [(0, 0)]


class MaskTailFunction(torch.autograd.Function):
    """``apply(head, x, w_up, b_up, w_logits, b_logits)`` -> mask logits (R, classes, 2H, 2W), channels_last memory.

    Forward: deconv + bias + ReLU (one launch), then ``conv_logits`` as ``linear_fwd`` over the (R * 2H * 2W, Cout)
    matrix that the upsampled map is in memory — the path that takes ragged (81-column) outputs.  Backward: the logits'
    ``linear_wgrad`` and ``linear_dgrad`` with ``mask_src`` = the upsampled map, which applies the deconv's ReLU mask for
    free, then the deconv's weight and input gradients.  The pixel rows are cut into chunks of at most 2^18 (the linear
    kernels' row limit): forward and dgrad run per chunk, the logits' weight and bias gradients accumulate with beta = 1
    from the second chunk on, in chunk order."""

    @staticmethod
    def forward(ctx, head, x, w_up, b_up, w_lg, b_lg):
        dtype = x.dtype
        xh = ops.to_nhwc_bf16(x, dtype).permute(0, 3, 1, 2)            # zero-copy for a channels_last input
        Cout = check_deconv_params(w_up, b_up, xh.shape[1])
        ncls = w_lg.shape[0]
        wl = w_lg.view(ncls, -1)
        check_params(wl, b_lg, Cout)
        up = head._deconv_unit(w_up, dtype)
        lg = head._logits_unit(w_lg, wl, dtype)
        y = deconv_ops.deconv2x2_fwd(xh, up.w_fwd, b_up.detach(), relu=True)
        R, _, H2, W2 = y.shape
        y2 = y.permute(0, 2, 3, 1).reshape(R * H2 * W2, Cout)          # a view: y is NHWC memory
        outs = [linear_ops.linear_fwd(y2[s:e], lg.w_fwd, ncls, b_lg.detach()) for s, e in row_chunks(y2.shape[0])]
        z = outs[0] if len(outs) == 1 else torch.cat(outs)
        ctx.save_for_backward(xh, y2)
        ctx.meta = (up, lg, (R, H2, W2, Cout, ncls), tuple(w_lg.shape))
        return z.view(R, H2, W2, ncls).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        xh, y2 = ctx.saved_tensors
        up, lg, (R, H2, W2, Cout, ncls), wshape = ctx.meta
        g2 = g.to(y2.dtype).permute(0, 2, 3, 1).reshape(R * H2 * W2, ncls)   # a view for a channels_last cotangent
        dwl = dbl = None
        gys = []
        for i, (s, e) in enumerate(row_chunks(y2.shape[0])):
            dwl, dbl = linear_ops.linear_wgrad(y2[s:e], g2[s:e], dw=dwl, dbias=dbl, beta=1.0 if i else 0.0)
            gys.append(linear_ops.linear_dgrad(g2[s:e], lg.w_dgrad, mask_src=y2[s:e]))
        gy = (gys[0] if len(gys) == 1 else torch.cat(gys)).view(R, H2, W2, Cout).permute(0, 3, 1, 2)
        dwu, dbu = deconv_ops.deconv2x2_wgrad(xh, gy)
        dx = deconv_ops.deconv2x2_dgrad(gy, up.w_dgrad) if ctx.needs_input_grad[1] else None
        return None, dx, dwu, dbu, dwl.view(wshape), dbl


@HEADS.register_module
class FCNMaskHead(nn.Module):
    """``FCNMaskHead`` of mmdetection v1: ``num_convs`` 3x3 ``ConvModule``s (bias, ReLU) on the
    (R, in_channels, roi_feat_size, roi_feat_size) RoI features, ``upsample`` = ``ConvTranspose2d(C, C, 2, stride=2)`` +
    ReLU and the 1x1 ``conv_logits`` to ``num_classes`` channels (1 when ``class_agnostic``).  The parameters live in
    ``ConvModule`` / ``nn.ConvTranspose2d`` / ``nn.Conv2d`` containers, so the state-dict keys are mmdetection's
    (``convs.0.conv.weight`` ... ``upsample.weight``, ``conv_logits.bias``); the last two containers' own forward is never
    called.  Anything the HIP path does not cover — an ``upsample_method`` other than 'deconv', a ratio other than 2,
    ``normalize``, channel counts that are no multiples of 64 — is accepted by the constructor and raises
    ``NotImplementedError`` in ``forward``."""

    def __init__(self, num_convs=4, roi_feat_size=14, in_channels=256, conv_kernel_size=3, conv_out_channels=256,
                 upsample_method='deconv', upsample_ratio=2, num_classes=81, class_agnostic=False, normalize=None):
        super().__init__()
        if upsample_method not in (None, 'deconv', 'nearest', 'bilinear'):
            raise ValueError('Invalid upsample method {}, accepted methods are "deconv", "nearest", "bilinear"'
                             .format(upsample_method))
        if num_convs < 0 or min(in_channels, conv_out_channels, roi_feat_size, num_classes, conv_kernel_size) < 1:
            raise ValueError("FCNMaskHead: sizes must be positive")
        self.num_convs = int(num_convs)
        self.roi_feat_size = int(roi_feat_size)
        self.in_channels = int(in_channels)
        self.conv_kernel_size = int(conv_kernel_size)
        self.conv_out_channels = int(conv_out_channels)
        self.upsample_method = upsample_method
        self.upsample_ratio = upsample_ratio
        self.num_classes = int(num_classes)
        self.class_agnostic = bool(class_agnostic)
        self.normalize = normalize
        self.with_bias = normalize is None
        self.convs = nn.ModuleList()
        for i in range(self.num_convs):
            self.convs.append(ConvModule(self.in_channels if i == 0 else self.conv_out_channels, self.conv_out_channels,
                                         self.conv_kernel_size, padding=(self.conv_kernel_size - 1) // 2,
                                         normalize=normalize, bias=self.with_bias, activation='relu'))
        up_in = self.conv_out_channels if self.num_convs > 0 else self.in_channels
        if upsample_method is None:
            self.upsample = None
        elif upsample_method == 'deconv':
            self.upsample = nn.ConvTranspose2d(up_in, self.conv_out_channels, self.upsample_ratio,
                                               stride=self.upsample_ratio)
        else:
            self.upsample = nn.Upsample(scale_factor=self.upsample_ratio, mode=upsample_method)
        out_channels = 1 if self.class_agnostic else self.num_classes
        self.conv_logits = nn.Conv2d(self.conv_out_channels if upsample_method == 'deconv' else up_in, out_channels, 1)
        self.init_weights()

    def init_weights(self):
        for m in [self.upsample, self.conv_logits]:
            if m is None or not hasattr(m, 'weight'):
                continue
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(m.bias, 0)

    def _deconv_unit(self, weight, dtype):
        cache = self.__dict__.setdefault('_hip_units', {})
        u = cache.get(('upsample', dtype))
        if u is None or u.weight is not weight:
            u = cache[('upsample', dtype)] = DeconvUnit(weight, dtype)
        return u.refresh()

    def _logits_unit(self, weight, w2d, dtype):
        cache = self.__dict__.setdefault('_hip_units', {})
        ent = cache.get(('conv_logits', dtype))
        if ent is None or ent.param is not weight:
            ent = cache[('conv_logits', dtype)] = LinearUnit((w2d,), dtype, None)
            ent.param = weight
        ent.sources = (w2d,)                 # a fresh (classes, Cout) view of the parameter's current storage
        return ent.refresh()

    def _check_supported(self):
        if self.upsample_method != 'deconv':
            raise NotImplementedError("FCNMaskHead: upsample_method %r is not on the HIP path (only 'deconv')"
                                      % (self.upsample_method,))
        if self.upsample_ratio != 2:
            raise NotImplementedError("FCNMaskHead: upsample_ratio %r is not on the HIP path (only 2)"
                                      % (self.upsample_ratio,))
        if self.normalize is not None:
            raise NotImplementedError("FCNMaskHead: normalize is not on the HIP path")
        if self.in_channels % 64 or self.conv_out_channels % 64:
            raise NotImplementedError("FCNMaskHead: in_channels=%d and conv_out_channels=%d must be multiples of 64 on "
                                      "the HIP path" % (self.in_channels, self.conv_out_channels))

    def forward(self, x):
        """x: (R, in_channels, S, S) RoI features (16-bit channels_last is read in place) -> mask logits
        (R, num_classes or 1, 2S, 2S) in the compute dtype, channels_last memory: what ``mask_head_loss`` and
        ``mask_head_masks`` take in place."""
        self._check_supported()
        if torch.is_tensor(x) and x.dtype == torch.float32:
            x = x.to(pick_dtype(self, x))
        for conv in self.convs:
            x = conv(x)
        return MaskTailFunction.apply(self, x, self.upsample.weight, self.upsample.bias, self.conv_logits.weight,
                                      self.conv_logits.bias)
