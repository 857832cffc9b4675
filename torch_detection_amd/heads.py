"""The RoI heads' learnable parts.

``BBoxHead`` — mmdetection v1's ``SharedFCBBoxHead`` with ``num_shared_fcs`` fully connected layers and
the two predictors ``fc_cls`` / ``fc_reg`` — between ``roi_align`` and ``bbox_head_loss`` / ``bbox_head_detections``.
Every product runs through csrc/linear.hip; the whole head is one autograd node.

``FCNMaskHead`` — mmdetection v1's mask head: ``num_convs`` 3x3 ``ConvModule``s, the 2x2 stride-2
transposed conv + ReLU (csrc/deconv.hip) and the 1x1 ``conv_logits``, run as a linear layer over the pixels
(csrc/linear.hip) — between ``roi_align`` and ``mask_head_loss`` / ``mask_head_masks``.  The convs are the existing conv
modules; the tail (upsampling + logits) is one autograd node.

``RPNHead`` — mmdetection v1's ``RPNHead``: the shared 3x3 ``rpn_conv`` + ReLU (the existing conv path,
level by level) and the two 1x1 predictors ``rpn_cls`` / ``rpn_reg`` over the whole pyramid in one launch per product
(csrc/dense_head.hip) — between ``FPN`` and ``rpn_loss`` / ``rpn_proposals``.  The whole head is one autograd node.

``RetinaHead`` — mmdetection v1's ``RetinaHead``: two towers of 3x3 ``ConvModule``s and the 3x3
predictors ``retina_cls`` / ``retina_reg``, weights shared by the levels, every layer one launch over the whole pyramid
(csrc/pyramid_conv.hip) or the existing conv path level by level, product by product as measured — between ``FPN`` and
``anchor_target_all`` / ``anchor_head_loss`` / ``anchor_head_detections``.  The whole head is one autograd node.

``FCOSHead`` — mmdetection v1's ``FCOSHead``: two towers of 3x3 conv -> GroupNorm -> ReLU layers and the
3x3 predictors ``fcos_cls`` / ``fcos_reg`` / ``fcos_centerness``, weights and affine parameters shared by the levels; the
convs as in ``RetinaHead``, the GroupNorm of a layer in three launches over the whole pyramid each way
(csrc/pyramid_gn.hip) — between ``FPN`` and ``fcos_target`` / ``fcos_loss`` / ``fcos_detections``.  One autograd node.

``MaskIoUHead`` — mmdetection v1's ``MaskIoUHead`` of Mask Scoring R-CNN: a 3x3 conv over the mask head's
features and its pooled predicted mask (``mask_iou_stem``, csrc/mask_iou.hip), further 3x3 convs (the last of stride 2),
fully connected layers and the ragged ``fc_mask_iou`` — beside ``FCNMaskHead``, between ``roi_align`` and
``mask_iou_loss`` / ``mask_scores``."""
import math

import torch
import torch.nn as nn

from . import dense_ops, deconv_ops, linear_ops, ops, pyramid_ops
from . import functional as HF
from .box import AnchorGenerator, anchor_pyramid, rpn_proposals
from .dense_detect import anchor_head_detections, anchor_target_all
from .deconv import DeconvUnit
from .deconv import check_params as check_deconv_params
from .functional import pick_dtype
from .fcos import fcos_detections, fcos_loss, fcos_points, fcos_target
from .ghm import GHMC, GHMR, ghm_head_loss
from .layers import ConvModule, Scale
from .linear import LinearUnit, check_params, flatten_input
from .linear import linear as _linear
from .mask_iou import MaskIoUStemFunction, MaskIoUStemUnit, mask_iou_loss, mask_iou_target, mask_scores
from .losses import anchor_head_loss, rpn_loss
from .registry import HEADS
from .target import anchor_target

__all__ = ["BBoxHead", "BBoxHeadFunction", "FCNMaskHead", "MaskTailFunction", "MaskIoUHead", "RPNHead", "RPNHeadFunction", "PredUnit",
           "RetinaHead", "RetinaHeadFunction", "PyrUnit", "FCOSHead", "FCOSHeadFunction"]


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


# ---- the mask-IoU head (Mask Scoring R-CNN) --------------------------------------------------------------------------------
@HEADS.register_module
class MaskIoUHead(nn.Module):
    """``MaskIoUHead`` of mmdetection v1 (Mask Scoring R-CNN): ``num_convs`` 3x3 convs + ReLU, the first over
    ``cat(mask_feat, max_pool2x2(sigmoid(mask_pred[r, label_r])))`` (``in_channels + 1`` inputs), the LAST of stride 2;
    ``num_fcs`` ``Linear + ReLU`` layers on the flattened map and ``fc_mask_iou`` to ``num_classes`` outputs.  The
    parameters live in plain ``nn.Conv2d`` / ``nn.Linear`` containers, so the state-dict keys are mmdetection's
    (``convs.0.weight`` ... ``fcs.1.bias``, ``fc_mask_iou.weight``); the containers' own forward is never called.
    Anything the HIP path does not cover — channel counts that are no multiples of 64, fewer than two convs, an odd
    ``roi_feat_size``, a ``loss_iou`` other than ``MSELoss`` — is accepted by the constructor and raises
    ``NotImplementedError`` in ``forward``."""

    def __init__(self, num_convs=4, num_fcs=2, roi_feat_size=14, in_channels=256, conv_out_channels=256,
                 fc_out_channels=1024, num_classes=81, loss_iou=dict(type='MSELoss', loss_weight=0.5)):
        super().__init__()
        if num_convs < 1 or num_fcs < 0 or min(roi_feat_size, in_channels, conv_out_channels, fc_out_channels,
                                               num_classes) < 1:
            raise ValueError("MaskIoUHead: sizes must be positive")
        self.num_convs = int(num_convs)
        self.num_fcs = int(num_fcs)
        self.roi_feat_size = int(roi_feat_size)
        self.in_channels = int(in_channels)
        self.conv_out_channels = int(conv_out_channels)
        self.fc_out_channels = int(fc_out_channels)
        self.num_classes = int(num_classes)
        self.loss_iou = dict(loss_iou)
        self.loss_weight = float(self.loss_iou.get('loss_weight', 1.0))
        self.convs = nn.ModuleList()
        for i in range(self.num_convs):
            cin = self.in_channels + 1 if i == 0 else self.conv_out_channels
            self.convs.append(nn.Conv2d(cin, self.conv_out_channels, 3, stride=2 if i == self.num_convs - 1 else 1,
                                        padding=1))
        pooled = self.roi_feat_size // 2
        self.fcs = nn.ModuleList()
        for i in range(self.num_fcs):
            fin = self.conv_out_channels * pooled * pooled if i == 0 else self.fc_out_channels
            self.fcs.append(nn.Linear(fin, self.fc_out_channels))
        last = self.fc_out_channels if self.num_fcs else self.conv_out_channels * pooled * pooled
        self.fc_mask_iou = nn.Linear(last, self.num_classes)
        self.init_weights()

    def init_weights(self):
        for conv in self.convs:
            nn.init.kaiming_normal_(conv.weight, mode='fan_out', nonlinearity='relu')
            nn.init.constant_(conv.bias, 0)
        for fc in self.fcs:
            nn.init.kaiming_uniform_(fc.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
            nn.init.constant_(fc.bias, 0)
        nn.init.normal_(self.fc_mask_iou.weight, 0, 0.01)
        nn.init.constant_(self.fc_mask_iou.bias, 0)

    def _stem_unit(self, weight, dtype):
        cache = self.__dict__.setdefault('_hip_units', {})
        u = cache.get(('stem', dtype))
        if u is None or u.weight is not weight:
            u = cache[('stem', dtype)] = MaskIoUStemUnit(weight, dtype)
        return u

    def _check_supported(self):
        if self.in_channels % 64 or self.conv_out_channels % 64:
            raise NotImplementedError("MaskIoUHead: in_channels=%d and conv_out_channels=%d must be multiples of 64 on "
                                      "the HIP path" % (self.in_channels, self.conv_out_channels))
        if self.num_convs < 2:
            raise NotImplementedError("MaskIoUHead: num_convs=%d is not on the HIP path (the first conv runs at stride "
                                      "1: at least 2)" % self.num_convs)
        if self.roi_feat_size % 2:
            raise NotImplementedError("MaskIoUHead: an odd roi_feat_size (%d) is not on the HIP path" % self.roi_feat_size)
        if self.loss_iou.get('type') != 'MSELoss':
            raise NotImplementedError("MaskIoUHead: loss_iou type %r is not on the HIP path (only 'MSELoss')"
                                      % (self.loss_iou.get('type'),))

    def forward(self, mask_feat, mask_pred, labels=None, label_offset=0):
        """mask_feat: (R, in_channels, S, S) RoI features of the mask branch (16-bit channels_last is read in place);
        mask_pred: (R, C, 2S, 2S) logits of ``FCNMaskHead`` (read in place); labels (R,) int64: row r pools channel
        ``labels[r] + label_offset`` (None: channel 0 of a class-agnostic ``mask_pred``) -> mask_iou_pred
        (R, num_classes) float32."""
        self._check_supported()
        if torch.is_tensor(mask_feat) and mask_feat.dtype == torch.float32:
            mask_feat = mask_feat.to(pick_dtype(self, mask_feat)).contiguous(memory_format=torch.channels_last)
        dtype = mask_feat.dtype
        if labels is None:
            if mask_pred.dim() == 4 and mask_pred.shape[1] != 1:
                raise ValueError("MaskIoUHead: labels are needed to pick a channel of a %d-channel mask_pred"
                                 % mask_pred.shape[1])
            labels = torch.zeros(mask_pred.shape[0], dtype=torch.int64, device=mask_pred.device)
        c0 = self.convs[0]
        x = MaskIoUStemFunction.apply(mask_feat, mask_pred, labels, c0.weight, c0.bias, int(label_offset), True,
                                      self._stem_unit(c0.weight, dtype))
        for i in range(1, self.num_convs):
            unit = HF.prepare_unit(self, 'conv%d' % i, self.convs[i], None, True, dtype)
            x = HF.ConvUnitFunction.apply(unit, x, *unit.params())
        for fc in self.fcs:
            x = _linear(x, fc.weight, fc.bias, relu=True)
        return _linear(x, self.fc_mask_iou.weight, self.fc_mask_iou.bias, out_f32=True)

    def get_target(self, rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_pred, labels,
                   mask_targets, img_shapes, thr=0.5):
        """:func:`mask_iou_target` (mmdetection's ``get_target`` with ``rcnn_train_cfg.mask_thr_binary`` as ``thr``)."""
        return mask_iou_target(rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_pred, labels,
                               mask_targets, img_shapes, thr)

    def loss(self, mask_iou_pred, labels, mask_iou_targets):
        return dict(loss_mask_iou=mask_iou_loss(mask_iou_pred, labels, mask_iou_targets, self.loss_weight))

    def get_mask_scores(self, mask_iou_pred, dets, labels, counts):
        """:func:`mask_scores`."""
        return mask_scores(mask_iou_pred, dets, labels, counts)


# ---- the RPN head -------------------------------------------------------------------------------------------------------
class PredUnit(object):
    """Packed 16-bit operands of the stacked predictor weight (``rpn_cls`` rows, then ``rpn_reg`` rows) for one compute
    dtype, cached like ``LinearUnit`` / ``DeconvUnit``: under a version key (data pointers, ``_version``s, device); an
    in-place update re-packs into the same buffers, ``invalidate_packed`` drops the key, and inside a graph capture the
    pack is enqueued again when ``functional.REPACK_IN_CAPTURE`` is set."""

    def __init__(self, w_cls, w_reg, dtype):
        self.sources = (w_cls, w_reg)
        self.dtype = dtype
        self.key = None
        self.w_fwd = self.w_dgrad = None
        self._layout = None

    def _version_key(self):
        return (self.dtype,) + tuple((w.data_ptr(), w._version, w.device) for w in self.sources)

    def refresh(self):
        wc, wr = self.sources
        if not wc.is_cuda:
            raise RuntimeError('torch_detection_amd modules run on the MI355X HIP path only: move the module to '
                               'a CUDA/HIP device (no CPU fallback)')
        key = self._version_key()
        capturing = HF.REPACK_IN_CAPTURE and torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        layout = (wc.device, self.dtype, tuple(wc.shape), tuple(wr.shape))
        reuse = self.w_fwd is not None and layout == self._layout
        self._layout = layout
        with torch.no_grad():
            self.w_fwd, self.w_dgrad = dense_ops.pack_pred_weight(
                wc.detach(), wr.detach(), True, self.dtype, out=(self.w_fwd, self.w_dgrad) if reuse else None)
        self.key = key
        return self


class RPNHeadFunction(torch.autograd.Function):
    """``apply(head, n, feat_0 .. feat_{n-1}, w_conv, b_conv, w_cls, b_cls, w_reg, b_reg)`` ->
    (cls_0 .. cls_{n-1}, reg_0 .. reg_{n-1}).

    Forward: ``rpn_conv`` + ReLU level by level through the conv unit, then ONE ``pred_fwd`` over the pyramid.
    Backward: ``pred_wgrad`` (two launches), then ONE ``pred_dgrad`` whose mask source is the hidden maps themselves —
    the ReLU mask costs no launch —, then ``rpn_conv``'s weight gradients level by level on one shared ``WgradQueue``
    flushed once, then its input gradients where an input needs one.  The shared ``rpn_conv`` weight and bias gradients
    are the float32 sum of the per-level gradients in level order, finest (first) level first:
    ``((g_0 + g_1) + g_2) + ...``."""

    @staticmethod
    def forward(ctx, head, n, *args):
        feats, (w_conv, b_conv, w_cls, b_cls, w_reg, b_reg) = args[:n], args[n:]
        dtype = HF.pick_dtype(head, feats)
        unit = HF.prepare_unit(head, 'rpn_conv', head.rpn_conv, None, True, dtype)
        if unit.sink is not None:
            raise NotImplementedError("RPNHead: rpn_conv's per-level gradients cannot be written into a gradient bucket")
        pred = head._pred_unit(dtype)
        xs = [ops.to_nhwc_bf16(f, dtype) for f in feats]                  # zero-copy for channels_last 16-bit maps
        hs = [HF.unit_fwd(unit, x).permute(0, 3, 1, 2) for x in xs]       # ReLU fused
        cls, reg = dense_ops.pred_fwd(hs, pred.w_fwd, b_cls.detach(), b_reg.detach())
        ctx.save_for_backward(*xs, *hs)
        # (dtype, plain NCHW-contiguous?) of every input: its gradient comes back in the same dtype and layout
        ctx.meta = (unit, pred, n, [(f.dtype, f.is_contiguous() and not f.permute(0, 2, 3, 1).is_contiguous())
                                    for f in feats])
        return tuple(cls) + tuple(reg)

    @staticmethod
    def backward(ctx, *gs):
        unit, pred, n, layouts = ctx.meta
        xs, hs = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        dtype = hs[0].dtype
        B, C = hs[0].shape[:2]
        A = pred.sources[0].shape[0]
        sizes = [tuple(h.shape[2:]) for h in hs]
        zero = lambda g, ch, hw: torch.zeros((B, hw[0], hw[1], ch), dtype=dtype, device=hs[0].device).permute(0, 3, 1, 2) \
            if g is None else g
        g_cls = dense_ops.cotangents([zero(g, A, s) for g, s in zip(gs[:n], sizes)], "g_cls", dtype, B, A, sizes)
        g_reg = dense_ops.cotangents([zero(g, 4 * A, s) for g, s in zip(gs[n:], sizes)], "g_reg", dtype, B, 4 * A, sizes)
        dwc, dbc, dwr, dbr = dense_ops.pred_wgrad(hs, g_cls, g_reg)
        dhs = [d.permute(0, 2, 3, 1) for d in dense_ops.pred_dgrad(g_cls, g_reg, pred.w_dgrad, hs)]   # masked by h > 0
        dev = dhs[0].device
        wq = HF.WgradQueue(dev)
        per_level = [HF.unit_wgrad(unit, x, dh, queue=wq) for x, dh in zip(xs, dhs)]
        wq.flush()
        dxs = []
        for l, (x, dh) in enumerate(zip(xs, dhs)):
            dx = None
            if ctx.needs_input_grad[2 + l]:
                dx = HF.unit_dgrad(unit, dh, (x.shape[1], x.shape[2])).permute(0, 3, 1, 2)
                in_dtype, nchw = layouts[l]
                if dx.dtype != in_dtype:
                    dx = dx.to(in_dtype)
                if nchw:                                                  # the input's own layout
                    dx = dx.contiguous()
            dxs.append(dx)
        HF.join_side_stream(dev)
        dw, db = per_level[0]
        for gw, gb in per_level[1:]:                                      # level order, finest first
            dw, db = dw + gw, db + gb
        return (None, None) + tuple(dxs) + (dw, db, dwc, dbc, dwr, dbr)


@HEADS.register_module
class RPNHead(nn.Module):
    """``RPNHead`` of mmdetection v1: the 3x3 ``rpn_conv`` (in_channels -> feat_channels, bias, ReLU), shared by all
    pyramid levels, and the two 1x1 predictors ``rpn_cls`` (A channels, A = len(anchor_scales) * len(anchor_ratios)) and
    ``rpn_reg`` (4A channels).  The parameters live in ``nn.Conv2d`` containers, so the state-dict keys and shapes are
    mmdetection's (``rpn_conv.weight`` ... ``rpn_reg.bias``); the containers' own forward is never called.  What the HIP
    path does not cover — ``use_sigmoid_cls=False``, 5A > 64, channel counts that are no multiples of 64 or above 512 —
    is accepted by the constructor and raises ``NotImplementedError`` in ``forward``."""

    def __init__(self, in_channels=256, feat_channels=256, anchor_scales=(8,), anchor_ratios=(0.5, 1.0, 2.0),
                 anchor_strides=(4, 8, 16, 32, 64), anchor_base_sizes=None, target_means=(0, 0, 0, 0),
                 target_stds=(1, 1, 1, 1), use_sigmoid_cls=True):
        super().__init__()
        if min(in_channels, feat_channels) < 1 or not len(anchor_scales) or not len(anchor_ratios) or \
                not len(anchor_strides):
            raise ValueError("RPNHead: sizes must be positive and the anchor lists non-empty")
        self.in_channels = int(in_channels)
        self.feat_channels = int(feat_channels)
        self.anchor_scales = list(anchor_scales)
        self.anchor_ratios = list(anchor_ratios)
        self.anchor_strides = list(anchor_strides)
        self.anchor_base_sizes = list(anchor_strides) if anchor_base_sizes is None else list(anchor_base_sizes)
        if len(self.anchor_base_sizes) != len(self.anchor_strides):
            raise ValueError("RPNHead: one anchor base size per stride")
        self.target_means = tuple(target_means)
        self.target_stds = tuple(target_stds)
        self.use_sigmoid_cls = bool(use_sigmoid_cls)
        self.anchor_generators = [AnchorGenerator(b, self.anchor_scales, self.anchor_ratios)
                                  for b in self.anchor_base_sizes]
        self.num_anchors = len(self.anchor_ratios) * len(self.anchor_scales)
        self.rpn_conv = nn.Conv2d(self.in_channels, self.feat_channels, 3, padding=1)
        if self.in_channels % 64 == 0:                   # the conv path's K-major layout (layers._channels_last_)
            self.rpn_conv.weight.data = self.rpn_conv.weight.data.contiguous(memory_format=torch.channels_last)
        self.rpn_cls = nn.Conv2d(self.feat_channels, self.num_anchors * (1 if self.use_sigmoid_cls else 2), 1)
        self.rpn_reg = nn.Conv2d(self.feat_channels, self.num_anchors * 4, 1)
        self.init_weights()

    def init_weights(self):
        for m in (self.rpn_conv, self.rpn_cls, self.rpn_reg):
            nn.init.normal_(m.weight, 0, 0.01)
            nn.init.constant_(m.bias, 0)

    def _pred_unit(self, dtype):
        cache = self.__dict__.setdefault('_hip_units', {})
        u = cache.get(('pred', dtype))
        wc, wr = self.rpn_cls.weight, self.rpn_reg.weight
        if u is None or u.sources[0] is not wc or u.sources[1] is not wr:
            u = cache[('pred', dtype)] = PredUnit(wc, wr, dtype)
        return u.refresh()

    def _check_supported(self):
        if not self.use_sigmoid_cls:
            raise NotImplementedError("RPNHead: use_sigmoid_cls=False (a softmax RPN) is not on the HIP path")
        if 5 * self.num_anchors > 64 or self.num_anchors > dense_ops.MAX_A:
            raise NotImplementedError("RPNHead: %d anchors per cell are not on the HIP path (at most %d)"
                                      % (self.num_anchors, dense_ops.MAX_A))
        for name, c in (("in_channels", self.in_channels), ("feat_channels", self.feat_channels)):
            if c % 64 or c > dense_ops.MAX_C:
                raise NotImplementedError("RPNHead: %s=%d must be a multiple of 64, at most %d, on the HIP path"
                                          % (name, c, dense_ops.MAX_C))

    def forward(self, feats):
        """feats: a list of 1..8 (B, in_channels, H_l, W_l) maps (16-bit channels_last is read in place, float32 is
        converted as in the other heads) -> (cls_scores, bbox_preds): lists of (B, A, H_l, W_l) and (B, 4A, H_l, W_l)
        tensors in the compute dtype, channel order ``a`` and ``4a + j``, channels_last memory: what ``rpn_loss``,
        ``anchor_head_loss`` and ``rpn_proposals`` take in place."""
        self._check_supported()
        feats = list(feats)
        if not 1 <= len(feats) <= dense_ops.MAX_LEVELS:
            raise ValueError("feats must be a list of 1..%d levels, got %d" % (dense_ops.MAX_LEVELS, len(feats)))
        if torch.is_tensor(feats[0]) and feats[0].dtype == torch.float32:
            dtype = pick_dtype(self, feats[0])
            feats = [f.to(dtype) for f in feats]
        n = len(feats)
        out = RPNHeadFunction.apply(self, n, *feats, self.rpn_conv.weight, self.rpn_conv.bias, self.rpn_cls.weight,
                                    self.rpn_cls.bias, self.rpn_reg.weight, self.rpn_reg.bias)
        return list(out[:n]), list(out[n:])

    def get_anchors(self, featmap_sizes, valid_sizes=None, device='cuda'):
        """(anchors, valid_flags): per-level lists from one ``anchor_pyramid`` launch over the head's own generators."""
        n = len(featmap_sizes)
        return anchor_pyramid(self.anchor_generators[:n], featmap_sizes, self.anchor_strides[:n], device, valid_sizes)

    def loss(self, cls_scores, bbox_preds, anchors, valid_flags, gt_bboxes, gt_counts, img_shapes, **target_cfg):
        """``anchor_target`` with the head's means / stds, then ``rpn_loss`` averaged over the sampled anchors
        (``avg_factor=(num_pos, num_neg)``): -> losses (2,) = [loss_cls, loss_bbox].  ``anchors`` / ``valid_flags``: what
        ``get_anchors`` returned (per-level lists) or their concatenation."""
        cat = lambda t: torch.cat(list(t)) if isinstance(t, (list, tuple)) else t
        cfg = dict(target_means=self.target_means, target_stds=self.target_stds)
        cfg.update(target_cfg)
        labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, _ = anchor_target(
            cat(anchors), cat(valid_flags), gt_bboxes, gt_counts, img_shapes, **cfg)
        return rpn_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights,
                        avg_factor=(num_pos, num_neg))

    def get_proposals(self, cls_scores, bbox_preds, anchors, img_shapes, **proposal_cfg):
        """``rpn_proposals`` with the head's means / stds on the head's outputs, in place.  ``rpn_proposals`` takes
        float32 or bfloat16 only: float16 outputs are cast to float32 first (one copy per map)."""
        if cls_scores[0].dtype == torch.float16:
            cls_scores = [t.float() for t in cls_scores]
            bbox_preds = [t.float() for t in bbox_preds]
        cfg = dict(target_means=self.target_means, target_stds=self.target_stds)
        cfg.update(proposal_cfg)
        return rpn_proposals(cls_scores, bbox_preds, anchors, img_shapes, **cfg)


# ---- the RetinaNet head -------------------------------------------------------------------------------------------------
PYRAMID, COMPOSED, SPLIT = 'pyramid', 'composed', 'split'
# Route of every product of every Cout class, decided by measurement (profiles/pyramid_conv_bench.jsonl)
# with §4k's rule: a product stays on the pyramid kernel where its slowest repeat is below the composed form's fastest.
# 'split': the levels of at least SPLIT_PIXELS pixels (B * H * W) level by level on the tuned conv path, the tail levels in
# one pyramid launch — taken where it measured below both.
RETINA_ROUTES = {
    'tower': {'fwd': SPLIT, 'dgrad': SPLIT, 'wgrad': COMPOSED},
    'cls': {'fwd': SPLIT, 'dgrad': SPLIT, 'wgrad': COMPOSED},
    'reg': {'fwd': PYRAMID, 'dgrad': SPLIT, 'wgrad': COMPOSED},
}
RETINA_COMPOSED = {k: {p: COMPOSED for p in ('fwd', 'dgrad', 'wgrad')} for k in ('tower', 'cls', 'reg')}
# between the second and the third level of the measured pyramid (8 400 and 2 100 pixels): the split that was timed
SPLIT_PIXELS = 4096


def split_levels(maps):
    """(indices of the levels the split route runs level by level, indices of its pyramid launch)"""
    big = [l for l, t in enumerate(maps) if t.shape[0] * t.shape[2] * t.shape[3] >= SPLIT_PIXELS]
    return big, [l for l in range(len(maps)) if l not in big]


class PyrUnit(object):
    """Packed 16-bit operands of one shared 3x3 weight (``pyramid_ops.pack_pyramid_weight``) for one compute dtype,
    cached under ``PredUnit``'s rules: a version key (data pointer, ``_version``, device); an in-place update re-packs
    into the same buffers, ``invalidate_packed`` drops the key, and inside a graph capture the pack is enqueued again
    when ``functional.REPACK_IN_CAPTURE`` is set."""

    def __init__(self, weight, dtype):
        self.sources = (weight,)
        self.dtype = dtype
        self.key = None
        self.w_fwd = self.w_dgrad = None
        self._layout = None

    def refresh(self):
        w = self.sources[0]
        if not w.is_cuda:
            raise RuntimeError('torch_detection_amd modules run on the MI355X HIP path only: move the module to '
                               'a CUDA/HIP device (no CPU fallback)')
        key = (self.dtype, w.data_ptr(), w._version, w.device)
        capturing = HF.REPACK_IN_CAPTURE and torch.cuda.is_current_stream_capturing()
        if key == self.key and not capturing:
            return self
        layout = (w.device, self.dtype, tuple(w.shape))
        reuse = self.w_fwd is not None and layout == self._layout
        self._layout = layout
        with torch.no_grad():
            self.w_fwd, self.w_dgrad = pyramid_ops.pack_pyramid_weight(
                w.detach(), True, self.dtype, out=(self.w_fwd, self.w_dgrad) if reuse else None)
        self.key = key
        return self


class _Layer(object):
    """One shared 3x3 conv of the head during one forward / backward: its parameters, its Cout class (the routing key),
    and the operands of the routes in use — the ``PyrUnit`` and / or the ``ConvUnit`` of the composition (for a
    predictor: of a hidden conv whose weight and bias are the parameter zero padded to the next multiple of 64)."""

    def __init__(self, head, name, conv, kind, relu, dtype):
        self.name, self.kind, self.relu = name, kind, relu
        self.weight, self.bias = conv.weight, conv.bias
        self.Cout, self.Cin = conv.weight.shape[:2]
        self.Cp = -(-self.Cout // 64) * 64
        routes = head._routes[kind]
        self.routes = routes
        self.pyr = self.unit = None
        self._pads = {}
        if PYRAMID in routes.values() or SPLIT in routes.values():
            self.pyr = head._pyr_unit(name, conv.weight, dtype)
        if COMPOSED in routes.values() or SPLIT in routes.values():
            if self.Cp != self.Cout:
                conv = head._padded_conv(name, conv, self.Cp)
            self.unit = HF.prepare_unit(head, name + '.composed', conv, None, relu, dtype)
            if self.unit.sink is not None:
                raise NotImplementedError("RetinaHead: %s's per-level gradients cannot be written into a gradient "
                                          "bucket" % name)

    @staticmethod
    def _pick(ts, idx):
        return None if ts is None else [ts[l] for l in idx]

    def _routed(self, route, maps, pyramid, composed):
        """The levels of ``maps`` through ``pyramid(indices)`` / ``composed(indices)`` as the route says, in level order"""
        every = list(range(len(maps)))
        big, tail = (every, []) if route == COMPOSED else ([], every) if route == PYRAMID else split_levels(maps)
        out = [None] * len(maps)
        for idx, fn in ((big, composed), (tail, pyramid)):
            if idx:
                for l, t in zip(idx, fn(idx)):
                    out[l] = t
        return out

    # every map below is a logical (B, C, H, W) tensor in channels_last memory
    def fwd(self, xs):
        def composed(idx):
            ys = [HF.unit_fwd(self.unit, xs[l].permute(0, 2, 3, 1)).permute(0, 3, 1, 2) for l in idx]
            return [_dense_channels(y, self.Cout) for y in ys] if self.Cp != self.Cout else ys   # the slicing copies
        return self._routed(self.routes['fwd'], xs, lambda idx: pyramid_ops.pyramid_conv_fwd(
            self._pick(xs, idx), self.pyr.w_fwd, self.bias.detach(), self.Cout, self.relu), composed)

    def _padded(self, g):
        """A cotangent as the composition reads it: (B, H, W, Cp) with zero pad channels — one copy, shared by the input
        and the weight gradient."""
        if self.Cp == self.Cout:
            return g.permute(0, 2, 3, 1)
        hit = self._pads.get(id(g))
        if hit is None or hit[0] is not g:
            B, _, H, W = g.shape
            p = torch.zeros((B, H, W, self.Cp), dtype=g.dtype, device=g.device)
            p[..., :self.Cout].copy_(g.permute(0, 2, 3, 1))
            hit = self._pads[id(g)] = (g, p)
        return hit[1]

    def dgrad(self, gs, mask_src=None, addend=None):
        def composed(idx):
            out = []
            for l in idx:
                g = self._padded(gs[l])
                a = addend[l].permute(0, 2, 3, 1) if addend is not None else None
                m = mask_src[l].permute(0, 2, 3, 1) if mask_src is not None else None
                out.append(HF.unit_dgrad(self.unit, g, (g.shape[1], g.shape[2]), a, HF.ADD_SAME if a is not None else
                                         HF.ADD_NONE, m).permute(0, 3, 1, 2))
            return out
        return self._routed(self.routes['dgrad'], gs, lambda idx: pyramid_ops.pyramid_conv_dgrad(
            self._pick(gs, idx), self.pyr.w_dgrad, self._pick(mask_src, idx), self._pick(addend, idx)), composed)

    def wgrad(self, xs, gs, queue):
        """-> a thunk giving (dw, dbias) once the queue has been flushed and the side streams joined."""
        if self.routes['wgrad'] == PYRAMID:
            grads = pyramid_ops.pyramid_conv_wgrad(xs, gs, self.weight.permute(0, 2, 3, 1).is_contiguous())
            return lambda: grads
        if self.routes['wgrad'] != COMPOSED:
            raise ValueError("RetinaHead: the weight gradient has the routes 'pyramid' and 'composed', got %r"
                             % (self.routes['wgrad'],))
        per_level = [HF.unit_wgrad(self.unit, x.permute(0, 2, 3, 1), self._padded(g), queue=queue)
                     for x, g in zip(xs, gs)]

        def total():
            dw, db = per_level[0]
            for gw, gb in per_level[1:]:                              # level order, finest first
                dw, db = dw + gw, db + gb
            return (dw[:self.Cout], db[:self.Cout]) if self.Cp != self.Cout else (dw, db)
        return total


def _dense_channels(y, C):
    """The first C channels of a channels_last map as a dense channels_last map of its own."""
    B, _, H, W = y.shape
    out = torch.empty((B, H, W, C), dtype=y.dtype, device=y.device).permute(0, 3, 1, 2)
    out.copy_(y[:, :C])
    return out


class RetinaHeadFunction(torch.autograd.Function):
    """``apply(head, n, feat_0 .. feat_{n-1}, *parameters)`` -> (cls_0 .. cls_{n-1}, reg_0 .. reg_{n-1}); the parameters
    in ``head.parameters()`` order (cls tower, reg tower, ``retina_cls``, ``retina_reg``; weight, bias each).

    Forward: the two towers layer by layer (bias and ReLU fused), then the two predictors; every layer is ONE launch
    over the pyramid on the pyramid route, one launch per level on the composed route (``head._routes``).  Backward: the
    predictors' weight gradients, their input gradients masked by the last hidden maps, then down each tower — a
    layer's weight gradient from the map below and the gradient above, its input gradient masked by the map below —;
    the two first layers' input gradients meet in ``dfeats[l]``: the cls chain's is the addend of the reg chain's launch,
    summed in fp32 and rounded once."""

    @staticmethod
    def forward(ctx, head, n, *args):
        feats = args[:n]
        dtype = HF.pick_dtype(head, feats)
        chains = head._chains(dtype)
        xs = [ops.to_nhwc_bf16(f, dtype).permute(0, 3, 1, 2) for f in feats]   # zero-copy for channels_last 16-bit maps
        acts = []
        for chain in chains:
            maps = [xs]
            for layer in chain:
                maps.append(layer.fwd(maps[-1]))
            acts.append(maps)
        ctx.save_for_backward(*[t for maps in acts for level in maps[:-1] for t in level])
        ctx.meta = (chains, n, [(f.dtype, f.is_contiguous() and not f.permute(0, 2, 3, 1).is_contiguous())
                                for f in feats])
        return tuple(acts[0][-1]) + tuple(acts[1][-1])

    @staticmethod
    def backward(ctx, *gs):
        chains, n, layouts = ctx.meta
        saved = list(ctx.saved_tensors)
        acts = []
        for chain in chains:
            acts.append([saved[i * n:(i + 1) * n] for i in range(len(chain))])
            saved = saved[len(chain) * n:]
        dtype, dev = acts[0][0][0].dtype, acts[0][0][0].device
        B = acts[0][0][0].shape[0]
        sizes = [tuple(x.shape[2:]) for x in acts[0][0]]
        need_dx = any(ctx.needs_input_grad[2:2 + n])
        wq = HF.WgradQueue(dev)
        thunks, first_dx = [], None
        for ci, (chain, maps, g) in enumerate(zip(chains, acts, (gs[:n], gs[n:]))):
            ch = chain[-1].Cout
            g = [torch.zeros((B, H, W, ch), dtype=dtype, device=dev).permute(0, 3, 1, 2) if t is None else t
                 for t, (H, W) in zip(g, sizes)]
            g = dense_ops.cotangents(g, "g_cls" if ci == 0 else "g_reg", dtype, B, ch, sizes)
            mine = []
            for i in reversed(range(len(chain))):
                mine.append(chain[i].wgrad(maps[i], g, wq))
                if i:
                    g = chain[i].dgrad(g, mask_src=maps[i])
                elif need_dx:
                    g = chain[i].dgrad(g, addend=first_dx)
                    first_dx = g
            thunks.append(mine[::-1])
        wq.flush()
        dxs = []
        for l in range(n):
            dx = None
            if ctx.needs_input_grad[2 + l]:
                dx = first_dx[l]
                in_dtype, nchw = layouts[l]
                if dx.dtype != in_dtype:
                    dx = dx.to(in_dtype)
                if nchw:                                                  # the input's own layout
                    dx = dx.contiguous()
            dxs.append(dx)
        HF.join_side_stream(dev)
        grads = []
        for mine in (thunks[0][:-1], thunks[1][:-1], thunks[0][-1:], thunks[1][-1:]):
            for t in mine:
                grads += list(t())
        return (None, None) + tuple(dxs) + tuple(grads)


def _ghm_pair(loss_cls, loss_bbox):
    """``RetinaHead``'s ``loss_cls`` / ``loss_bbox``: None for both (the focal / smooth-L1 default), or a ``GHMC`` / ``GHMR``
    pair, each a module instance or mmdetection's ``dict(type='GHMC', ...)`` -> None or the two modules."""
    if loss_cls is None and loss_bbox is None:
        return None
    pair = []
    for cfg, kind, name in ((loss_cls, GHMC, "loss_cls"), (loss_bbox, GHMR, "loss_bbox")):
        if isinstance(cfg, dict) and cfg.get('type') == kind.__name__:
            cfg = kind(**{k: v for k, v in cfg.items() if k != 'type'})
        if not isinstance(cfg, kind):
            raise NotImplementedError("RetinaHead: %s must be a %s (a module or a dict with type=%r) when either loss is "
                                      "configured, got %r; loss_cls=None with loss_bbox=None is focal + smooth L1"
                                      % (name, kind.__name__, kind.__name__, cfg))
        pair.append(cfg)
    return pair


@HEADS.register_module
class RetinaHead(nn.Module):
    """``RetinaHead`` of mmdetection v1: two towers of ``stacked_convs`` 3x3 ``ConvModule``s (bias, ReLU), shared by all
    pyramid levels, and the two 3x3 predictors ``retina_cls`` (A * (num_classes - 1) channels, A = ``scales_per_octave``
    * len(anchor_ratios)) and ``retina_reg`` (4A channels).  The state-dict keys and shapes are mmdetection's
    (``cls_convs.0.conv.weight`` ... ``retina_reg.bias``); the predictors live in ``nn.Conv2d`` containers whose own
    forward is never called.  The whole head is one autograd node.  What the HIP path does not cover —
    ``norm_cfg`` / ``conv_cfg``, channel counts that are no multiples of 64 or above 512, more than 1024 predictor
    channels, more than 8 levels — is accepted by the constructor and raises ``NotImplementedError`` in ``forward``.
    ``loss_cls`` / ``loss_bbox``: both None for the focal + smooth-L1 ``loss``, or ``GHMC`` and ``GHMR`` (modules, or
    mmdetection's ``dict(type='GHMC', bins=30, momentum=0.75)`` / ``dict(type='GHMR', mu=0.02, bins=10, momentum=0.7)``)
    for the gradient-harmonised one; any other value raises ``NotImplementedError`` here."""

    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, octave_base_scale=4,
                 scales_per_octave=3, anchor_ratios=(0.5, 1.0, 2.0), anchor_strides=(8, 16, 32, 64, 128),
                 anchor_base_sizes=None, target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0), conv_cfg=None,
                 norm_cfg=None, loss_cls=None, loss_bbox=None):
        super().__init__()
        ghm = _ghm_pair(loss_cls, loss_bbox)
        if ghm is not None:               # no parameters, no state-dict keys: the running averages are non-persistent
            self.loss_cls, self.loss_bbox = ghm
        if num_classes < 2 or min(in_channels, feat_channels, scales_per_octave) < 1 or stacked_convs < 0 or \
                not len(anchor_ratios) or not len(anchor_strides):
            raise ValueError("RetinaHead: num_classes >= 2 (background included), positive sizes and non-empty anchor "
                             "lists are required")
        self.num_classes = int(num_classes)
        self.cls_out_channels = self.num_classes - 1
        self.in_channels = int(in_channels)
        self.feat_channels = int(feat_channels)
        self.stacked_convs = int(stacked_convs)
        self.octave_base_scale = octave_base_scale
        self.scales_per_octave = int(scales_per_octave)
        self.anchor_scales = [octave_base_scale * 2 ** (i / self.scales_per_octave)
                              for i in range(self.scales_per_octave)]
        self.anchor_ratios = list(anchor_ratios)
        self.anchor_strides = list(anchor_strides)
        self.anchor_base_sizes = list(anchor_strides) if anchor_base_sizes is None else list(anchor_base_sizes)
        if len(self.anchor_base_sizes) != len(self.anchor_strides):
            raise ValueError("RetinaHead: one anchor base size per stride")
        self.target_means = tuple(target_means)
        self.target_stds = tuple(target_stds)
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.anchor_generators = [AnchorGenerator(b, self.anchor_scales, self.anchor_ratios)
                                  for b in self.anchor_base_sizes]
        self.num_anchors = len(self.anchor_ratios) * len(self.anchor_scales)
        self.cls_convs, self.reg_convs = nn.ModuleList(), nn.ModuleList()
        for convs in (self.cls_convs, self.reg_convs):
            for i in range(self.stacked_convs):
                convs.append(ConvModule(self.in_channels if i == 0 else self.feat_channels, self.feat_channels, 3,
                                        padding=1, bias=True, activation='relu'))
        last = self.feat_channels if self.stacked_convs else self.in_channels
        self.retina_cls = nn.Conv2d(last, self.num_anchors * self.cls_out_channels, 3, padding=1)
        self.retina_reg = nn.Conv2d(last, self.num_anchors * 4, 3, padding=1)
        for m in (self.retina_cls, self.retina_reg):     # K-major, like the conv modules' weights (layers._channels_last_)
            m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
        self._routes = RETINA_ROUTES
        self.init_weights()

    def init_weights(self):
        for m in list(self.cls_convs) + list(self.reg_convs):
            nn.init.normal_(m.conv.weight, 0, 0.01)
            nn.init.constant_(m.conv.bias, 0)
        for m in (self.retina_cls, self.retina_reg):
            nn.init.normal_(m.weight, 0, 0.01)
            nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.retina_cls.bias, -math.log((1 - 0.01) / 0.01))

    def _pyr_unit(self, name, weight, dtype):
        cache = self.__dict__.setdefault('_hip_units', {})
        u = cache.get((name, dtype))
        if not isinstance(u, PyrUnit) or u.sources[0] is not weight:
            u = cache[(name, dtype)] = PyrUnit(weight, dtype)
        return u.refresh()

    def _padded_conv(self, name, conv, Cp):
        """The composed route's stand-in for a predictor: a conv of Cp output channels, not a submodule, whose weight and
        bias are overwritten with the zero-padded parameter on every call (two copies, graph nodes inside a capture)."""
        cache = self.__dict__.setdefault('_padded_convs', {})
        pc = cache.get(name)
        w = conv.weight
        if pc is None or pc.weight.device != w.device or pc.weight.shape[1] != w.shape[1] or pc.weight.shape[0] != Cp:
            pc = nn.Conv2d(w.shape[1], Cp, 3, padding=1).to(w.device)
            pc.weight.data = torch.zeros_like(pc.weight.data).contiguous(memory_format=torch.channels_last)
            pc.bias.data.zero_()
            pc.requires_grad_(False)
            cache[name] = pc
        with torch.no_grad():
            pc.weight[:w.shape[0]].copy_(w)
            pc.bias[:w.shape[0]].copy_(conv.bias)
        return pc

    def _chains(self, dtype):
        """[[the cls tower's layers ..., retina_cls], [the reg tower's layers ..., retina_reg]] with refreshed operands"""
        for m in list(self.cls_convs) + list(self.reg_convs):
            for u in m.__dict__.get('_hip_units', {}).values():
                if getattr(u, 'sink', None) is not None:
                    raise NotImplementedError("RetinaHead: a shared tower weight's per-level gradients cannot be written "
                                              "into a gradient bucket")
        chains = []
        for tower, tname, pred, pname, kind in ((self.cls_convs, 'cls_convs', self.retina_cls, 'retina_cls', 'cls'),
                                                (self.reg_convs, 'reg_convs', self.retina_reg, 'retina_reg', 'reg')):
            chain = [_Layer(self, '%s.%d' % (tname, i), m.conv, 'tower', True, dtype) for i, m in enumerate(tower)]
            chain.append(_Layer(self, pname, pred, kind, False, dtype))
            chains.append(chain)
        return chains

    def _check_supported(self):
        if self.norm_cfg is not None or self.conv_cfg is not None:
            raise NotImplementedError("RetinaHead: norm_cfg / conv_cfg other than None are not on the HIP path")
        for name, c in (("in_channels", self.in_channels), ("feat_channels", self.feat_channels)):
            if c % 64 or c > pyramid_ops.MAX_CIN:
                raise NotImplementedError("RetinaHead: %s=%d must be a multiple of 64, at most %d, on the HIP path"
                                          % (name, c, pyramid_ops.MAX_CIN))
        for name, c in (("A * cls_out_channels", self.num_anchors * self.cls_out_channels), ("4A", 4 * self.num_anchors)):
            if c > pyramid_ops.MAX_COUT:
                raise NotImplementedError("RetinaHead: %s = %d output channels are not on the HIP path (at most %d)"
                                          % (name, c, pyramid_ops.MAX_COUT))

    def forward(self, feats):
        """feats: a list of 1..8 (B, in_channels, H_l, W_l) maps (16-bit channels_last is read in place, float32 is
        converted as in the other heads) -> (cls_scores, bbox_preds): lists of (B, A*C, H_l, W_l) and (B, 4A, H_l, W_l)
        tensors in the compute dtype, channel order ``a*C + c`` and ``4a + j``, channels_last memory: what
        ``anchor_head_loss`` and ``anchor_head_detections`` take in place."""
        self._check_supported()
        feats = list(feats)
        if not 1 <= len(feats) <= pyramid_ops.MAX_LEVELS:
            raise NotImplementedError("RetinaHead: feats must be a list of 1..%d levels on the HIP path, got %d"
                                      % (pyramid_ops.MAX_LEVELS, len(feats)))
        if torch.is_tensor(feats[0]) and feats[0].dtype == torch.float32:
            dtype = pick_dtype(self, feats[0])
            feats = [f.to(dtype) for f in feats]
        n = len(feats)
        out = RetinaHeadFunction.apply(self, n, *feats, *self.parameters())
        return list(out[:n]), list(out[n:])

    def get_anchors(self, featmap_sizes, valid_sizes=None, device='cuda'):
        """(anchors, valid_flags): per-level lists from one ``anchor_pyramid`` launch over the head's own generators."""
        n = len(featmap_sizes)
        return anchor_pyramid(self.anchor_generators[:n], featmap_sizes, self.anchor_strides[:n], device, valid_sizes)

    def loss(self, cls_scores, bbox_preds, anchors, valid_flags, gt_bboxes, gt_labels, gt_counts, img_shapes, beta=1.0 / 9.0,
             **target_cfg):
        """``anchor_target_all`` (pos_iou_thr 0.5, neg_iou_thr 0.4, min_pos_iou 0, the head's means / stds), then the focal
        ``anchor_head_loss`` (gamma 2, alpha 0.25, smooth-L1 ``beta``) averaged over the positives: -> losses (2,) =
        [loss_cls, loss_bbox].  ``anchors`` / ``valid_flags``: what ``get_anchors`` returned or their concatenation.  A head
        built with ``loss_cls=GHMC`` / ``loss_bbox=GHMR`` calls ``ghm_head_loss`` (scope 'level') on the same targets
        instead and multiplies the two terms by the modules' ``loss_weight``; ``beta`` is then not used."""
        cat = lambda t: torch.cat(list(t)) if isinstance(t, (list, tuple)) else t
        cfg = dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, target_means=self.target_means,
                   target_stds=self.target_stds)
        cfg.update(target_cfg)
        labels, label_weights, bbox_targets, bbox_weights, num_pos, _, _ = anchor_target_all(
            cat(anchors), cat(valid_flags), gt_bboxes, gt_labels, gt_counts, img_shapes, **cfg)
        lc, lb = getattr(self, 'loss_cls', None), getattr(self, 'loss_bbox', None)
        if lc is not None:
            losses = ghm_head_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, lc.acc_sum,
                                   lb.acc_sum, self.cls_out_channels, bins_cls=lc.bins, bins_reg=lb.bins,
                                   momentum_cls=lc.momentum, momentum_reg=lb.momentum, mu=lb.mu)
            if lc.loss_weight == 1.0 and lb.loss_weight == 1.0:
                return losses
            return torch.stack((losses[0] * lc.loss_weight, losses[1] * lb.loss_weight))   # no host tensor: capturable
        return anchor_head_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights,
                                avg_factor=num_pos, num_classes=self.cls_out_channels, beta=beta, gamma=2.0, alpha=0.25)

    def get_bboxes(self, cls_scores, bbox_preds, anchors, img_shapes, scale_factors=None, **test_cfg):
        """``anchor_head_detections`` with the head's means / stds on the head's outputs, in place; defaults nms_pre 1000,
        score_thr 0.05, nms_thr 0.5, max_per_img 100.  ``nms=dict(type='soft_nms', ...)`` is forwarded as it is."""
        cfg = dict(nms_pre=1000, score_thr=0.05, nms_thr=0.5, max_per_img=100, target_means=self.target_means,
                   target_stds=self.target_stds)
        cfg.update(test_cfg)
        return anchor_head_detections(cls_scores, bbox_preds, anchors, img_shapes, scale_factors, **cfg)


# ---- the FCOS head ------------------------------------------------------------------------------------------------------
INF = 1e8
# Routes of the FCOS head's products, set by §4k's rule from profiles/pyramid_gn_bench.jsonl: a product
# is on the form whose slowest repeat is below the others' fastest, else composed.  'cls' (80 columns), 'reg' (4) and 'ctr'
# (1) are the predictors: the pyramid kernel measured below both other forms for every product but the 80-column weight
# gradient.  'gn' is the GroupNorm (+ ReLU) of a tower layer, forward and backward ('pyramid' or 'composed').  The tower
# convs are §4m's 256 -> 256 product without its epilogue and keep that section's routes (not timed again).
FCOS_ROUTES = {
    'tower': {'fwd': SPLIT, 'dgrad': SPLIT, 'wgrad': COMPOSED},
    'cls': {'fwd': PYRAMID, 'dgrad': PYRAMID, 'wgrad': COMPOSED},
    'reg': {'fwd': PYRAMID, 'dgrad': PYRAMID, 'wgrad': PYRAMID},
    'ctr': {'fwd': PYRAMID, 'dgrad': PYRAMID, 'wgrad': PYRAMID},
    'gn': {'fwd': PYRAMID, 'bwd': PYRAMID},
}
FCOS_COMPOSED = {k: {p: COMPOSED for p in v} for k, v in FCOS_ROUTES.items()}


class _RawLayer(_Layer):
    """A bias-free shared 3x3 conv whose raw product feeds a GroupNorm: ``_Layer`` without the bias and its gradient."""

    def fwd(self, xs):
        def composed(idx):
            return [HF.unit_fwd(self.unit, xs[l].permute(0, 2, 3, 1)).permute(0, 3, 1, 2) for l in idx]
        return self._routed(self.routes['fwd'], xs, lambda idx: pyramid_ops.pyramid_conv_fwd(
            self._pick(xs, idx), self.pyr.w_fwd, None, self.Cout, False), composed)

    def wgrad(self, xs, gs, queue):
        if self.routes['wgrad'] == PYRAMID:
            dw, _ = pyramid_ops.pyramid_conv_wgrad(xs, gs, self.weight.permute(0, 2, 3, 1).is_contiguous())
            return lambda: (dw,)
        if self.routes['wgrad'] != COMPOSED:
            raise ValueError("FCOSHead: the weight gradient has the routes 'pyramid' and 'composed', got %r"
                             % (self.routes['wgrad'],))
        per_level = [HF.unit_wgrad(self.unit, x.permute(0, 2, 3, 1), g.permute(0, 2, 3, 1), queue=queue)[0]
                     for x, g in zip(xs, gs)]

        def total():
            dw = per_level[0]
            for gw in per_level[1:]:                                  # level order, finest first
                dw = dw + gw
            return (dw,)
        return total


class _GnLayer(object):
    """The GroupNorm + ReLU of one tower layer during one forward / backward: shared (gamma, beta) over the pyramid."""

    def __init__(self, head, norm, frozen):
        self.norm, self.frozen = norm, frozen
        self.routes = head._routes['gn']
        for p in ('fwd', 'bwd'):
            if self.routes[p] not in (PYRAMID, COMPOSED):
                raise ValueError("FCOSHead: the GroupNorm has the routes 'pyramid' and 'composed', got %r"
                                 % (self.routes[p],))
        if self.routes['fwd'] != self.routes['bwd']:
            raise ValueError("FCOSHead: the GroupNorm's backward reads its forward's statistics table: one route for both")

    def fwd(self, zs):
        """-> (ys, [statistics tensors])"""
        nm = self.norm
        if self.routes['fwd'] == PYRAMID:
            ys, stats = pyramid_ops.pyramid_gn_fwd(zs, nm.weight.detach(), nm.bias.detach(), nm.num_groups, nm.eps, True)
            return ys, [stats]
        ys, stats = [], []
        for z in zs:
            y, st = ops.gn_fwd(z.permute(0, 2, 3, 1), nm.weight.detach(), nm.bias.detach(), nm.num_groups, nm.eps, None,
                               True)
            ys.append(y.permute(0, 3, 1, 2))
            stats.append(st)
        return ys, stats

    def bwd(self, gs, ys, zs, stats):
        """-> (dzs, dgamma, dbeta) from the unmasked cotangents"""
        nm = self.norm
        if self.routes['bwd'] == PYRAMID:
            return pyramid_ops.pyramid_gn_bwd(gs, ys, zs, stats[0], nm.weight.detach(), nm.num_groups, True)
        dzs, dg, db = [], None, None
        for g, y, z, st in zip(gs, ys, zs, stats):                    # level order, finest first
            gm = ops.act_mask(g.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1))
            dz, dg, db = ops.gn_bwd(gm, z.permute(0, 2, 3, 1), st, nm.weight.detach(), nm.num_groups, dg, db,
                                    dg is not None)
            dzs.append(dz.permute(0, 3, 1, 2))
        return dzs, dg, db


class FCOSHeadFunction(torch.autograd.Function):
    """``apply(head, n, feat_0 .. feat_{n-1}, *parameters)`` -> (cls_0 .. cls_{n-1}, reg_0 .., ctr_0 ..); the parameters
    in the order of ``head._chains``: per tower layer the conv weight (and bias without GroupNorm, or gamma, beta with
    it), cls tower first, then ``fcos_cls``, ``fcos_reg``, ``fcos_centerness`` (weight, bias each).

    Forward: per tower layer the raw conv product over the pyramid and the GroupNorm + ReLU product (three launches over
    the pyramid); then the three predictors, centre-ness off the cls tower.  Saved per GroupNorm layer and level: the raw
    map z and the output y.  Backward per chain: the predictor's weight gradient, its UNMASKED input gradient (the cls
    tower receives ``fcos_cls``'s as the addend of ``fcos_centerness``'s), then per layer ``pyramid_gn_bwd`` — which
    masks by y and gives dz, dgamma, dbeta —, the conv's weight gradient from the map below and dz, and its input
    gradient; the two first layers' input gradients meet in ``dfeats[l]`` through the addend, as in ``RetinaHead``."""

    @staticmethod
    def forward(ctx, head, n, *args):
        feats = args[:n]
        dtype = HF.pick_dtype(head, feats)
        towers, preds = head._chains(dtype)
        xs = [ops.to_nhwc_bf16(f, dtype).permute(0, 3, 1, 2) for f in feats]
        saved, counts, tops = list(xs), [], []
        for tower in towers:
            cur, cnt = xs, []
            for conv, gn in tower:
                if gn is None:
                    cur = conv.fwd(cur)
                    saved += cur
                    cnt.append(0)
                else:
                    zs = conv.fwd(cur)
                    cur, stats = gn.fwd(zs)
                    saved += zs + cur + stats
                    cnt.append(len(stats))
            counts.append(cnt)
            tops.append(cur)
        outs = [preds[0].fwd(tops[0]), preds[1].fwd(tops[1]), preds[2].fwd(tops[0])]
        ctx.save_for_backward(*saved)
        ctx.meta = (towers, preds, counts, n, [(f.dtype, f.is_contiguous() and not f.permute(0, 2, 3, 1).is_contiguous())
                                               for f in feats])
        return tuple(outs[0]) + tuple(outs[1]) + tuple(outs[2])

    @staticmethod
    def backward(ctx, *gs):
        towers, preds, counts, n, layouts = ctx.meta
        saved = list(ctx.saved_tensors)
        xs, saved = saved[:n], saved[n:]
        acts = []                      # per tower, per layer: (zs or None, ys, stats or None)
        for tower, cnt in zip(towers, counts):
            rows = []
            for (conv, gn), k in zip(tower, cnt):
                if gn is None:
                    rows.append((None, saved[:n], None))
                    saved = saved[n:]
                else:
                    rows.append((saved[:n], saved[n:2 * n], saved[2 * n:2 * n + k]))
                    saved = saved[2 * n + k:]
            acts.append(rows)
        dtype, dev, B = xs[0].dtype, xs[0].device, xs[0].shape[0]
        sizes = [tuple(x.shape[2:]) for x in xs]
        need_dx = any(ctx.needs_input_grad[2:2 + n])
        wq = HF.WgradQueue(dev)

        def cot(g, ch, name):
            g = [torch.zeros((B, H, W, ch), dtype=dtype, device=dev).permute(0, 3, 1, 2) if t is None else t
                 for t, (H, W) in zip(g, sizes)]
            return dense_ops.cotangents(g, name, dtype, B, ch, sizes)

        g_cls, g_reg, g_ctr = (cot(gs[i * n:(i + 1) * n], preds[i].Cout, nm)
                               for i, nm in enumerate(("g_cls", "g_reg", "g_ctr")))
        tower_thunks, pred_thunks, first_dx = [], [None] * 3, None
        for ti, (tower, rows) in enumerate(zip(towers, acts)):
            top = rows[-1][1] if rows else xs
            # the map a predictor reads is masked by the GroupNorm's backward when there is one, else here
            mask = top if rows and tower[-1][1] is None else None
            below = bool(rows) or need_dx
            if ti == 0:
                pred_thunks[0] = preds[0].wgrad(top, g_cls, wq)
                pred_thunks[2] = preds[2].wgrad(top, g_ctr, wq)
                g = None
                if below:
                    last = not rows
                    g = preds[0].dgrad(g_cls, mask_src=mask, addend=first_dx if last else None)
                    g = preds[2].dgrad(g_ctr, mask_src=mask, addend=g)
            else:
                pred_thunks[1] = preds[1].wgrad(top, g_reg, wq)
                g = preds[1].dgrad(g_reg, mask_src=mask, addend=first_dx if not rows else None) if below else None
            mine = []
            for i in reversed(range(len(tower))):
                conv, gn = tower[i]
                zs, ys, stats = rows[i]
                x_in = rows[i - 1][1] if i else xs
                if gn is not None:
                    g, dgam, dbet = gn.bwd(g, ys, zs, stats)
                    aff = (None, None) if gn.frozen else (dgam, dbet)
                else:
                    aff = ()
                t = conv.wgrad(x_in, g, wq)
                mine.append((t, aff))
                if i:
                    g = conv.dgrad(g, mask_src=x_in if tower[i - 1][1] is None else None)
                elif need_dx:
                    g = conv.dgrad(g, addend=first_dx)
            if need_dx:
                first_dx = g
            tower_thunks.append(mine[::-1])
        wq.flush()
        dxs = []
        for l in range(n):
            dx = None
            if ctx.needs_input_grad[2 + l]:
                dx = first_dx[l]
                in_dtype, nchw = layouts[l]
                if dx.dtype != in_dtype:
                    dx = dx.to(in_dtype)
                if nchw:                                                  # the input's own layout
                    dx = dx.contiguous()
            dxs.append(dx)
        HF.join_side_stream(dev)
        grads = []
        for mine in tower_thunks:
            for t, aff in mine:
                grads += list(t()) + list(aff)
        for t in pred_thunks:
            grads += list(t())
        return (None, None) + tuple(dxs) + tuple(grads)


@HEADS.register_module
class FCOSHead(nn.Module):
    """``FCOSHead`` of mmdetection v1: two towers of ``stacked_convs`` 3x3 ``ConvModule``s shared by all pyramid levels —
    bias-free conv, GroupNorm(``norm_cfg['num_groups']``), ReLU with the default ``norm_cfg``; conv with bias, ReLU with
    ``norm_cfg=None`` —, the 3x3 predictors ``fcos_cls`` (num_classes - 1 channels), ``fcos_reg`` (4) and
    ``fcos_centerness`` (1, off the cls tower) and one ``Scale`` per stride.  The state-dict keys are those of the modules
    (``cls_convs.0.conv.weight``, ``cls_convs.0.norm.weight`` ... ``scales.4.scale``); mmdetection's ``.gn.`` spelling of
    the norm keys is accepted on loading.  The predictors live in ``nn.Conv2d`` containers whose own forward is never
    called.  ``forward`` returns the RAW ``fcos_reg`` outputs: ``fcos_loss`` and ``fcos_detections`` take the ``Scale``
    parameters (``scale_vector()``) and apply ``exp(scale * x)`` themselves.  The whole head is one autograd node
    (DESIGN.md §4o).  What the HIP path does not cover is accepted by the constructor and raises ``NotImplementedError``
    in ``forward``."""

    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, strides=(8, 16, 32, 64, 128),
                 regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)), conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)):
        super().__init__()
        if num_classes < 2 or min(in_channels, feat_channels) < 1 or stacked_convs < 0 or not len(strides):
            raise ValueError("FCOSHead: num_classes >= 2 (background included), positive sizes and a non-empty stride "
                             "list are required")
        if len(regress_ranges) != len(strides):
            raise ValueError("FCOSHead: one regress range per stride")
        self.num_classes = int(num_classes)
        self.cls_out_channels = self.num_classes - 1
        self.in_channels = int(in_channels)
        self.feat_channels = int(feat_channels)
        self.stacked_convs = int(stacked_convs)
        self.strides = list(strides)
        self.regress_ranges = [tuple(r) for r in regress_ranges]
        self.conv_cfg = conv_cfg
        self.norm_cfg = None if norm_cfg is None else dict(norm_cfg)
        gn = self.norm_cfg is not None and self.norm_cfg.get('type') == 'GN'
        self.cls_convs, self.reg_convs = nn.ModuleList(), nn.ModuleList()
        for convs in (self.cls_convs, self.reg_convs):
            for i in range(self.stacked_convs):
                m = ConvModule(self.in_channels if i == 0 else self.feat_channels, self.feat_channels, 3, padding=1,
                               bias=not gn, normalize=True if gn else None, use_gn=gn, activation='relu')
                if gn:
                    m.norm = nn.GroupNorm(int(self.norm_cfg.get('num_groups', 32)), self.feat_channels)
                    if not self.norm_cfg.get('requires_grad', True):
                        m.norm.requires_grad_(False)
                convs.append(m)
        last = self.feat_channels if self.stacked_convs else self.in_channels
        self.fcos_cls = nn.Conv2d(last, self.cls_out_channels, 3, padding=1)
        self.fcos_reg = nn.Conv2d(last, 4, 3, padding=1)
        self.fcos_centerness = nn.Conv2d(last, 1, 3, padding=1)
        for m in (self.fcos_cls, self.fcos_reg, self.fcos_centerness):   # K-major, like the conv modules' weights
            m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.strides])
        self._routes = FCOS_ROUTES
        self.init_weights()

    def init_weights(self):
        for m in list(self.cls_convs) + list(self.reg_convs):
            nn.init.normal_(m.conv.weight, 0, 0.01)
            if m.conv.bias is not None:
                nn.init.constant_(m.conv.bias, 0)
        for m in (self.fcos_cls, self.fcos_reg, self.fcos_centerness):
            nn.init.normal_(m.weight, 0, 0.01)
            nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.fcos_cls.bias, -math.log((1 - 0.01) / 0.01))    # bias_init_with_prob(0.01)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # mmdetection names a ConvModule's norm layer after its type: cls_convs.0.gn.weight
        for k in [k for k in state_dict if k.startswith(prefix)]:
            parts = k[len(prefix):].split('.')
            if len(parts) == 4 and parts[0] in ('cls_convs', 'reg_convs') and parts[2] == 'gn':
                parts[2] = 'norm'
                state_dict[prefix + '.'.join(parts)] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    _pyr_unit = RetinaHead._pyr_unit
    _padded_conv = RetinaHead._padded_conv

    def _chains(self, dtype):
        """([cls tower, reg tower], [fcos_cls, fcos_reg, fcos_centerness]) with refreshed operands; a tower is a list of
        (conv layer, GroupNorm layer or None)."""
        for u in self.__dict__.get('_hip_units', {}).values():
            if getattr(u, 'sink', None) is not None:
                raise NotImplementedError("FCOSHead: a shared weight's per-level gradients cannot be written into a "
                                          "gradient bucket")
        frozen = self.norm_cfg is not None and not self.norm_cfg.get('requires_grad', True)
        towers = []
        for convs, tname in ((self.cls_convs, 'cls_convs'), (self.reg_convs, 'reg_convs')):
            tower = []
            for i, m in enumerate(convs):
                name = '%s.%d' % (tname, i)
                if m.with_norm:
                    layer = (_RawLayer(self, name, m.conv, 'tower', False, dtype), _GnLayer(self, m.norm, frozen))
                else:
                    layer = (_Layer(self, name, m.conv, 'tower', True, dtype), None)
                tower.append(layer)
            towers.append(tower)
        preds = [_Layer(self, name, conv, kind, False, dtype) for name, conv, kind in (
            ('fcos_cls', self.fcos_cls, 'cls'), ('fcos_reg', self.fcos_reg, 'reg'),
            ('fcos_centerness', self.fcos_centerness, 'ctr'))]
        return towers, preds

    def _params(self):
        """The parameters in the order ``FCOSHeadFunction`` returns their gradients"""
        out = []
        for convs in (self.cls_convs, self.reg_convs):
            for m in convs:
                out.append(m.conv.weight)
                if m.conv.bias is not None:
                    out.append(m.conv.bias)
                if m.with_norm:
                    out += [m.norm.weight, m.norm.bias]
        for m in (self.fcos_cls, self.fcos_reg, self.fcos_centerness):
            out += [m.weight, m.bias]
        return out

    def _check_supported(self):
        if self.conv_cfg is not None:
            raise NotImplementedError("FCOSHead: conv_cfg other than None is not on the HIP path")
        if self.norm_cfg is not None and self.norm_cfg.get('type') != 'GN':
            raise NotImplementedError("FCOSHead: norm type %r is not on the HIP path (GN or no norm_cfg)"
                                      % (self.norm_cfg.get('type'),))
        for name, c in (("in_channels", self.in_channels), ("feat_channels", self.feat_channels)):
            if c % 64 or c > pyramid_ops.MAX_CIN:
                raise NotImplementedError("FCOSHead: %s=%d must be a multiple of 64, at most %d, on the HIP path"
                                          % (name, c, pyramid_ops.MAX_CIN))
        if self.cls_out_channels > pyramid_ops.MAX_COUT:
            raise NotImplementedError("FCOSHead: %d class channels are not on the HIP path (at most %d)"
                                      % (self.cls_out_channels, pyramid_ops.MAX_COUT))
        if self.norm_cfg is not None and self.stacked_convs:
            C, G = self.feat_channels, int(self.norm_cfg.get('num_groups', 32))
            if C not in pyramid_ops.GN_CHANNELS or C % G or C // G > pyramid_ops.GN_MAX_CPG:
                raise NotImplementedError("FCOSHead: GroupNorm(%d groups, feat_channels=%d) is not on the HIP path "
                                          "(feat_channels one of %s, at most %d channels per group)"
                                          % (G, C, ", ".join(map(str, pyramid_ops.GN_CHANNELS)), pyramid_ops.GN_MAX_CPG))

    def forward(self, feats):
        """feats: a list of 1..8 (B, in_channels, H_l, W_l) maps (16-bit channels_last is read in place, float32 is
        converted as in the other heads) -> (cls_scores, bbox_preds, centernesses): lists of (B, num_classes - 1, H_l,
        W_l), (B, 4, H_l, W_l) and (B, 1, H_l, W_l) tensors in the compute dtype, channels_last memory: what ``fcos_loss``
        and ``fcos_detections`` take in place.  ``bbox_preds`` are the raw ``fcos_reg`` outputs."""
        self._check_supported()
        feats = list(feats)
        if not 1 <= len(feats) <= pyramid_ops.MAX_LEVELS:
            raise NotImplementedError("FCOSHead: feats must be a list of 1..%d levels on the HIP path, got %d"
                                      % (pyramid_ops.MAX_LEVELS, len(feats)))
        if torch.is_tensor(feats[0]) and feats[0].dtype == torch.float32:
            dtype = pick_dtype(self, feats[0])
            feats = [f.to(dtype) for f in feats]
        n = len(feats)
        out = FCOSHeadFunction.apply(self, n, *feats, *self._params())
        return list(out[:n]), list(out[n:2 * n]), list(out[2 * n:])

    def scale_vector(self):
        """The ``Scale`` parameters as one (L,) float32 tensor (differentiable): ``fcos_loss`` / ``fcos_detections``'
        ``scales``."""
        return torch.stack([s.scale for s in self.scales])

    def get_points(self, featmap_sizes, device=None):
        return fcos_points(featmap_sizes, self.strides[:len(featmap_sizes)], device)

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, gt_counts, center_sample_radius=None,
             **cfg):
        """``fcos_target`` with the head's strides and regress ranges, then ``fcos_loss`` with the head's ``Scale``s:
        -> what ``fcos_loss`` returns.  ``cfg``: ``fcos_loss``'s loss_type / gamma / alpha / eps."""
        n = len(cls_scores)
        sizes = [tuple(t.shape[2:]) for t in cls_scores]
        labels, bbox_targets, _, _ = fcos_target(sizes, self.strides[:n], self.regress_ranges[:n], gt_bboxes, gt_labels,
                                                 gt_counts, center_sample_radius)
        return fcos_loss(cls_scores, bbox_preds, centernesses, labels, bbox_targets, self.scale_vector()[:n], **cfg)

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_shapes, scale_factors=None, **test_cfg):
        """``fcos_detections`` with the head's strides and ``Scale``s on the head's outputs, in place; defaults nms_pre
        1000, score_thr 0.05, nms_thr 0.5, max_per_img 100.  ``nms=dict(type='soft_nms', ...)`` is forwarded as it is."""
        n = len(cls_scores)
        cfg = dict(nms_pre=1000, score_thr=0.05, nms_thr=0.5, max_per_img=100)
        cfg.update(test_cfg)
        return fcos_detections(cls_scores, bbox_preds, centernesses, self.strides[:n], img_shapes,
                               self.scale_vector().detach()[:n], scale_factors, **cfg)
