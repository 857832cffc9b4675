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
(csrc/dense_head.hip) — between ``FPN`` and ``rpn_loss`` / ``rpn_proposals``.  The whole head is one autograd node."""
import torch
import torch.nn as nn

from . import dense_ops, deconv_ops, linear_ops, ops
from . import functional as HF
from .box import AnchorGenerator, anchor_pyramid, rpn_proposals
from .deconv import DeconvUnit
from .deconv import check_params as check_deconv_params
from .functional import pick_dtype
from .layers import ConvModule
from .linear import LinearUnit, check_params, flatten_input
from .losses import rpn_loss
from .registry import HEADS
from .target import anchor_target

__all__ = ["BBoxHead", "BBoxHeadFunction", "FCNMaskHead", "MaskTailFunction", "RPNHead", "RPNHeadFunction", "PredUnit"]


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
