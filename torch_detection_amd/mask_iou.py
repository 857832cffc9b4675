"""Mask Scoring R-CNN (Huang et al., CVPR 2019; ``ms_rcnn/`` of mmdetection v1) around the ``MaskIoUHead``'s layers (HIP
kernels of csrc/mask_iou.hip; DESIGN.md §4s has the exact arithmetic, tests/ms_rcnn_ref.py restates it): the regression
target of the head rasterised from the ground-truth polygons, the MSE loss on the positive targets with its gradient,
and at test time the product of the predicted mask IoU with the detection score.

Nothing here synchronises with the host or allocates inside the library, so a training or test step that uses these
stays capturable in a graph.  The semantics follow mmdetection v1 (``MaskIoUHead.get_target``, ``MSELoss`` over
``mask_iou_targets > 0``, ``get_mask_scores``); the arithmetic is the project's own.
"""
import weakref

import torch

from . import functional as _F
from . import mask_iou_ops as _m
from . import ops
from ._args import on_device, tensor

__all__ = ["MaskIoUStemFunction", "MaskIoUStemUnit", "MaskIoULossFunction", "mask_iou_stem", "mask_iou_target",
           "mask_iou_loss", "mask_scores"]

_16 = (torch.bfloat16, torch.float16)
_NO_CPU = ('torch_detection_amd modules run on the MI355X HIP path only: move the module to a CUDA/HIP device (no CPU '
           'fallback)')


class MaskIoUStemUnit(object):
    """Packed 16-bit operands of the feature part ``weight[:, :Cf]`` of one (Cout, Cf + 1, 3, 3) weight for one compute
    dtype: ``w_fwd`` (Cout, 3, 3, Cf) and ``w_dgrad`` (Cf, 3, 3, Cout), the conv path's operands.  The slice is packed in
    place through its strides; the mask channel ``weight[:, Cf]`` is read as float32 by the kernels of csrc/mask_iou.hip.
    Cached and re-packed in capture as ``deform.DeformUnit`` is."""

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
            self.w_fwd, self.w_dgrad = ops.pack_conv_weight(w.detach()[:, :w.shape[1] - 1], None, True, self.dtype,
                                                            out=(self.w_fwd, self.w_dgrad) if reuse else None)
        self.key = key
        return self


_units = {}   # id(weight) -> (weak reference to the weight, {dtype: MaskIoUStemUnit})


def _unit_for(weight, dtype):
    k = id(weight)
    ent = _units.get(k)
    if ent is None or ent[0]() is not weight:
        ent = (weakref.ref(weight, lambda _, k=k: _units.pop(k, None)), {})
        _units[k] = ent
    u = ent[1].get(dtype)
    if u is None:
        u = ent[1][dtype] = MaskIoUStemUnit(weight, dtype)
    return u


def forget(weight):
    """``invalidate_packed``'s hook: drop the version key of every packed copy of ``weight``."""
    ent = _units.get(id(weight))
    if ent is not None and ent[0]() is weight:
        for u in ent[1].values():
            u.key = None


def check_stem_args(mask_feats, mask_pred, labels, weight, bias, label_offset=0):
    """Every refusal of ``mask_iou_stem`` as a ValueError, before any launch: shapes, dtypes, layouts and limits first
    (no device needed), the device last."""
    if not isinstance(mask_feats, torch.Tensor) or mask_feats.dim() != 4:
        tensor(mask_feats, "mask_feats", _16, ("R", "Cf", "S", "S"), contiguous=False)
    R, Cf, S, S2 = tensor(mask_feats, "mask_feats", _16, ("R", "Cf", "S", "S"), contiguous=False)
    if S != S2 or not mask_feats.permute(0, 2, 3, 1).is_contiguous():
        raise ValueError("mask_feats must be a (R, Cf, S, S) channels_last tensor, got shape %s strides %s"
                         % (tuple(mask_feats.shape), tuple(mask_feats.stride())))
    Cout = tensor(weight, "weight", torch.float32, ("Cout", Cf + 1, 3, 3))[0]
    tensor(bias, "bias", torch.float32, (Cout,))
    _m._pred4(mask_pred, R)
    pred, _, C, S_pred, _, _, _, _ = _m._stem_setup(mask_pred, labels, weight, label_offset)
    if S_pred != S:
        raise ValueError("mask_pred must be (R, C, 2S, 2S) = (%d, C, %d, %d) for these mask_feats, got %s"
                         % (R, 2 * S, 2 * S, tuple(mask_pred.shape)))
    on_device([("mask_feats", mask_feats), ("mask_pred", mask_pred), ("labels", labels), ("weight", weight),
               ("bias", bias)])


class MaskIoUStemFunction(torch.autograd.Function):
    """``apply(mask_feats, mask_pred, labels, weight, bias, label_offset, relu, unit)``: the MaskIoUHead's first layer as
    one node.  Forward: the mask channel's addend (one launch of csrc/mask_iou.hip), then the conv launch over the
    features with bias, addend and ReLU in its epilogue.  Backward: ``act_mask``, the conv path's input and weight
    gradients, and two launches for ``dmask_pred`` and the mask channel's weight gradient.  Saves the features, the
    logits, P with its window indices, and the output when ``relu``."""

    @staticmethod
    def forward(ctx, mask_feats, mask_pred, labels, weight, bias, label_offset, relu, unit):
        check_stem_args(mask_feats, mask_pred, labels, weight, bias, label_offset)
        unit = (unit if unit is not None else _unit_for(weight, mask_feats.dtype)).refresh()
        x = mask_feats.permute(0, 2, 3, 1)
        w = weight.detach()
        a, P, idx = _m.mask_iou_stem_fwd(mask_pred, labels, w, label_offset, mask_feats.dtype)
        y = ops.conv2d_fwd(x, unit.w_fwd, 3, 1, 1, None, bias.detach(), addend=a, addend_mode=ops.ADD_SAME, relu=relu)
        ctx.save_for_backward(x, mask_pred, labels, weight, P, idx, y if relu else None)
        ctx.meta = (unit, label_offset, relu)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        x, mask_pred, labels, weight, P, idx, y = ctx.saved_tensors
        unit, label_offset, relu = ctx.meta
        gz = ops.to_nhwc_bf16(gy, x.dtype)
        if relu:
            gz = ops.act_mask(gz, y)
        S, Cf = x.shape[1], x.shape[3]
        need = ctx.needs_input_grad
        dfeats = dpred = dweight = dbias = None
        if need[0]:
            dfeats = ops.conv2d_dgrad(gz, unit.w_dgrad, (S, S), 3, 1, 1).permute(0, 3, 1, 2)
        if need[1] or need[3]:
            dpred, dw1, _ = _m.mask_iou_stem_bwd(gz, P, idx, mask_pred, labels, weight.detach(), label_offset)
        if need[3] or need[4]:
            dw, _, dbias = ops.conv2d_wgrad(x, gz, unit.w_fwd, 3, 1, 1)
            if need[3]:
                dweight = torch.cat([dw.permute(0, 3, 1, 2), dw1.view(-1, 1, 3, 3)], 1)
        return dfeats, dpred if need[1] else None, None, dweight, dbias if need[4] else None, None, None, None


def mask_iou_stem(mask_feats, mask_pred, labels, weight, bias, label_offset=0, relu=True):
    """The MaskIoUHead's first layer: ``relu?(conv3x3(cat(mask_feats, max_pool2x2(sigmoid(mask_pred[r, ch_r]))), weight)
    + bias)`` without forming the 257-channel input: by linearity the mask channel's share is the conv launch's epilogue
    addend.  ``mask_feats``: (R, Cf, S, S) bf16 / fp16, channels_last, Cf a multiple of 64; ``mask_pred``: (R, C, 2S, 2S)
    logits, float32 / bfloat16 / float16, NCHW-contiguous or channels_last ((R, 2S, 2S) is C = 1), read in place;
    ``labels`` (R,) int64: row r reads channel ``labels[r] + label_offset`` (offset 0 with the training labels, 1 with
    ``bbox_head_detections``' 0-based labels; channel 0 when C == 1) — a row whose channel is outside 1..C-1 contributes
    P = 0, its logits are never read and it gets no gradient; ``weight`` (Cout, Cf + 1, 3, 3) and ``bias`` (Cout,) float32,
    Cout a multiple of 64 up to 512.  The pooled value is the FIRST maximum of its window in row-major order, and the
    gradient of ``mask_pred`` lands on that element alone.  Returns (R, Cout, S, S) in ``mask_feats``' dtype,
    channels_last.  Differentiable in ``mask_feats``, ``mask_pred``, ``weight`` and ``bias``."""
    check_stem_args(mask_feats, mask_pred, labels, weight, bias, label_offset)
    return MaskIoUStemFunction.apply(mask_feats, mask_pred, labels, weight, bias, int(label_offset), bool(relu), None)


def mask_iou_target(rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_pred, labels, mask_targets,
                    img_shapes, thr=0.5):
    """The IoU of each row's predicted mask with its WHOLE ground-truth instance: the MaskIoUHead's regression target,
    in one launch and without a host synchronisation.

    ``rois`` (R, 5), ``pos_assigned_gt_inds`` (R,) int32 and the polygon tensors are :func:`mask_target`'s, and a row is
    valid by its rule; ``mask_targets`` (R, M, M) uint8 is its output.  ``mask_pred``: (R, C, M, M) logits (float32 /
    bfloat16 / float16, NCHW-contiguous or channels_last; (R, M, M) is C = 1) of which row r reads channel
    ``labels[r]`` (1..C-1; channel 0 when C == 1).  ``img_shapes``: (B, 2) int32 (h, w), the canvas of each image,
    1..8192 a side.

    The instance's bitmap on the canvas has pixel (x, y) set iff ``(x + 0.5, y + 0.5)`` lies inside any of its polygons
    (the edge rule of :func:`mask_target`); ``full`` is its pixel count and ``in`` the count inside the truncated box
    ``[x1, x2] x [y1, y2]`` clipped to the canvas.  With ``pa = #{logit > thr}``, ``ts = #{target == 1}`` and ``ov`` the
    count of both::

        ratio = in / (full + 1e-7);  gf = ts / (ratio + 1e-7);  iou = ov / (pa + gf - ov)

    in float32 (0 where the denominator is not positive: mmdetection's NaN there is dropped by its ``target > 0``).
    Like mmdetection v1 the LOGIT is compared with ``thr``; pass ``thr=0`` for probability 0.5.  An invalid row or a
    label without a channel gives 0 and neither its logits nor its polygons are read.  Returns (R,) float32."""
    return _m.mask_iou_target(rois, pos_assigned_gt_inds, poly_xy, poly_offsets, gt_poly_offsets, mask_pred, labels,
                              mask_targets, img_shapes, thr)


class MaskIoULossFunction(torch.autograd.Function):
    """``apply(loss_weight, labels, mask_iou_targets, mask_iou_pred)``."""

    @staticmethod
    def forward(ctx, loss_weight, labels, mask_iou_targets, mask_iou_pred):
        loss, avg = _m.mask_iou_loss_fwd(mask_iou_pred, labels, mask_iou_targets, loss_weight)
        ctx.save_for_backward(labels, mask_iou_targets, mask_iou_pred)
        ctx.loss_weight, ctx.avg = loss_weight, avg
        return loss

    @staticmethod
    def backward(ctx, g):
        labels, mask_iou_targets, mask_iou_pred = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        return None, None, None, _m.mask_iou_loss_bwd(mask_iou_pred, labels, mask_iou_targets, ctx.loss_weight, g,
                                                      ctx.avg)


def mask_iou_loss(mask_iou_pred, labels, mask_iou_targets, loss_weight=0.5):
    """mmdetection's ``MSELoss`` of the MaskIoUHead over the rows with a positive target.  ``mask_iou_pred``: (R, C)
    float32 / bfloat16 / float16; row r is live iff ``mask_iou_targets[r] > 0`` and ``labels[r]`` is in 1..C-1;
    ``loss = loss_weight * sum_live (pred[r, labels[r]] - target_r)^2 / max(#live, 1)``, the rows counted on the device.
    Rows that are not live are never read.  Returns a (1,) float32 loss; its backward gives ``mask_iou_pred`` a gradient
    of its own shape and dtype, exact zeros off the live rows' columns."""
    return MaskIoULossFunction.apply(loss_weight, labels, mask_iou_targets, mask_iou_pred)


def mask_scores(mask_iou_pred, dets, labels, counts):
    """mmdetection's ``get_mask_scores`` for a whole batch, one launch: ``mask_iou_pred`` (B*max_num, C) in the row order
    of :func:`rois_from_detections`, ``dets`` (B, max_num, 5), ``labels`` (B, max_num) int64 0-based foreground labels and
    ``counts`` (B,) int32 as ``multiclass_nms`` returns them -> (B, max_num) float32
    ``mask_iou_pred[b max_num + d, labels[b, d] + 1] * dets[b, d, 4]`` for ``d < counts[b]`` and a label with a column,
    0 elsewhere (every row under the overflow marker ``counts[b] = -1``)."""
    return _m.mask_scores(mask_iou_pred, dets, labels, counts)
