"""The box head's learnable part: ``BBoxHead`` — mmdetection v1's ``SharedFCBBoxHead`` with
``num_shared_fcs`` fully connected layers and the two predictors ``fc_cls`` / ``fc_reg`` — between ``roi_align`` and
``bbox_head_loss`` / ``bbox_head_detections``.  Every product runs through csrc/linear.hip; the whole head is one autograd
node."""
import torch
import torch.nn as nn

from . import linear_ops
from .functional import pick_dtype
from .linear import LinearUnit, check_params, flatten_input
from .registry import HEADS

__all__ = ["BBoxHead", "BBoxHeadFunction"]


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
