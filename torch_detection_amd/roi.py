"""Multi-level RoIAlign — the FPN RoI extractor between the neck and the box / mask heads.

mmdetection-v1 semantics (``SingleRoIExtractor`` + ``RoIAlign(out_size, sample_num)``, ``aligned=False``, '+1' ends),
computed by the gfx950 kernels of ``csrc/roi_align.hip``: one launch forward for every level and image, two backward,
with a fixed summation order (bitwise reproducible, eager or graph-replayed).  Features are the 16-bit NHWC tensors
``FPN`` returns (read in place); the level gradients go back in that layout, so ``FPN``'s backward takes them with no
copy."""
import torch

from . import ops

__all__ = ["RoIAlignFunction", "map_roi_levels", "roi_align", "SingleRoIExtractor", "rois_from_proposals"]


class RoIAlignFunction(torch.autograd.Function):
    """One autograd node for all levels: ``apply(rois, out_size, featmap_strides, sampling_ratio, finest_scale,
    *feats)``.  Saves the rois and the level shapes, not the features; ``rois`` get no gradient."""

    @staticmethod
    def forward(ctx, rois, out_size, featmap_strides, sampling_ratio, finest_scale, *feats):
        scales = [1.0 / float(s) for s in featmap_strides]
        out = ops.roi_align_fwd(list(feats), rois, out_size, scales, sampling_ratio, finest_scale)
        B, C, dtype, shapes = ops.roi_level_shapes(feats)
        ctx.save_for_backward(rois)
        ctx.meta = (shapes, B, C, dtype, int(out_size), scales, int(sampling_ratio), float(finest_scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        (rois,) = ctx.saved_tensors
        shapes, B, C, dtype, S, scales, sr, fs = ctx.meta
        grads = ops.roi_align_bwd(dout, rois, shapes, B, C, dtype, S, scales, sr, fs)
        return (None,) * 5 + tuple(g.permute(0, 3, 1, 2) for g in grads)


def map_roi_levels(rois, num_levels, finest_scale=56):
    """(R,) int64 level of every RoI: ``floor(log2(sqrt(w*h) / finest_scale + 1e-6))`` ('+1' widths) clamped to
    ``[0, num_levels-1]``, the floor taken exactly from the fp32 exponent."""
    return ops.roi_map_levels(rois, num_levels, finest_scale)


def roi_align(feats, rois, out_size=7, featmap_strides=(4, 8, 16, 32), sampling_ratio=2, finest_scale=56):
    """RoIAlign of every row of ``rois`` (R, 5) = (batch_idx, x1, y1, x2, y2) in input pixels on its FPN level.

    ``feats``: one (B, C, H_l, W_l) bfloat16 / float16 CUDA tensor per entry of ``featmap_strides`` (NHWC memory read
    in place, other layouts transposed once).  Rows whose batch index is outside ``[0, B)`` (the -1 padding of
    :func:`rois_from_proposals`) give zeros and no gradient.  Returns (R, C, out_size, out_size) in the features'
    dtype, channels_last.  Differentiable in ``feats``."""
    return RoIAlignFunction.apply(rois, int(out_size), tuple(featmap_strides), int(sampling_ratio),
                                  float(finest_scale), *feats)


def rois_from_proposals(proposals, counts):
    """``rpn_proposals``' padded (B, max_num, 5) proposals and (B,) int32 counts -> (B*max_num, 5) rois
    (batch_idx, x1, y1, x2, y2); rows at or past ``counts[b]`` get batch index -1.  No host synchronisation."""
    return ops.rois_from_proposals(proposals, counts)


class SingleRoIExtractor(torch.nn.Module):
    """mmdetection v1's ``SingleRoIExtractor``: each RoI is pooled from one level chosen by its scale.  Uses the
    first ``len(featmap_strides)`` of the levels it is given (an FPN's P6 then gets no gradient).  No parameters."""

    def __init__(self, roi_layer=dict(type='RoIAlign', out_size=7, sample_num=2), out_channels=256,
                 featmap_strides=[4, 8, 16, 32], finest_scale=56):
        super().__init__()
        cfg = dict(roi_layer)
        layer = cfg.pop('type', None)
        if layer != 'RoIAlign':
            raise ValueError("SingleRoIExtractor supports roi_layer type 'RoIAlign' only, got %r" % (layer,))
        self.out_size = int(cfg.pop('out_size', 7))
        self.sample_num = int(cfg.pop('sample_num', 2))
        if cfg:
            raise ValueError("unsupported RoIAlign options: %s" % sorted(cfg))
        self.out_channels = int(out_channels)
        self.featmap_strides = tuple(featmap_strides)
        self.finest_scale = finest_scale

    @property
    def num_inputs(self):
        return len(self.featmap_strides)

    def init_weights(self):
        pass

    def map_roi_levels(self, rois, num_levels):
        return map_roi_levels(rois, num_levels, self.finest_scale)

    def forward(self, feats, rois):
        feats = list(feats)
        if len(feats) < self.num_inputs:
            raise ValueError("%d feature levels given, %d expected" % (len(feats), self.num_inputs))
        feats = feats[:self.num_inputs]
        if feats[0].dim() != 4 or feats[0].shape[1] != self.out_channels:
            raise ValueError("features have %s channels, out_channels is %d" %
                             (tuple(feats[0].shape)[1:2], self.out_channels))
        return roi_align(feats, rois, self.out_size, self.featmap_strides, self.sample_num, self.finest_scale)
