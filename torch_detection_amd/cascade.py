"""Cascade R-CNN (DESIGN.md §4q has the specification, tests/cascade_ref.py restates it): the box head run more than once.

``refine_bboxes`` is mmdetection v1's ``BBoxHead.refine_bboxes`` / ``regress_by_class`` for a whole batch: every RoI
decoded by the deltas of its own class, handed back either row for row (test time, what ``roi_align`` reads) or compacted
per image without the ground truths (training, what ``sample_rois`` reads).  ``cascade_detections`` is
``bbox_head_detections`` on the mean of the stages' class logits (``CascadeRCNN.simple_test``).  ``CascadeRoIHead`` is the
orchestration: per stage ``sample_rois`` -> extractor -> ``BBoxHead`` -> ``bbox_head_loss`` -> ``refine_bboxes``.  Nothing
synchronises with the host, so a whole training or test step can be captured in a graph; outputs have fixed shapes and
are a pure function of the inputs.
"""
import torch
import torch.nn as nn

from . import cascade_ops as _c
from .heads import BBoxHead
from .losses import bbox_head_loss
from .registry import HEADS
from .roi import SingleRoIExtractor, rois_from_proposals
from .target import sample_rois

__all__ = ["refine_bboxes", "cascade_detections", "CascadeRoIHead"]


def _detached(t):
    return t.detach() if torch.is_tensor(t) else t


def refine_bboxes(rois, bbox_pred, img_shapes, labels=None, cls_score=None, pos_assigned_gt_inds=None, gt_bboxes=None,
                  max_per_img=None, target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2),
                  wh_ratio_clip=16 / 1000):
    """The RoIs of the next cascade stage: every row of ``rois`` decoded by the deltas of one class.

    ``rois``: (R, 5) float32 = (batch_idx, x1, y1, x2, y2); rows with an index outside ``[0, B)`` are padding.
    ``bbox_pred``: (R, 4C) — row r reads columns ``4 * label ..``, label 0 the background's, as mmdetection does — or
    (R, 4); float32 / bfloat16 / float16.  ``img_shapes``: CUDA int32 (B, 2) of (h, w).  Exactly one of ``labels``
    ((R,) int64, ``sample_rois``' labels) and ``cls_score`` ((R, C), ``bbox_pred``'s dtype: the label is the arg-max
    over all C columns, ties to the lowest column) is given; with (R, 4C) deltas a given label outside ``[0, C)`` makes
    the row padding.  The new box is ``delta2bbox(rois[r, 1:], deltas, means, stds, max_shape=img_shapes[b])``.

    ``max_per_img=None`` (test time): returns (R, 5) float32, row r = [b, box] of input row r, padding rows
    [-1, 0, 0, 0, 0]; no row moves.  One launch.

    ``max_per_img=P`` (training): returns ``proposals`` (B, P, 5) float32 = [x1, y1, x2, y2, 0] and ``counts`` (B,)
    int32 as ``sample_rois`` reads them: image b's kept rows in ascending input row, the first P of them, zeros past
    ``counts[b] = min(kept, P)``.  Padding rows are dropped; with ``pos_assigned_gt_inds`` (R,) int32 and ``gt_bboxes``
    (B, G, 4) so is every row whose index is >= 0 and whose four coordinates are bitwise those of
    ``gt_bboxes[b, index]`` — the ground truths ``sample_rois`` prepended (mmdetection's ``pos_is_gt``), and a proposal
    that coincides bitwise with its own ground truth, which the next stage's ``add_gt_as_proposals`` re-adds.  Two
    launches.

    Not differentiable (mmdetection runs it under ``no_grad``).  Limits: B 1..64, R <= 2^18, C 1..1024, P 1..8192."""
    return _c.refine_bboxes(_detached(rois), _detached(bbox_pred), img_shapes, _detached(labels), _detached(cls_score),
                            _detached(pos_assigned_gt_inds), _detached(gt_bboxes), max_per_img, target_means,
                            target_stds, wh_ratio_clip)


def cascade_detections(rois, cls_scores, bbox_pred, img_shapes, scale_factors=None, score_thr=0.05, nms_thr=0.5,
                       max_per_img=100, target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2),
                       wh_ratio_clip=16 / 1000, return_dense=False, nms=None):
    """Detections from several stages' class logits (mmdetection v1's ``CascadeRCNN.simple_test`` for a whole batch).

    ``cls_scores``: a list of S = 1..8 (R, C) tensors of one dtype (float32 / bfloat16 / float16), all on the rows of
    ``rois``; the logit of (r, c) is ``(((x_0 + x_1) + ...) + x_{S-1}) / float(S)`` — fp32 additions in stage order, one
    fp32 division.  From there on it is :func:`bbox_head_detections` operation for operation, with ``bbox_pred`` the
    last stage's deltas against ``rois``, the last stage's input RoIs; same launch count for any S, same outputs and
    limits, and with one stage the same bits.  ``nms``: as :func:`multiclass_nms` takes it."""
    out = _c.cascade_detections(rois, [_detached(x) for x in cls_scores] if isinstance(cls_scores, (list, tuple))
                                else cls_scores, _detached(bbox_pred), img_shapes, scale_factors, score_thr, nms_thr,
                                max_per_img, target_means, target_stds, wh_ratio_clip, nms)
    return out if return_dense else out[:4]


# ---- the module -----------------------------------------------------------------------------------------------------
STAGE_IOU = (0.5, 0.6, 0.7)
STAGE_STDS = ((0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1), (0.033, 0.033, 0.067, 0.067))
_TRAIN_KEYS = ("pos_iou_thr", "neg_iou_thr", "min_pos_iou", "num", "pos_fraction", "neg_pos_ub", "add_gt_as_proposals")


def _per_stage(value, n, what):
    """One entry per stage from one shared entry or a list of n."""
    if isinstance(value, (list, tuple)) and len(value) and isinstance(value[0], (list, tuple, dict)):
        if len(value) != n:
            raise ValueError("CascadeRoIHead: %s has %d entries for %d stages" % (what, len(value), n))
        return list(value)
    return [value] * n


def _stage_defaults(defaults, n, what):
    if n > len(defaults):
        raise ValueError("CascadeRoIHead: %s has defaults for %d stages only, give %d" % (what, len(defaults), n))
    return list(defaults[:n])


@HEADS.register_module
class CascadeRoIHead(nn.Module):
    """The RoI side of mmdetection v1's ``CascadeRCNN``: ``num_stages`` box heads, each trained on the boxes the one
    before it refined, at a rising IoU threshold; at test time the stages' class logits are averaged.

    ``bbox_roi_extractor`` / ``bbox_head``: one config dict shared by the stages' constructors, or a list of one per
    stage (``type`` defaults to ``SingleRoIExtractor`` / ``BBoxHead``); the sub-modules are ``bbox_roi_extractor.{i}``
    and ``bbox_head.{i}``, so the state-dict keys are mmdetection's.  ``train_cfg``: one flat dict per stage with
    ``pos_iou_thr`` / ``neg_iou_thr`` / ``min_pos_iou``, ``num``, ``pos_fraction``, ``add_gt_as_proposals`` (and
    ``neg_pos_ub``), the arguments of ``sample_rois``.  ``target_means`` / ``target_stds``: one 4-tuple for all stages
    or one per stage.  Mask stages (``mask_roi_extractor`` / ``mask_head``), a ``shared_head`` and ``roi_layer`` types
    other than RoIAlign are accepted here and raise ``NotImplementedError`` in ``forward_train`` / ``simple_test``."""

    def __init__(self, num_stages=3, stage_loss_weights=(1, 0.5, 0.25), bbox_roi_extractor=None, bbox_head=None,
                 train_cfg=None, target_means=(0.0, 0.0, 0.0, 0.0), target_stds=None, mask_roi_extractor=None,
                 mask_head=None, shared_head=None):
        super().__init__()
        n = int(num_stages)
        if n < 1 or n > _c._lib.CASCADE_MAX_STAGES:
            raise ValueError("CascadeRoIHead: num_stages must be in 1..%d, got %d" % (_c._lib.CASCADE_MAX_STAGES, n))
        self.num_stages = n
        self.stage_loss_weights = tuple(float(w) for w in stage_loss_weights)
        if len(self.stage_loss_weights) != n:
            raise ValueError("CascadeRoIHead: %d stage_loss_weights for %d stages" % (len(self.stage_loss_weights), n))
        self._unsupported = None
        if mask_roi_extractor is not None or mask_head is not None:
            self._unsupported = "mask stages (Cascade Mask R-CNN) are not on the HIP path"
        elif shared_head is not None:
            self._unsupported = "a shared_head is not on the HIP path"
        if bbox_roi_extractor is None:
            bbox_roi_extractor = dict(type='SingleRoIExtractor', roi_layer=dict(type='RoIAlign', out_size=7, sample_num=2),
                                      out_channels=256, featmap_strides=[4, 8, 16, 32])
        if bbox_head is None:
            bbox_head = dict(type='BBoxHead', num_fcs=2, in_channels=256, fc_out_channels=1024, roi_feat_size=7,
                             num_classes=81, reg_class_agnostic=True)
        self.bbox_roi_extractor = nn.ModuleList()
        self.bbox_head = nn.ModuleList()
        for cfg in _per_stage(bbox_roi_extractor, n, "bbox_roi_extractor"):
            cfg = dict(cfg)
            kind = cfg.pop('type', 'SingleRoIExtractor')
            layer = dict(cfg.get('roi_layer', dict(type='RoIAlign')))
            if kind != 'SingleRoIExtractor' or layer.get('type') != 'RoIAlign':
                self._unsupported = self._unsupported or ("bbox_roi_extractor %r with roi_layer %r is not on the HIP path "
                                                          "(SingleRoIExtractor with RoIAlign)" % (kind, layer.get('type')))
                cfg['roi_layer'] = dict(type='RoIAlign', out_size=layer.get('out_size', 7))   # a stand-in, never run
            self.bbox_roi_extractor.append(SingleRoIExtractor(**cfg))
        for cfg in _per_stage(bbox_head, n, "bbox_head"):
            cfg = dict(cfg)
            kind = cfg.pop('type', 'BBoxHead')
            if kind != 'BBoxHead':
                raise ValueError("CascadeRoIHead: bbox_head type %r (only 'BBoxHead')" % (kind,))
            cfg.setdefault('reg_class_agnostic', True)
            self.bbox_head.append(BBoxHead(**cfg))
        if train_cfg is None:
            train_cfg = [dict(pos_iou_thr=t, neg_iou_thr=t, min_pos_iou=t, num=512, pos_fraction=0.25,
                              add_gt_as_proposals=True) for t in _stage_defaults(STAGE_IOU, n, "train_cfg")]
        self.train_cfg = [dict(c) for c in _per_stage(list(train_cfg) if isinstance(train_cfg, (list, tuple))
                                                      else train_cfg, n, "train_cfg")]
        for c in self.train_cfg:
            extra = sorted(set(c) - set(_TRAIN_KEYS))
            if extra or "num" not in c:
                raise ValueError("CascadeRoIHead: a train_cfg entry takes %s (num is required), got %s"
                                 % (", ".join(_TRAIN_KEYS), sorted(c)))
        if target_stds is None:
            target_stds = _stage_defaults(STAGE_STDS, n, "target_stds")
        self.target_means = [tuple(float(v) for v in m) for m in _per_stage(tuple(target_means), n, "target_means")]
        self.target_stds = [tuple(float(v) for v in s) for s in _per_stage(tuple(target_stds), n, "target_stds")]

    def init_weights(self):
        for h in self.bbox_head:
            h.init_weights()

    def _check_supported(self):
        if self._unsupported:
            raise NotImplementedError("CascadeRoIHead: " + self._unsupported)

    def forward_train(self, feats, proposals, counts, gt_bboxes, gt_labels, gt_counts, img_shapes, seed=0):
        """``proposals`` (B, P, 5) / ``counts`` (B,) as ``rpn_proposals`` returns them -> a dict of ``s{i}.loss_cls`` /
        ``s{i}.loss_bbox``, already multiplied by ``stage_loss_weights[i]``.  Stage i samples with seed ``seed + i``
        from the boxes stage i - 1 refined with its own labels' deltas, the ground truths dropped."""
        self._check_supported()
        losses = {}
        for i in range(self.num_stages):
            cfg = self.train_cfg[i]
            rois, labels, label_weights, bbox_targets, bbox_weights, gt_inds, _, _ = sample_rois(
                proposals, counts, gt_bboxes, gt_labels, gt_counts, target_means=self.target_means[i],
                target_stds=self.target_stds[i], seed=seed + i, **cfg)
            x = self.bbox_roi_extractor[i](feats, rois)
            cls_score, bbox_pred = self.bbox_head[i](x)
            loss = bbox_head_loss(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights)
            losses["s%d.loss_cls" % i] = loss[0] * self.stage_loss_weights[i]
            losses["s%d.loss_bbox" % i] = loss[1] * self.stage_loss_weights[i]
            if i < self.num_stages - 1:
                proposals, counts = refine_bboxes(rois, bbox_pred, img_shapes, labels=labels,
                                                  pos_assigned_gt_inds=gt_inds, gt_bboxes=gt_bboxes,
                                                  max_per_img=cfg["num"], target_means=self.target_means[i],
                                                  target_stds=self.target_stds[i])
        return losses

    @torch.no_grad()
    def simple_test(self, feats, proposals, counts, img_shapes, scale_factors=None, score_thr=0.05, nms_thr=0.5,
                    max_per_img=100, nms=None):
        """-> ``(dets, labels, row_idx, counts)`` of :func:`cascade_detections`: every stage's logits on the RoIs it
        was given, averaged; boxes from the last stage's deltas against the last stage's input RoIs.  ``nms``: the
        ``test_cfg``'s ``nms`` dict, as :func:`cascade_detections` takes it."""
        self._check_supported()
        rois = rois_from_proposals(proposals, counts)
        scores = []
        last = self.num_stages - 1
        for i in range(self.num_stages):
            x = self.bbox_roi_extractor[i](feats, rois)
            cls_score, bbox_pred = self.bbox_head[i](x)
            scores.append(cls_score)
            if i < last:
                rois = refine_bboxes(rois, bbox_pred, img_shapes, cls_score=cls_score,
                                     target_means=self.target_means[i], target_stds=self.target_stds[i])
        return cascade_detections(rois, scores, bbox_pred, img_shapes, scale_factors, score_thr, nms_thr, max_per_img,
                                  self.target_means[last], self.target_stds[last], nms=nms)
