"""Host wrappers of the training-target kernels (csrc/target.hip), written in the vocabulary of
``_args.py``: every shape, dtype and limit is checked here, before any launch (ValueError) — shapes,
limits and scalars first, so that those refusals need no GPU, the device last; outputs and the workspace are allocated
here, the library allocates nothing and never synchronises, so every call can be captured in a graph.

These live beside ``ops.py`` rather than in it: ``tests/test_gpu_guarded.py`` demands of every public function of
``ops.py`` that its own cases ran it, and ``tests/test_gpu_targets.py`` puts THIS module under the same guard
(``guard_util.install`` needs only the ``torch`` / ``_workspace`` / ``_aligned_ws`` names below).
"""
import ctypes

import torch

from . import _lib
from ._args import batch, f4, integer, number, on_device, tensor
from .ops import _aligned_ws, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)

F32 = torch.float32


def _gt(gt_bboxes, gt_counts):
    B, G, _ = tensor(gt_bboxes, "gt_bboxes", F32, ("B", "G", 4))          # zero rows past gt_counts
    batch(B)
    if G > _lib.TARGET_MAX_GT:
        raise ValueError("%d ground truths per image (max %d)" % (G, _lib.TARGET_MAX_GT))
    tensor(gt_counts, "gt_counts", torch.int32, (B,))
    return B, G


def _boxes(boxes, B, name):
    """(N, 4) shared by all images or (B, N, 4) -> (N, floats between images)."""
    shared = torch.is_tensor(boxes) and boxes.dim() == 2
    N = tensor(boxes, name, F32, ("N", 4) if shared else (B, "N", 4))[-2]
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%s: %d boxes per image (max %d)" % (name, N, _lib.TARGET_MAX_BOXES))
    return N, (0 if shared else N * 4)


def _valid(valid, B, N, name):
    """(N,) shared by all images or (B, N), uint8 or bool, whatever the boxes' shape -> (tensor, bytes between images)."""
    if valid is None:
        return None, 0
    shared = torch.is_tensor(valid) and valid.dim() == 1
    tensor(valid, name, (torch.uint8, torch.bool), (N,) if shared else (B, N))
    return valid.view(torch.uint8), (0 if shared else N)


def _sampling(cfg, num, pos_fraction, neg_pos_ub, seed):
    cfg.num = integer(num, "num", 0, _lib.TARGET_MAX_NUM)
    pos_fraction = number(pos_fraction, "pos_fraction")
    if not 0.0 <= pos_fraction <= 1.0:
        raise ValueError("pos_fraction must be in [0, 1]")
    cfg.num_pos_expected = int(cfg.num * pos_fraction)
    cfg.neg_pos_ub = number(neg_pos_ub, "neg_pos_ub")
    cfg.seed = int(seed) & 0xFFFFFFFF
    return cfg.num


def _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all):
    """Scalar thresholds only: a tuple ``neg_iou_thr`` is refused."""
    cfg.pos_iou_thr = number(pos_iou_thr, "pos_iou_thr")
    cfg.neg_iou_thr = number(neg_iou_thr, "neg_iou_thr")
    cfg.min_pos_iou = number(min_pos_iou, "min_pos_iou")
    cfg.gt_max_assign_all = 1 if gt_max_assign_all else 0


def _keys(keys, shape):
    if keys is not None:
        tensor(keys, "keys", torch.int32, shape)


def assign_max_iou(boxes, gt_bboxes, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all, valid):
    B, G = _gt(gt_bboxes, gt_counts)
    N, stride = _boxes(boxes, B, "boxes")
    valid, vstride = _valid(valid, B, N, "valid")
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    on_device([("boxes", boxes), ("gt_bboxes", gt_bboxes), ("gt_counts", gt_counts), ("valid", valid)])
    dev = boxes.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_assign_max_iou_workspace_bytes(B, G), "assign_max_iou")
    assigned = torch.empty(B, N, dtype=torch.int32, device=dev)
    max_overlaps = torch.empty(B, N, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_assign_max_iou(_ptr(boxes), stride, _ptr(valid), vstride, _ptr(gt_bboxes), _ptr(gt_counts), B, N, G,
                                      ctypes.byref(cfg), _ptr(assigned), _ptr(max_overlaps), wp, nbytes,
                                      _lib.stream_ptr()), "tdn_assign_max_iou")
    return assigned, max_overlaps


def sample_assigned(assigned_gt_inds, num, pos_fraction, neg_pos_ub, keys, seed):
    B, N = tensor(assigned_gt_inds, "assigned_gt_inds", torch.int32, ("B", "N"))
    batch(B)
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%d boxes per image (max %d)" % (N, _lib.TARGET_MAX_BOXES))
    _keys(keys, (B, N))
    cfg = _lib.TargetConfig()
    _sampling(cfg, num, pos_fraction, neg_pos_ub, seed)
    on_device([("assigned_gt_inds", assigned_gt_inds), ("keys", keys)])
    dev = assigned_gt_inds.device
    pos_mask = torch.empty(B, N, dtype=torch.uint8, device=dev)
    neg_mask = torch.empty(B, N, dtype=torch.uint8, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tdn_sample_assigned(_ptr(assigned_gt_inds), B, N, ctypes.byref(cfg), _ptr(keys),
                                               _ptr(pos_mask), _ptr(neg_mask), _ptr(num_pos), _ptr(num_neg),
                                               _lib.stream_ptr()), "tdn_sample_assigned")
    return pos_mask, neg_mask, num_pos, num_neg


def anchor_target(anchors, valid_flags, gt_bboxes, gt_counts, img_shapes, pos_iou_thr, neg_iou_thr, min_pos_iou,
                  gt_max_assign_all, num, pos_fraction, neg_pos_ub, allowed_border, means, stds, keys, seed):
    B, G = _gt(gt_bboxes, gt_counts)
    N, stride = _boxes(anchors, B, "anchors")
    valid_flags, vstride = _valid(valid_flags, B, N, "valid_flags")
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    _sampling(cfg, num, pos_fraction, neg_pos_ub, seed)
    cfg.means, cfg.stds = f4(means, "target_means"), f4(stds, "target_stds")
    cfg.allowed_border = int(allowed_border)
    if cfg.allowed_border >= 0 or img_shapes is not None:
        tensor(img_shapes, "img_shapes", torch.int32, (B, 2))
    _keys(keys, (B, N))
    on_device([("anchors", anchors), ("valid_flags", valid_flags), ("gt_bboxes", gt_bboxes), ("gt_counts", gt_counts),
               ("img_shapes", img_shapes), ("keys", keys)])
    dev = anchors.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_anchor_target_workspace_bytes(B, N, G), "anchor_target")
    labels = torch.empty(B, N, dtype=torch.int64, device=dev)
    label_weights = torch.empty(B, N, dtype=torch.float32, device=dev)
    bbox_targets = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
    bbox_weights = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    assigned = torch.empty(B, N, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_anchor_target(_ptr(anchors), stride, _ptr(valid_flags), vstride, _ptr(gt_bboxes), _ptr(gt_counts),
                                     _ptr(img_shapes), B, N, G, ctypes.byref(cfg), _ptr(keys), _ptr(labels),
                                     _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights), _ptr(num_pos),
                                     _ptr(num_neg), _ptr(assigned), wp, nbytes, _lib.stream_ptr()),
               "tdn_anchor_target")
    return labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, assigned


def sample_rois(proposals, counts, gt_bboxes, gt_labels, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou,
                gt_max_assign_all, num, pos_fraction, neg_pos_ub, add_gt_as_proposals, means, stds, keys, seed):
    B, G = _gt(gt_bboxes, gt_counts)
    P = tensor(proposals, "proposals", F32, (B, "P", 5))[1]               # as rpn_proposals returns them
    if P > _lib.TARGET_MAX_BOXES - _lib.TARGET_MAX_GT:
        raise ValueError("%d proposals per image (max %d)" % (P, _lib.TARGET_MAX_BOXES - _lib.TARGET_MAX_GT))
    tensor(counts, "counts", torch.int32, (B,))
    tensor(gt_labels, "gt_labels", torch.int64, (B, G))
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    num = _sampling(cfg, num, pos_fraction, neg_pos_ub, seed)
    cfg.means, cfg.stds = f4(means, "target_means"), f4(stds, "target_stds")
    cfg.add_gt_as_proposals = 1 if add_gt_as_proposals else 0
    cfg.allowed_border = -1
    _keys(keys, (B, P + (G if add_gt_as_proposals else 0)))
    on_device([("proposals", proposals), ("counts", counts), ("gt_bboxes", gt_bboxes), ("gt_labels", gt_labels),
               ("gt_counts", gt_counts), ("keys", keys)])
    dev = proposals.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_sample_rois_workspace_bytes(B, P, G, cfg.add_gt_as_proposals), "sample_rois")
    rois = torch.empty(B * num, 5, dtype=torch.float32, device=dev)
    labels = torch.empty(B * num, dtype=torch.int64, device=dev)
    label_weights = torch.empty(B * num, dtype=torch.float32, device=dev)
    bbox_targets = torch.empty(B * num, 4, dtype=torch.float32, device=dev)
    bbox_weights = torch.empty(B * num, 4, dtype=torch.float32, device=dev)
    pos_gt_inds = torch.empty(B * num, dtype=torch.int32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_sample_rois(_ptr(proposals), _ptr(counts), _ptr(gt_bboxes), _ptr(gt_labels), _ptr(gt_counts),
                                   B, P, G, ctypes.byref(cfg), _ptr(keys), _ptr(rois), _ptr(labels),
                                   _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights), _ptr(pos_gt_inds),
                                   _ptr(num_pos), _ptr(num_neg), wp, nbytes, _lib.stream_ptr()), "tdn_sample_rois")
    return rois, labels, label_weights, bbox_targets, bbox_weights, pos_gt_inds, num_pos, num_neg
