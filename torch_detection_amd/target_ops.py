"""Host wrappers of the training-target kernels (csrc/target.hip): every shape, dtype and limit is
checked here, before any launch (ValueError); outputs and the workspace are allocated here, the library allocates
nothing and never synchronises, so every call can be captured in a graph.

These live beside ``ops.py`` rather than in it: ``tests/test_gpu_guarded.py`` demands of every public function of
``ops.py`` that its own cases ran it, and ``tests/test_gpu_targets.py`` puts THIS module under the same guard
(``guard_util.install`` needs only the ``torch`` / ``_workspace`` / ``_aligned_ws`` names below).
"""
import ctypes

import torch

from . import _lib
from .ops import _aligned_ws, _chk_dev, _ptr, _workspace  # noqa: F401  (_workspace: swapped by the guard)


def _scalar(v, name):
    if isinstance(v, (tuple, list)) or torch.is_tensor(v):
        raise ValueError("%s must be a scalar (tuple thresholds are not supported)" % name)
    v = float(v)
    if v != v:
        raise ValueError("%s is NaN" % name)
    return v


def _chk_t(t, name, dtype, shape=None, ndim=None):
    if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or \
            (shape is not None and tuple(t.shape) != tuple(shape)) or (ndim is not None and t.dim() != ndim):
        raise ValueError("%s must be a contiguous CUDA %s tensor%s, got %s" % (
            name, str(dtype).replace("torch.", ""), " of shape %s" % (tuple(shape),) if shape is not None else "",
            (t.dtype, str(t.device), tuple(t.shape)) if torch.is_tensor(t) else type(t)))
    _chk_dev(t, name)


def _chk_gt(gt_bboxes, gt_counts):
    if not torch.is_tensor(gt_bboxes) or gt_bboxes.dim() != 3 or gt_bboxes.shape[2] != 4:
        raise ValueError("gt_bboxes must be a (B, G, 4) tensor (zero rows past gt_counts)")
    B, G = gt_bboxes.shape[0], gt_bboxes.shape[1]
    _chk_t(gt_bboxes, "gt_bboxes", torch.float32)
    if not 1 <= B <= 64:
        raise ValueError("batch size must be 1..64, got %d" % B)
    if G > _lib.TARGET_MAX_GT:
        raise ValueError("%d ground truths per image (max %d)" % (G, _lib.TARGET_MAX_GT))
    _chk_t(gt_counts, "gt_counts", torch.int32, (B,))
    return B, G


def _chk_boxes(boxes, B, name):
    """(N, 4) shared by all images or (B, N, 4) -> (N, floats between images)."""
    if not torch.is_tensor(boxes) or boxes.dim() not in (2, 3) or boxes.shape[-1] != 4 or \
            (boxes.dim() == 3 and boxes.shape[0] != B):
        raise ValueError("%s must be (N, 4) or (B, N, 4) with B = %d" % (name, B))
    _chk_t(boxes, name, torch.float32)
    N = boxes.shape[-2]
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%s: %d boxes per image (max %d)" % (name, N, _lib.TARGET_MAX_BOXES))
    return N, (N * 4 if boxes.dim() == 3 else 0)


def _chk_valid(valid, B, N, name):
    """(N,) shared by all images or (B, N), uint8 or bool, whatever the boxes' shape -> (tensor, bytes between images)."""
    if valid is None:
        return None, 0
    if torch.is_tensor(valid) and valid.dtype == torch.bool and valid.is_contiguous():
        valid = valid.view(torch.uint8)
    if not torch.is_tensor(valid) or tuple(valid.shape) not in ((N,), (B, N)):
        raise ValueError("%s must be (N,) or (B, N) with B = %d, N = %d" % (name, B, N))
    _chk_t(valid, name, torch.uint8)
    return valid, (N if valid.dim() == 2 else 0)


def _sampling(cfg, num, pos_fraction, neg_pos_ub):
    num = int(num)
    if not 0 <= num <= _lib.TARGET_MAX_NUM:
        raise ValueError("num must be in 0..%d" % _lib.TARGET_MAX_NUM)
    pos_fraction = _scalar(pos_fraction, "pos_fraction")
    if not 0.0 <= pos_fraction <= 1.0:
        raise ValueError("pos_fraction must be in [0, 1]")
    cfg.num, cfg.num_pos_expected = num, int(num * pos_fraction)
    cfg.neg_pos_ub = _scalar(neg_pos_ub, "neg_pos_ub")
    return num


def _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all):
    cfg.pos_iou_thr = _scalar(pos_iou_thr, "pos_iou_thr")
    cfg.neg_iou_thr = _scalar(neg_iou_thr, "neg_iou_thr")
    cfg.min_pos_iou = _scalar(min_pos_iou, "min_pos_iou")
    cfg.gt_max_assign_all = 1 if gt_max_assign_all else 0


def _f4(cfg, means, stds):
    if len(means) != 4 or len(stds) != 4:
        raise ValueError("target_means / target_stds must have 4 entries")
    cfg.means[:] = [float(x) for x in means]
    cfg.stds[:] = [float(x) for x in stds]


def _chk_keys(keys, shape):
    if keys is not None:
        _chk_t(keys, "keys", torch.int32, shape)


def assign_max_iou(boxes, gt_bboxes, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all, valid):
    B, G = _chk_gt(gt_bboxes, gt_counts)
    N, stride = _chk_boxes(boxes, B, "boxes")
    valid, vstride = _chk_valid(valid, B, N, "valid")
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    dev = boxes.device
    assigned = torch.empty(B, N, dtype=torch.int32, device=dev)
    max_overlaps = torch.empty(B, N, dtype=torch.float32, device=dev)
    lib = _lib.load()
    nbytes = lib.tdn_assign_max_iou_workspace_bytes(B, G)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_assign_max_iou(_ptr(boxes), stride, _ptr(valid), vstride, _ptr(gt_bboxes), _ptr(gt_counts), B, N, G,
                                      ctypes.byref(cfg), _ptr(assigned), _ptr(max_overlaps), wp, nbytes,
                                      _lib.stream_ptr()), "tdn_assign_max_iou")
    return assigned, max_overlaps


def sample_assigned(assigned_gt_inds, num, pos_fraction, neg_pos_ub, keys, seed):
    if not torch.is_tensor(assigned_gt_inds) or assigned_gt_inds.dim() != 2:
        raise ValueError("assigned_gt_inds must be a (B, N) int32 tensor")
    _chk_t(assigned_gt_inds, "assigned_gt_inds", torch.int32)
    B, N = assigned_gt_inds.shape
    if not 1 <= B <= 64:
        raise ValueError("batch size must be 1..64, got %d" % B)
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%d boxes per image (max %d)" % (N, _lib.TARGET_MAX_BOXES))
    _chk_keys(keys, (B, N))
    cfg = _lib.TargetConfig()
    _sampling(cfg, num, pos_fraction, neg_pos_ub)
    cfg.seed = int(seed) & 0xFFFFFFFF
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
    B, G = _chk_gt(gt_bboxes, gt_counts)
    N, stride = _chk_boxes(anchors, B, "anchors")
    valid_flags, vstride = _chk_valid(valid_flags, B, N, "valid_flags")
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    _sampling(cfg, num, pos_fraction, neg_pos_ub)
    _f4(cfg, means, stds)
    cfg.seed = int(seed) & 0xFFFFFFFF
    cfg.allowed_border = int(allowed_border)
    if cfg.allowed_border >= 0 or img_shapes is not None:
        _chk_t(img_shapes, "img_shapes", torch.int32, (B, 2))
    _chk_keys(keys, (B, N))
    dev = anchors.device
    labels = torch.empty(B, N, dtype=torch.int64, device=dev)
    label_weights = torch.empty(B, N, dtype=torch.float32, device=dev)
    bbox_targets = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
    bbox_weights = torch.empty(B, N, 4, dtype=torch.float32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    assigned = torch.empty(B, N, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = lib.tdn_anchor_target_workspace_bytes(B, N, G)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_anchor_target(_ptr(anchors), stride, _ptr(valid_flags), vstride, _ptr(gt_bboxes), _ptr(gt_counts),
                                     _ptr(img_shapes), B, N, G, ctypes.byref(cfg), _ptr(keys), _ptr(labels),
                                     _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights), _ptr(num_pos),
                                     _ptr(num_neg), _ptr(assigned), wp, nbytes, _lib.stream_ptr()),
               "tdn_anchor_target")
    return labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, assigned


def sample_rois(proposals, counts, gt_bboxes, gt_labels, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou,
                gt_max_assign_all, num, pos_fraction, neg_pos_ub, add_gt_as_proposals, means, stds, keys, seed):
    B, G = _chk_gt(gt_bboxes, gt_counts)
    if not torch.is_tensor(proposals) or proposals.dim() != 3 or proposals.shape[0] != B or proposals.shape[2] != 5:
        raise ValueError("proposals must be (B, P, 5) with B = %d, as rpn_proposals returns them" % B)
    _chk_t(proposals, "proposals", torch.float32)
    P = proposals.shape[1]
    if P > _lib.TARGET_MAX_BOXES - _lib.TARGET_MAX_GT:
        raise ValueError("%d proposals per image (max %d)" % (P, _lib.TARGET_MAX_BOXES - _lib.TARGET_MAX_GT))
    _chk_t(counts, "counts", torch.int32, (B,))
    _chk_t(gt_labels, "gt_labels", torch.int64, (B, G))
    cfg = _lib.TargetConfig()
    _thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    num = _sampling(cfg, num, pos_fraction, neg_pos_ub)
    _f4(cfg, means, stds)
    cfg.seed = int(seed) & 0xFFFFFFFF
    cfg.add_gt_as_proposals = 1 if add_gt_as_proposals else 0
    cfg.allowed_border = -1
    Nc = P + (G if add_gt_as_proposals else 0)
    _chk_keys(keys, (B, Nc))
    dev = proposals.device
    rois = torch.empty(B * num, 5, dtype=torch.float32, device=dev)
    labels = torch.empty(B * num, dtype=torch.int64, device=dev)
    label_weights = torch.empty(B * num, dtype=torch.float32, device=dev)
    bbox_targets = torch.empty(B * num, 4, dtype=torch.float32, device=dev)
    bbox_weights = torch.empty(B * num, 4, dtype=torch.float32, device=dev)
    pos_gt_inds = torch.empty(B * num, dtype=torch.int32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nbytes = lib.tdn_sample_rois_workspace_bytes(B, P, G, cfg.add_gt_as_proposals)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_sample_rois(_ptr(proposals), _ptr(counts), _ptr(gt_bboxes), _ptr(gt_labels), _ptr(gt_counts),
                                   B, P, G, ctypes.byref(cfg), _ptr(keys), _ptr(rois), _ptr(labels),
                                   _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights), _ptr(pos_gt_inds),
                                   _ptr(num_pos), _ptr(num_neg), wp, nbytes, _lib.stream_ptr()), "tdn_sample_rois")
    return rois, labels, label_weights, bbox_targets, bbox_weights, pos_gt_inds, num_pos, num_neg
