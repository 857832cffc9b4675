"""Host wrappers of the Libra R-CNN kernels: the Balanced Feature Pyramid (csrc/bfp.hip), the RoI box
loss with balanced L1 (csrc/loss.hip, beside ``loss_ops.py``'s smooth-L1 pair) and IoU-balanced negative sampling
(csrc/target.hip, beside ``target_ops.py``'s random sampler), written in the vocabulary of ``_args.py``:
every dtype, layout and limit is checked here, before any launch (ValueError that names the argument) — dtypes, layouts
and sizes first, so that those refusals need no GPU, the device last.

A pyramid is a list of 1..8 levels of one batch size B (1..64) and one channel count C (a multiple of 8 in 8..1024).  The
maps ``xs[l]`` are logical (B, C, H_l, W_l) 16-bit tensors in channels_last MEMORY (``t.permute(0, 2, 3, 1)`` is
contiguous); the level sizes stand in no relation to one another.  ``bsf`` and its cotangent are (B, C, Hg, Wg), the size
of level ``refine_level``.  A cotangent that is not channels_last memory of the compute dtype is brought there by ONE copy
(``dense_ops.cotangents``).  One launch per call, no workspace.

Like the other ``*_ops`` modules this lives beside ``ops.py`` rather than in it; ``tests/test_gpu_bfp.py`` and
``tests/test_gpu_libra.py`` put THIS module under the guard of ``tests/guard_util.py``.
"""
import ctypes

import torch

from . import _lib
from . import target_ops as _t
from ._args import CODES, integer, number, on_device, tensor
from .deconv_ops import _nhwc
from .dense_ops import _levels, cotangents
from .loss_ops import _avg, _roi_setup
from .ops import BF16, F16, _aligned_ws, _ptr, dtype_code
from .ops import _workspace  # noqa: F401  (not called here: the guard swaps the name)

_16 = (BF16, F16)
MAX_LEVELS, MAX_C, MAX_B, MAX_SIDE, MAX_ELEMS = _lib.PYR_MAX_LEVELS, 1024, 64, 32767, (1 << 31) - 1


def _channels(C, name="C"):
    C = integer(C, name, 8, MAX_C)
    if C % 8:
        raise ValueError("%s must be a multiple of 8 in 8..%d, got %d" % (name, MAX_C, C))
    return C


def _refine(refine_level, num_levels):
    num_levels = integer(num_levels, "num_levels", 1, MAX_LEVELS)
    return integer(refine_level, "refine_level", 0, num_levels - 1)


def _maps(xs, name="xs"):
    """The levels' maps: -> (list, dtype, B, C, [(H, W)]).  One dtype, one batch size, one channel count; no level is
    empty (levels are never skipped)."""
    xs = _levels(xs, name)
    B, C, H, W = _nhwc(xs[0], "%s[0]" % name, _16, ("B", "C", "H", "W"))
    C = _channels(C)
    dtype = xs[0].dtype
    sizes = []
    for l, x in enumerate(xs):
        _, _, H, W = _nhwc(x, "%s[%d]" % (name, l), dtype, (B, C, "H", "W"))
        if B < 1 or B > MAX_B:
            raise ValueError("%s[%d]: the batch size must be in 1..%d, got %d" % (name, l, MAX_B, B))
        if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError("%s[%d]: H and W must be in 1..%d, got %d x %d" % (name, l, MAX_SIDE, H, W))
        integer(B * H * W * C, "%s[%d]: B*H*W*C" % (name, l), 1, MAX_ELEMS)
        sizes.append((H, W))
    return xs, dtype, B, C, sizes


def _table(sizes, x=None, out=None, g=None, dx=None):
    arr = (_lib.BfpLevel * len(sizes))()
    ptr = lambda ts, l: ts[l].data_ptr() if ts is not None else None
    for l, (H, W) in enumerate(sizes):
        arr[l].x, arr[l].out, arr[l].g, arr[l].dx = ptr(x, l), ptr(out, l), ptr(g, l), ptr(dx, l)
        arr[l].H, arr[l].W = H, W
    return arr


def _named(name, ts):
    return [("%s[%d]" % (name, l), t) for l, t in enumerate(ts)]


def _new(B, H, W, C, dtype, device):
    return torch.empty((B, H, W, C), dtype=dtype, device=device)


def bfp_gather_fwd(xs, refine_level):
    """-> bsf (B, C, Hg, Wg) in ``xs``'s dtype, channels_last memory: the mean over the levels of each level brought to
    the size of level ``refine_level`` — ``adaptive_max_pool2d`` for the levels before it, ``interpolate(mode='nearest')``
    from it on —, an fp32 sum in ascending level order from +0, one fp32 division, one rounding."""
    xs, dtype, B, C, sizes = _maps(xs)
    r = _refine(refine_level, len(xs))
    on_device(_named("xs", xs))
    bsf = _new(B, sizes[r][0], sizes[r][1], C, dtype, xs[0].device)
    _lib.check(_lib.load().tdn_bfp_gather_fwd(_table(sizes, x=xs), len(xs), r, B, C, _ptr(bsf), dtype_code(dtype),
                                              _lib.stream_ptr()), "tdn_bfp_gather_fwd")
    return bsf.permute(0, 3, 1, 2)


def bfp_scatter_fwd(xs, bsf, refine_level):
    """-> outs: ``outs[l] = resize_l(bsf) + xs[l]`` like ``xs[l]`` — nearest for the levels before ``refine_level``,
    ``adaptive_max_pool2d`` from it on —, one fp32 add, one rounding, all levels in one launch.  ``bsf``: the refined
    map."""
    xs, dtype, B, C, sizes = _maps(xs)
    r = _refine(refine_level, len(xs))
    _nhwc(bsf, "bsf", dtype, (B, C) + sizes[r])
    on_device(_named("xs", xs) + [("bsf", bsf)])
    outs = [_new(B, H, W, C, dtype, xs[0].device) for H, W in sizes]
    _lib.check(_lib.load().tdn_bfp_scatter_fwd(_table(sizes, x=xs, out=outs), len(xs), r, B, C, _ptr(bsf),
                                               dtype_code(dtype), _lib.stream_ptr()), "tdn_bfp_scatter_fwd")
    return [t.permute(0, 3, 1, 2) for t in outs]


def bfp_scatter_bwd(gs, bsf, refine_level):
    """-> dbsf like ``bsf``: the adjoint of ``bfp_scatter_fwd``'s resizes applied to the cotangents ``gs[l]`` of its
    outputs: per level the sum, in row-major order, of the cotangents whose source element this is (for a pooled level:
    whose window has its FIRST maximum here, recomputed from ``bsf``), the levels added in ascending order, fp32, one
    rounding.  The map sizes are the cotangents'."""
    gs = _levels(gs, "gs")
    for l, g in enumerate(gs):
        if not torch.is_tensor(g) or g.dim() != 4:
            raise ValueError("gs[%d] must be a 4-D tensor" % l)
    r = _refine(refine_level, len(gs))
    B, C, Hg, Wg = _nhwc(bsf, "bsf", _16, ("B", "C", "Hg", "Wg"))
    dtype = bsf.dtype
    gs = cotangents(gs, "gs", dtype, B, C, [(g.shape[2], g.shape[3]) for g in gs])
    gs, dtype, B, C, sizes = _maps(gs, "gs")
    if sizes[r] != (Hg, Wg):
        raise ValueError("bsf must have the size of gs[%d], %d x %d, got %d x %d" % ((r,) + sizes[r] + (Hg, Wg)))
    on_device(_named("gs", gs) + [("bsf", bsf)])
    dbsf = _new(B, Hg, Wg, C, dtype, bsf.device)
    _lib.check(_lib.load().tdn_bfp_scatter_bwd(_table(sizes, g=gs), len(gs), r, B, C, _ptr(bsf), _ptr(dbsf),
                                               dtype_code(dtype), _lib.stream_ptr()), "tdn_bfp_scatter_bwd")
    return dbsf.permute(0, 3, 1, 2)


def bfp_gather_bwd(xs, gs, dbsf, refine_level):
    """-> dxs: ``dxs[l] = gs[l] + adjoint_l(dbsf) / L`` like ``xs[l]``: the cotangent of the level's own pass-through plus
    its share of ``bfp_gather_fwd``'s mean — for a pooled level the ``dbsf`` of the windows whose FIRST maximum, recomputed
    from ``xs[l]``, this element is; for a resized level the sum over the elements it was copied to, in row-major order —,
    one fp32 division, one add, one rounding, all levels in one launch."""
    xs, dtype, B, C, sizes = _maps(xs)
    r = _refine(refine_level, len(xs))
    gs = cotangents(gs, "gs", dtype, B, C, sizes)
    _nhwc(dbsf, "dbsf", dtype, (B, C) + sizes[r])
    on_device(_named("xs", xs) + _named("gs", gs) + [("dbsf", dbsf)])
    dxs = [_new(B, H, W, C, dtype, xs[0].device) for H, W in sizes]
    _lib.check(_lib.load().tdn_bfp_gather_bwd(_table(sizes, x=xs, g=gs, dx=dxs), len(xs), r, B, C, _ptr(dbsf),
                                              dtype_code(dtype), _lib.stream_ptr()), "tdn_bfp_gather_bwd")
    return [t.permute(0, 3, 1, 2) for t in dxs]


# ---- RoI box loss with balanced L1 (csrc/loss.hip) ----------------------------------------------------------------------
def _balanced(alpha, gamma):
    alpha, gamma = number(alpha, "reg_alpha", positive=True), number(gamma, "reg_gamma", positive=True)
    if gamma / alpha > 80.0:
        raise ValueError("reg_gamma / reg_alpha must be at most 80 (e^(gamma / alpha) in fp32), got %r" % (gamma / alpha))
    return alpha, gamma


def bbox_head_loss_balanced_fwd(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, avg_factor, beta,
                                alpha, gamma):
    """``loss_ops.bbox_head_loss_fwd`` with balanced L1 (knee ``beta``, ``alpha``, ``gamma``) as the box term:
    -> (losses (2,) float32 = [loss_cls, loss_bbox], the divisor (1,) float32 that the backward call takes)."""
    R, C, cols, beta, named = _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta)
    alpha, gamma = _balanced(alpha, gamma)
    av, avg_ts = _avg(avg_factor, allow_none=True)
    on_device(named + [("avg_factor", t) for t in avg_ts])
    dev = cls_score.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_loss_roi_workspace_bytes(R), "bbox_head_loss")
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    avg = torch.empty(1, dtype=torch.float32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_loss_roi_balanced_fwd(_ptr(cls_score), _ptr(bbox_pred), CODES[cls_score.dtype], R, C, cols,
                                             _ptr(labels), _ptr(label_weights), _ptr(bbox_targets), _ptr(bbox_weights),
                                             beta, alpha, gamma, ctypes.byref(av), _ptr(losses), _ptr(avg), wp, nbytes,
                                             _lib.stream_ptr()), "tdn_loss_roi_balanced_fwd")
    return losses, avg


def bbox_head_loss_balanced_bwd(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, g, avg, beta,
                                alpha, gamma):
    """Gradients of ``g[0] * loss_cls + g[1] * loss_bbox`` in the head outputs' dtype; ``avg``: the forward's divisor."""
    R, C, cols, beta, named = _roi_setup(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, beta)
    alpha, gamma = _balanced(alpha, gamma)
    tensor(g, "g", torch.float32, (2,))
    tensor(avg, "avg", torch.float32, (1,))
    on_device(named + [("g", g), ("avg", avg)])
    dcls = torch.empty(R, C, dtype=cls_score.dtype, device=cls_score.device)
    dreg = torch.empty(R, cols, dtype=cls_score.dtype, device=cls_score.device)
    _lib.check(_lib.load().tdn_loss_roi_balanced_bwd(_ptr(cls_score), _ptr(bbox_pred), CODES[cls_score.dtype], R, C, cols,
                                                     _ptr(labels), _ptr(label_weights), _ptr(bbox_targets),
                                                     _ptr(bbox_weights), beta, alpha, gamma, _ptr(g), _ptr(avg),
                                                     _ptr(dcls), _ptr(dreg), _lib.stream_ptr()),
               "tdn_loss_roi_balanced_bwd")
    return dcls, dreg


# ---- IoU-balanced negative sampling (csrc/target.hip) -------------------------------------------------------------------
def _balanced_cfg(floor_thr, floor_fraction, num_bins):
    bal = _lib.BalancedConfig()
    bal.floor_thr = number(floor_thr, "floor_thr")
    bal.floor_fraction = number(floor_fraction, "floor_fraction")
    bal.num_bins = integer(num_bins, "num_bins", 1, 8)
    if not 0.0 <= bal.floor_fraction <= 1.0:
        raise ValueError("floor_fraction must be in [0, 1], got %r" % (floor_fraction,))
    if not bal.floor_thr < 1.0:
        raise ValueError("floor_thr must be below 1, got %r" % (floor_thr,))
    return bal


def sample_assigned_iou_balanced(assigned_gt_inds, max_overlaps, num, pos_fraction, neg_pos_ub, floor_thr, floor_fraction,
                                 num_bins, keys, seed):
    """``target_ops.sample_assigned`` with the negatives chosen by IoU-balanced sampling from
    ``assign_max_iou``'s two outputs: -> (pos_mask, neg_mask (B, N) uint8, num_pos, num_neg (B,) int32); one launch."""
    B, N = tensor(assigned_gt_inds, "assigned_gt_inds", torch.int32, ("B", "N"))
    _t.batch(B)
    if N > _lib.TARGET_MAX_BOXES:
        raise ValueError("%d boxes per image (max %d)" % (N, _lib.TARGET_MAX_BOXES))
    tensor(max_overlaps, "max_overlaps", torch.float32, (B, N))
    _t._keys(keys, (B, N))
    cfg = _lib.TargetConfig()
    _t._sampling(cfg, num, pos_fraction, neg_pos_ub, seed)
    bal = _balanced_cfg(floor_thr, floor_fraction, num_bins)
    on_device([("assigned_gt_inds", assigned_gt_inds), ("max_overlaps", max_overlaps), ("keys", keys)])
    dev = assigned_gt_inds.device
    pos_mask = torch.empty(B, N, dtype=torch.uint8, device=dev)
    neg_mask = torch.empty(B, N, dtype=torch.uint8, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().tdn_sample_assigned_balanced(_ptr(assigned_gt_inds), _ptr(max_overlaps), B, N,
                                                        ctypes.byref(cfg), ctypes.byref(bal), _ptr(keys), _ptr(pos_mask),
                                                        _ptr(neg_mask), _ptr(num_pos), _ptr(num_neg), _lib.stream_ptr()),
               "tdn_sample_assigned_balanced")
    return pos_mask, neg_mask, num_pos, num_neg


def sample_rois_iou_balanced(proposals, counts, gt_bboxes, gt_labels, gt_counts, pos_iou_thr, neg_iou_thr, min_pos_iou,
                             gt_max_assign_all, num, pos_fraction, neg_pos_ub, add_gt_as_proposals, means, stds, keys,
                             seed, floor_thr, floor_fraction, num_bins):
    """``target_ops.sample_rois`` with the negatives chosen by IoU-balanced sampling: the same outputs, the same number
    of launches; the workspace also holds the candidates' ``max_overlaps``."""
    B, G = _t._gt(gt_bboxes, gt_counts)
    P = tensor(proposals, "proposals", torch.float32, (B, "P", 5))[1]
    if P > _lib.TARGET_MAX_BOXES - _lib.TARGET_MAX_GT:
        raise ValueError("%d proposals per image (max %d)" % (P, _lib.TARGET_MAX_BOXES - _lib.TARGET_MAX_GT))
    tensor(counts, "counts", torch.int32, (B,))
    tensor(gt_labels, "gt_labels", torch.int64, (B, G))
    cfg = _lib.TargetConfig()
    _t._thresholds(cfg, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all)
    num = _t._sampling(cfg, num, pos_fraction, neg_pos_ub, seed)
    cfg.means, cfg.stds = _t.f4(means, "target_means"), _t.f4(stds, "target_stds")
    cfg.add_gt_as_proposals = 1 if add_gt_as_proposals else 0
    cfg.allowed_border = -1
    bal = _balanced_cfg(floor_thr, floor_fraction, num_bins)
    _t._keys(keys, (B, P + (G if add_gt_as_proposals else 0)))
    on_device([("proposals", proposals), ("counts", counts), ("gt_bboxes", gt_bboxes), ("gt_labels", gt_labels),
               ("gt_counts", gt_counts), ("keys", keys)])
    dev = proposals.device
    lib = _lib.load()
    nbytes = _lib.ws_bytes(lib.tdn_sample_rois_balanced_workspace_bytes(B, P, G, cfg.add_gt_as_proposals), "sample_rois")
    rois = torch.empty(B * num, 5, dtype=torch.float32, device=dev)
    labels = torch.empty(B * num, dtype=torch.int64, device=dev)
    label_weights = torch.empty(B * num, dtype=torch.float32, device=dev)
    bbox_targets = torch.empty(B * num, 4, dtype=torch.float32, device=dev)
    bbox_weights = torch.empty(B * num, 4, dtype=torch.float32, device=dev)
    pos_gt_inds = torch.empty(B * num, dtype=torch.int32, device=dev)
    num_pos = torch.empty(B, dtype=torch.int32, device=dev)
    num_neg = torch.empty(B, dtype=torch.int32, device=dev)
    ws, wp = _aligned_ws(nbytes, dev)
    _lib.check(lib.tdn_sample_rois_balanced(_ptr(proposals), _ptr(counts), _ptr(gt_bboxes), _ptr(gt_labels),
                                            _ptr(gt_counts), B, P, G, ctypes.byref(cfg), ctypes.byref(bal), _ptr(keys),
                                            _ptr(rois), _ptr(labels), _ptr(label_weights), _ptr(bbox_targets),
                                            _ptr(bbox_weights), _ptr(pos_gt_inds), _ptr(num_pos), _ptr(num_neg), wp, nbytes,
                                            _lib.stream_ptr()), "tdn_sample_rois_balanced")
    return rois, labels, label_weights, bbox_targets, bbox_weights, pos_gt_inds, num_pos, num_neg
