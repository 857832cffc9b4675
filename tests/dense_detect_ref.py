"""NumPy restatement of the single-stage head spec — the CPU oracle of
torch_detection_amd.dense_detect.{anchor_head_detections, anchor_target_all}.

Built from the oracles of the neighbouring sections: the sigmoid, decode and encode are proposal_ref's (§4b), the
selection is detect_ref.multiclass_nms (§4f), the assignment is target_ref.assign_image / inside_border (§4d).  Head
outputs come as float32 arrays holding the STORED values (a bf16 / fp16 tensor converted exactly).
"""
import numpy as np

import detect_ref as D
import proposal_ref as P
import target_ref as R

f32 = np.float32
SEG_MAX, MAX_LEVELS, MAX_ROWS, MAX_CLASSES = 4096, 8, 1 << 18, 1023


def head_rows(cls_score, bbox_pred, C):
    """(B, A*C, H, W) logits and (B, 4A, H, W) deltas -> (B, H*W*A, C) logits and (B, H*W*A, 4) deltas in the anchors'
    (y, x, a) order."""
    c = np.asarray(cls_score, dtype=f32)
    d = np.asarray(bbox_pred, dtype=f32)
    Bn, AC, H, W = c.shape
    A = AC // C
    logits = c.reshape(Bn, A, C, H, W).transpose(0, 3, 4, 1, 2).reshape(Bn, H * W * A, C)
    deltas = d.reshape(Bn, A, 4, H, W).transpose(0, 3, 4, 1, 2).reshape(Bn, H * W * A, 4)
    return logits, deltas


def kept_anchors(keys, nms_pre, info=None):
    """Step 2 for one (image, level): the anchors kept, ascending.  ``info`` (a dict) receives, for a level that selects,
    the cut key, the anchors strictly above it, the ties at it and the ties taken."""
    n = keys.shape[0]
    if not 0 < nms_pre < n:
        return np.arange(n)
    order = P.key_order(keys)[:nms_pre]                 # (key desc, anchor asc), -0.0 == +0.0
    if info is not None:
        cut = keys[order[-1]]
        above = int((keys > cut).sum())
        info.setdefault("cuts", []).append(dict(cut=float(cut), above=above, ties=int((keys == cut).sum()),
                                                taken=nms_pre - above))
    return np.sort(order)


def plan(level_sizes, nms_pre):
    """k_l, off_l and K of step 2 for levels of ``level_sizes`` anchors."""
    k = [nms_pre if 0 < nms_pre < n else n for n in level_sizes]
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    return k, off[:-1], int(off[-1])


def dense(cls_scores, bbox_preds, anchors, img_shapes, scale_factors=None, nms_pre=1000, target_means=(0, 0, 0, 0),
          target_stds=(1, 1, 1, 1), wh_ratio_clip=16 / 1000, info=None):
    """Steps 1-3.  -> dict: scores (B*K, C+1) f32, boxes (B*K, 4) f32, batch_idx (B*K,) i32, anchor_idx (B*K,) i64, and
    for the error bounds of the GPU tests logits (B*K, C) f32 (the stored x of every score), boxes_unscaled f32, scale
    (B*K,) f32 or None, rois (B*K, 4) and deltas (B*K, 4) of every row."""
    Bn = np.asarray(cls_scores[0]).shape[0]
    A = np.asarray(bbox_preds[0]).shape[1] // 4
    C = np.asarray(cls_scores[0]).shape[1] // A
    if not isinstance(anchors, (list, tuple)):
        sizes = [np.asarray(c).shape[2] * np.asarray(c).shape[3] * A for c in cls_scores]
        cuts = np.cumsum([0] + sizes)
        anchors = [np.asarray(anchors, f32)[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    rows = [head_rows(c, d, C) for c, d in zip(cls_scores, bbox_preds)]
    scale = None
    if scale_factors is not None:
        s = np.asarray(scale_factors, dtype=f32).reshape(-1)
        scale = np.broadcast_to(s, (Bn,)) if s.shape[0] == 1 else s
    out = {k: [] for k in ("logits", "boxes_unscaled", "batch_idx", "anchor_idx", "scale", "rois", "deltas")}
    for b in range(Bn):
        shape = (int(img_shapes[b][0]), int(img_shapes[b][1]))
        aoff = 0
        for l, (logits, deltas) in enumerate(rows):
            x = logits[b]
            keep = kept_anchors(x.max(axis=1), nms_pre, info)
            anc = np.asarray(anchors[l], f32)[keep]
            out["logits"].append(x[keep])
            out["rois"].append(anc)
            out["deltas"].append(deltas[b][keep])
            out["boxes_unscaled"].append(P.delta2bbox(anc, deltas[b][keep], target_means, target_stds, shape,
                                                      wh_ratio_clip).reshape(-1, 4))
            out["batch_idx"].append(np.full((keep.shape[0],), b, np.int32))
            out["anchor_idx"].append(aoff + keep.astype(np.int64))
            out["scale"].append(np.full((keep.shape[0],), 1 if scale is None else scale[b], f32))
            aoff += x.shape[0]
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["scores"] = np.concatenate([np.zeros((out["logits"].shape[0], 1), f32), P.sigmoid(out["logits"])], axis=1)
    out["boxes"] = out["boxes_unscaled"] if scale is None else (out["boxes_unscaled"] / out["scale"][:, None]).astype(f32)
    if scale is None:
        out["scale"] = None
    return out


def select(dense_boxes, dense_scores, batch_idx, dense_anchor_idx, num_imgs, score_thr=0.05, nms_thr=0.5,
           max_per_img=100, stats=None):
    """Steps 4-5 on given dense tensors -> (dets, labels, anchor_idx, counts, row_idx)."""
    dets, labels, rows, counts = D.multiclass_nms(dense_boxes, dense_scores, batch_idx, num_imgs, score_thr, nms_thr,
                                                  max_per_img, stats)
    aidx = np.where(rows >= 0, np.asarray(dense_anchor_idx, np.int64)[np.maximum(rows, 0)], -1)
    return dets, labels, aidx, counts, rows


def anchor_head_detections(cls_scores, bbox_preds, anchors, img_shapes, scale_factors=None, nms_pre=1000,
                           score_thr=0.05, nms_thr=0.5, max_per_img=100, target_means=(0, 0, 0, 0),
                           target_stds=(1, 1, 1, 1), wh_ratio_clip=16 / 1000, info=None, stats=None):
    """The whole spec on the CPU -> (dets, labels, anchor_idx, counts, dense_scores, dense_boxes, batch_idx,
    dense_anchor_idx, row_idx)."""
    d = dense(cls_scores, bbox_preds, anchors, img_shapes, scale_factors, nms_pre, target_means, target_stds,
              wh_ratio_clip, info)
    Bn = np.asarray(cls_scores[0]).shape[0]
    dets, labels, aidx, counts, rows = select(d["boxes"], d["scores"], d["batch_idx"], d["anchor_idx"], Bn, score_thr,
                                              nms_thr, max_per_img, stats)
    return dets, labels, aidx, counts, d["scores"], d["boxes"], d["batch_idx"], d["anchor_idx"], rows


def anchor_target_all(anchors, valid_flags, gt_bboxes, gt_labels, gt_counts, img_shapes, pos_iou_thr=0.5,
                      neg_iou_thr=0.4, min_pos_iou=0.0, allowed_border=-1, target_means=(0, 0, 0, 0),
                      target_stds=(1, 1, 1, 1), gt_max_assign_all=True, info=None):
    """-> (labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, assigned)."""
    gt = np.asarray(gt_bboxes, dtype=f32)
    Bn = gt.shape[0]
    anchors = np.asarray(anchors, dtype=f32)
    n = anchors.shape[-2]
    labels = np.zeros((Bn, n), np.int64)
    label_weights = np.zeros((Bn, n), f32)
    bbox_targets, bbox_weights = np.zeros((Bn, n, 4), f32), np.zeros((Bn, n, 4), f32)
    num_pos, num_neg = np.zeros((Bn,), np.int32), np.zeros((Bn,), np.int32)
    assigned = np.zeros((Bn, n), np.int32)
    for b in range(Bn):
        bx = anchors if anchors.ndim == 2 else anchors[b]
        part = np.ones((n,), bool)
        if valid_flags is not None:
            v = np.asarray(valid_flags)
            part &= (v if v.ndim == 1 else v[b]) != 0
        if allowed_border >= 0:
            part &= R.inside_border(bx, img_shapes[b], allowed_border)
        one = {}
        a = R.assign_image(bx, part, gt[b, :int(gt_counts[b])], pos_iou_thr, neg_iou_thr, min_pos_iou,
                           gt_max_assign_all, one)[0]
        if info is not None:
            info.setdefault("only_step6", []).append(one.get("only_step6", 0))
            info.setdefault("ignored", []).append(int((part & (a < 0)).sum()))
            info.setdefault("outside", []).append(int((~part).sum()))
        assigned[b] = a
        ip = np.nonzero(a > 0)[0]
        labels[b, ip] = 1 if gt_labels is None else np.asarray(gt_labels, np.int64)[b, a[ip] - 1]
        label_weights[b, a >= 0] = 1
        bbox_targets[b, ip] = P.bbox2delta(bx[ip], gt[b, a[ip] - 1], target_means, target_stds)
        bbox_weights[b, ip] = 1
        num_pos[b], num_neg[b] = ip.shape[0], int((a == 0).sum())
    return labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, assigned
