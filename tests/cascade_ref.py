"""NumPy restatement of the Cascade R-CNN spec — the CPU oracle of
torch_detection_amd.cascade.{refine_bboxes, cascade_detections}, written from the specification.

The decode is proposal_ref.delta2bbox (§4b), softmax / NMS / top-k are detect_ref's (§4f), the image of a row is
detect_ref.roi_images.  fp32 arithmetic in the spec's order: every numpy float32 operation rounds once.

The one operation the kernels do not share with NumPy bit for bit is ``expf``: proposal_ref evaluates exp in float64 and
rounds, the device calls its own fp32 ``expf`` (§4b bounds the difference, tests/test_gpu_proposals.py).  So both
functions take the transcendental part from outside when asked, like ``proposal_ref.rpn_proposals(decode=...)``:
``decode(boxes (n, 4), deltas (n, 4), (h, w)) -> (n, 4)`` replaces delta2bbox (by the library's own ``delta2bbox``), and
``cascade_select`` runs the selection on given dense scores and boxes.  Everything else — which class's columns a row
reads, the arg-max, which rows are kept, where they go, the counts, the averaged logits — is restated here.
"""
import numpy as np

import detect_ref as D
import proposal_ref as P

f32 = np.float32


def argmax_labels(cls_score):
    """cls_score.argmax(dim=1) over all C columns of the stored values; ties go to the lowest column."""
    return np.argmax(np.asarray(cls_score, dtype=f32), axis=1).astype(np.int64)


def regress(rois, bbox_pred, img_shapes, labels, target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2),
            wh_ratio_clip=16 / 1000, decode=None):
    """-> (image of every row or -1, new boxes (R, 4) f32 with zeros on the rows that take no part).  A row takes no
    part if it is padding or, with (R, 4C) deltas, its label is outside [0, C)."""
    rois = np.asarray(rois, dtype=f32).reshape(-1, 5)
    d = np.asarray(bbox_pred, dtype=f32)
    labels = np.asarray(labels, dtype=np.int64)
    R = rois.shape[0]
    img = D.roi_images(rois, len(img_shapes))
    if d.shape[1] != 4:
        C = d.shape[1] // 4
        img = np.where((labels >= 0) & (labels < C), img, -1)
        col = 4 * np.clip(labels, 0, C - 1)[:, None] + np.arange(4)[None, :]
        d = np.take_along_axis(d, col, axis=1)
    if decode is None:
        def decode(r, dd, shape):
            return P.delta2bbox(r, dd, target_means, target_stds, shape, wh_ratio_clip)
    boxes = np.zeros((R, 4), f32)
    for b in range(len(img_shapes)):
        m = img == b
        if m.any():
            boxes[m] = decode(rois[m, 1:], d[m], (int(img_shapes[b][0]), int(img_shapes[b][1])))
    return img, boxes


def refine_bboxes(rois, bbox_pred, img_shapes, labels=None, cls_score=None, pos_assigned_gt_inds=None, gt_bboxes=None,
                  max_per_img=None, target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2), wh_ratio_clip=16 / 1000,
                  decode=None):
    """Row-aligned (max_per_img None): rois_out (R, 5) f32.  Compacted: (proposals (B, P, 5) f32, counts (B,) i32)."""
    assert (labels is None) != (cls_score is None)
    if labels is None:
        labels = argmax_labels(cls_score)
    rois = np.asarray(rois, dtype=f32).reshape(-1, 5)
    img, boxes = regress(rois, bbox_pred, img_shapes, labels, target_means, target_stds, wh_ratio_clip, decode)
    R, Bn = rois.shape[0], len(img_shapes)
    if max_per_img is None:
        out = np.zeros((R, 5), f32)
        out[:, 0] = np.where(img >= 0, img, -1).astype(f32)
        out[:, 1:] = boxes
        return out
    keep = img >= 0
    if pos_assigned_gt_inds is not None:
        gi = np.asarray(pos_assigned_gt_inds, dtype=np.int64)
        gt = np.asarray(gt_bboxes, dtype=f32)
        for r in np.nonzero(keep & (gi >= 0) & (gi < gt.shape[1]))[0]:
            if np.array_equal(rois[r, 1:].view(np.uint32), gt[img[r], gi[r]].view(np.uint32)):
                keep[r] = False
    props = np.zeros((Bn, max_per_img, 5), f32)
    counts = np.zeros((Bn,), np.int32)
    for b in range(Bn):
        rows = np.nonzero(keep & (img == b))[0][:max_per_img]          # ascending input rows
        props[b, :rows.shape[0], :4] = boxes[rows]
        counts[b] = rows.shape[0]
    return props, counts


def average_logits(cls_scores):
    """(((x_0 + x_1) + ...) + x_{S-1}) / float(S) in fp32 on the stored values."""
    acc = np.asarray(cls_scores[0], dtype=f32).copy()
    for x in cls_scores[1:]:
        acc = acc + np.asarray(x, dtype=f32)
    return (acc / f32(len(cls_scores))).astype(f32)


def cascade_detections(rois, cls_scores, bbox_pred, img_shapes, scale_factors=None, score_thr=0.05, nms_thr=0.5,
                       max_per_img=100, target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2),
                       wh_ratio_clip=16 / 1000, stats=None):
    """detect_ref.bbox_head_detections on the averaged logits -> (dets, labels, row_idx, counts, scores, boxes)."""
    return D.bbox_head_detections(rois, average_logits(cls_scores), np.asarray(bbox_pred, dtype=f32), img_shapes,
                                  scale_factors, score_thr, nms_thr, max_per_img, target_means, target_stds,
                                  wh_ratio_clip, stats)


def cascade_select(rois, scores, boxes, num_imgs, score_thr=0.05, nms_thr=0.5, max_per_img=100, stats=None):
    """The selection of cascade_detections on given dense (R, C) scores and (R, 4C' or 4) boxes."""
    return D.multiclass_nms(boxes, scores, D.roi_images(rois, num_imgs), num_imgs, score_thr, nms_thr, max_per_img,
                            stats)
