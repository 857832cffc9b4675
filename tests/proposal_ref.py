"""NumPy restatement of the box-delta and RPN-proposal spec — the CPU oracle of
torch_detection_amd.box.{bbox2delta, delta2bbox, batched_nms, rpn_proposals}.

fp32 arithmetic in the spec's operation order (every numpy float32 operation rounds once, like the kernels'
__f*_rn); exp / log are evaluated in float64 and rounded to fp32.  NMS is oracle.box_ref.nms (the C oracle of
Appendix B); normalisation is oracle.box_ref.np_bbox_normalize / np_bbox_denormalize, which tests/golden/bbox_norm.npz
pins to the reference's bbox_normalize / bbox_denormalize.
"""
import numpy as np

from oracle import box_ref as B

f32 = np.float32
HALF, ONE = f32(0.5), f32(1.0)


def _exp(x):
    return np.exp(np.asarray(x, dtype=np.float64)).astype(f32)


def _log(x):
    return np.log(np.asarray(x, dtype=np.float64)).astype(f32)


def max_ratio(wh_ratio_clip=16 / 1000):
    """|log(wh_ratio_clip)| in double, rounded to fp32 (16/1000 -> 4.1351666)."""
    return f32(abs(np.log(wh_ratio_clip)))


def bbox2delta(proposals, gt, means=(0, 0, 0, 0), stds=(1, 1, 1, 1)):
    p = np.asarray(proposals, dtype=f32).reshape(-1, 4)
    g = np.asarray(gt, dtype=f32).reshape(-1, 4)
    px, py = (p[:, 0] + p[:, 2]) * HALF, (p[:, 1] + p[:, 3]) * HALF
    pw, ph = (p[:, 2] - p[:, 0]) + ONE, (p[:, 3] - p[:, 1]) + ONE
    gx, gy = (g[:, 0] + g[:, 2]) * HALF, (g[:, 1] + g[:, 3]) * HALF
    gw, gh = (g[:, 2] - g[:, 0]) + ONE, (g[:, 3] - g[:, 1]) + ONE
    d = np.stack([(gx - px) / pw, (gy - py) / ph, _log(gw / pw), _log(gh / ph)], axis=-1)
    return B.np_bbox_normalize(d, means, stds)


def delta2bbox(rois, deltas, means=(0, 0, 0, 0), stds=(1, 1, 1, 1), max_shape=None, wh_ratio_clip=16 / 1000):
    r = np.asarray(rois, dtype=f32).reshape(-1, 4)
    n = r.shape[0]
    d = B.np_bbox_denormalize(np.asarray(deltas, dtype=f32).reshape(n, -1), means, stds).reshape(n, -1, 4)
    mr = max_ratio(wh_ratio_clip)
    dw = np.minimum(np.maximum(d[..., 2], -mr), mr)
    dh = np.minimum(np.maximum(d[..., 3], -mr), mr)
    px, py = ((r[:, 0] + r[:, 2]) * HALF)[:, None], ((r[:, 1] + r[:, 3]) * HALF)[:, None]
    pw, ph = ((r[:, 2] - r[:, 0]) + ONE)[:, None], ((r[:, 3] - r[:, 1]) + ONE)[:, None]
    gw, gh = pw * _exp(dw), ph * _exp(dh)
    gx, gy = px + pw * d[..., 0], py + ph * d[..., 1]
    hw, hh = gw * HALF, gh * HALF
    x1, y1, x2, y2 = (gx - hw) + HALF, (gy - hh) + HALF, (gx + hw) - HALF, (gy + hh) - HALF
    if max_shape is not None:
        xm, ym = f32(int(max_shape[1]) - 1), f32(int(max_shape[0]) - 1)
        x1, x2 = np.minimum(np.maximum(x1, f32(0)), xm), np.minimum(np.maximum(x2, f32(0)), xm)
        y1, y2 = np.minimum(np.maximum(y1, f32(0)), ym), np.minimum(np.maximum(y2, f32(0)), ym)
    return np.stack([x1, y1, x2, y2], axis=-1).reshape(n, -1).astype(f32)


def key_order(logits):
    """Indices by logit descending, ties lower index first (-0.0 == +0.0)."""
    x = np.asarray(logits, dtype=f32)
    return np.lexsort((np.arange(x.shape[0]), -x))


def sigmoid(logits):
    return ONE / (ONE + _exp(-np.asarray(logits, dtype=f32)))


def batched_nms(boxes, scores, seg_offsets, thr):
    """Per-segment oracle.box_ref.nms; outputs laid out like torch_detection_amd.box.batched_nms."""
    n = len(scores)
    keep = np.zeros((n,), np.uint8)
    kept = np.full((n,), -1, np.int64)
    counts = []
    for a, b in zip(seg_offsets[:-1], seg_offsets[1:]):
        k, ki, c = B.nms(boxes[a:b], scores[a:b], thr)
        keep[a:b] = k
        kept[a:a + c] = ki[:c] + a
        counts.append(c)
    return keep, kept, np.asarray(counts, np.int32)


def level_rows(cls_score, bbox_pred):
    """(B, A, H, W) logits and (B, 4A, H, W) deltas -> per image (H*W*A,) logits and (H*W*A, 4) deltas in the anchors'
    (y, x, a) order."""
    c = np.asarray(cls_score, dtype=f32)
    d = np.asarray(bbox_pred, dtype=f32)
    Bn, A, H, W = c.shape
    logits = c.transpose(0, 2, 3, 1).reshape(Bn, H * W * A)
    deltas = d.reshape(Bn, A, 4, H, W).transpose(0, 3, 4, 1, 2).reshape(Bn, H * W * A, 4)
    return logits, deltas


def rpn_proposals(cls_scores, bbox_preds, anchors, img_shapes, nms_pre=2000, nms_post=2000, max_num=2000,
                  nms_thr=0.7, min_bbox_size=0, target_means=(0, 0, 0, 0), target_stds=(1, 1, 1, 1), decode=None):
    """The spec of §4b.  ``decode(rois, deltas, (h, w))`` replaces delta2bbox (e.g. by the GPU's own) when given."""
    if decode is None:
        def decode(r, d, shape):
            return delta2bbox(r, d, target_means, target_stds, shape)
    rows = [level_rows(c, d) for c, d in zip(cls_scores, bbox_preds)]
    Bn = rows[0][0].shape[0]
    props = np.zeros((Bn, max_num, 5), f32)
    aidx = np.full((Bn, max_num), -1, np.int64)
    counts = np.zeros((Bn,), np.int32)
    for b in range(Bn):
        shape = (int(img_shapes[b][0]), int(img_shapes[b][1]))
        c_logit, c_aidx, c_box = [], [], []
        aoff = 0
        for l, (logits, deltas) in enumerate(rows):
            x = logits[b]
            n = x.shape[0]
            order = key_order(x)
            if 0 < nms_pre < n:
                order = order[:nms_pre]
            boxes = np.asarray(decode(np.asarray(anchors[l], f32)[order], deltas[b][order], shape), f32).reshape(-1, 4)
            if min_bbox_size > 0:
                w = (boxes[:, 2] - boxes[:, 0]) + ONE
                h = (boxes[:, 3] - boxes[:, 1]) + ONE
                ok = ~((w < f32(min_bbox_size)) | (h < f32(min_bbox_size)))
                order, boxes = order[ok], boxes[ok]
            m = order.shape[0]
            # rows are in key order already: strictly decreasing stand-in scores keep that order inside the oracle
            _, kept, cnt = B.nms(boxes, np.arange(m, 0, -1).astype(f32), nms_thr)
            kept = kept[:min(cnt, nms_post)]
            c_logit.append(x[order[kept]])
            c_aidx.append(aoff + order[kept].astype(np.int64))
            c_box.append(boxes[kept])
            aoff += n
        lg, ai, bx = np.concatenate(c_logit), np.concatenate(c_aidx), np.concatenate(c_box)
        sel = np.lexsort((ai, -lg))[:max_num]       # (logit desc, level asc, anchor asc) = (logit desc, ai asc)
        k = sel.shape[0]
        props[b, :k, :4] = bx[sel]
        props[b, :k, 4] = sigmoid(lg[sel])
        aidx[b, :k] = ai[sel]
        counts[b] = k
    return props, aidx, counts
