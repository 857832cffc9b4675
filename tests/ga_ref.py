"""CPU oracle of the Guided Anchoring operations: torch_detection_amd.guided.{ga_loc_target,
ga_shape_target, guided_anchors, ga_loss, ga_rpn_proposals}.

Targets and anchors: numpy float32 in the spec's operation order (every numpy float32 operation rounds once, like the
kernels' __f*_rn); the location targets are painted ground truth after ground truth with slice assignments, as
mmdetection v1 writes them — the kernel's gather form has to agree with that.  The IoU is oracle.box_ref's, the
assignment rule is restated on a given overlap matrix (tests/test_ga_oracle.py pins it to target_ref's), the sampling is
target_ref's, the decode proposal_ref's.

The loss: float64; the location term with loss_ref's focal element, the shape term with torch autograd on mmdetection's
``delta2bbox`` / ``bounded_iou_loss`` formulas, so the ties of ``min`` / ``clamp`` are torch's by construction.  Its
a-priori error bounds come from a first-order rounding analysis of the kernel's own operation sequence (``_Seq``): every
rounded fp32 operation is given a relative perturbation and the bound is u * MARGIN * sum |d out / d perturbation|,
evaluated in float64 by autograd.  Nothing here looks at a GPU result.
"""
import numpy as np
import torch

import loss_ref as R
import proposal_ref as PR
import target_ref as TR
from oracle import box_ref as B

f32 = np.float32
U = 2.0 ** -24
MARGIN = 16.0 / 9.0          # §4e's margin over the operation count, as §4n applies it
K_FOCAL = 16.0               # §4e's constant of the focal element, with its factor D
EXP_COST = 4.0               # expf: two ulp
CLIP = 1e-6


def sizes_n(featmap_sizes):
    return int(sum(h * w for h, w in featmap_sizes))


# ---- location targets -----------------------------------------------------------------------------------------------------
def level_thresholds(anchor_scale, stride0, L):
    m = float(anchor_scale) * stride0
    return [f32(m * m * 2.0 ** (2 * k - 1)) for k in range(1, L)]


def gt_areas(gt):
    gt = np.asarray(gt, f32).reshape(-1, 4)
    return ((gt[:, 2] - gt[:, 0]) + f32(1)) * ((gt[:, 3] - gt[:, 1]) + f32(1))


def gt_levels(gt, anchor_scale, stride0, L):
    """#{k in 1..L-1 : area >= t_k}."""
    area = gt_areas(gt)
    lv = np.zeros(area.shape, np.int64)
    for t in level_thresholds(anchor_scale, stride0, L):
        lv += area >= t
    return lv


def gt_levels_log2(gt, anchor_scale, stride0, L):
    """mmdetection's formula in float64: floor(log2(sqrt(w h)) - log2(m) + 0.5), clamped."""
    gt = np.asarray(gt, np.float64).reshape(-1, 4)
    scale = np.sqrt((gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1))
    lv = np.floor(np.log2(scale) - np.log2(float(anchor_scale) * stride0) + 0.5)
    return np.clip(lv, 0, L - 1).astype(np.int64)


def ratio_pair(ratio):
    r = (1.0 - float(ratio)) / 2.0
    return f32(r), f32(1.0 - r)


def calc_region(g, pair, H, W):
    """(x1, y1, x2, y2) as ints: the region of ratio pair (r, c) of the fp32 box g on an H x W map."""
    r, c = pair
    g = np.asarray(g, f32)
    x1, y1 = np.rint(c * g[0] + r * g[2]), np.rint(c * g[1] + r * g[3])
    x2, y2 = np.rint(r * g[0] + c * g[2]), np.rint(r * g[1] + c * g[3])
    xm, ym = f32(W - 1), f32(H - 1)
    cl = lambda v, m: int(np.minimum(np.maximum(v, f32(0)), m))
    return cl(x1, xm), cl(y1, ym), cl(x2, xm), cl(y2, ym)


def loc_target(featmap_sizes, strides, anchor_scale, gt_bboxes, gt_counts, center_ratio=0.2, ignore_ratio=0.5,
               info=None):
    """-> (loc_targets (B, N) int64, loc_weights (B, N) float32, loc_avg_factor)."""
    gt = np.asarray(gt_bboxes, f32)
    Bn, L = gt.shape[0], len(featmap_sizes)
    pc, pi = ratio_pair(center_ratio), ratio_pair(ignore_ratio)
    tg, wt = [], []
    for b in range(Bn):
        t = [np.zeros((h, w), np.int64) for h, w in featmap_sizes]
        wgt = [np.full((h, w), f32(-1)) for h, w in featmap_sizes]
        ig = [np.zeros((h, w), np.int64) for h, w in featmap_sizes]
        boxes = gt[b, :int(gt_counts[b])]
        lv = gt_levels(boxes, anchor_scale, strides[0], L)
        for j in range(boxes.shape[0]):
            l = int(lv[j])
            H, W = featmap_sizes[l]
            g = boxes[j] / f32(strides[l])
            ix1, iy1, ix2, iy2 = calc_region(g, pi, H, W)
            cx1, cy1, cx2, cy2 = calc_region(g, pc, H, W)
            if info is not None:
                info["one_pixel"] = info.get("one_pixel", 0) + int(cx1 == cx2 and cy1 == cy2)
                info.setdefault("levels", set()).add(l)
                info["clamped"] = info.get("clamped", 0) + int(ix1 == 0 or iy1 == 0 or ix2 == W - 1 or iy2 == H - 1)
            t[l][cy1:cy2 + 1, cx1:cx2 + 1] = 1
            wgt[l][iy1:iy2 + 1, ix1:ix2 + 1] = 0
            wgt[l][cy1:cy2 + 1, cx1:cx2 + 1] = 1
            for d in (l - 1, l + 1):
                if 0 <= d < L:
                    Hd, Wd = featmap_sizes[d]
                    x1, y1, x2, y2 = calc_region(boxes[j] / f32(strides[d]), pi, Hd, Wd)
                    ig[d][y1:y2 + 1, x1:x2 + 1] = 1
        for l in range(L):
            wgt[l][(wgt[l] < 0) & (ig[l] > 0)] = 0
            wgt[l][wgt[l] < 0] = f32(0.1)
        tg.append(np.concatenate([v.reshape(-1) for v in t]))
        wt.append(np.concatenate([v.reshape(-1) for v in wgt]))
    tg, wt = np.stack(tg), np.stack(wt).astype(f32)
    if info is not None:
        info["erased_final"] = int(((tg == 1) & (wt == 0)).sum())
    return tg, wt, Bn * sizes_n(featmap_sizes) / 200.0


# ---- shape targets --------------------------------------------------------------------------------------------------------
def approx_overlaps(approxs, gts):
    """(N, G) float32: max over a of IoU(approxs[i, a], gt[j]); the lowest a wins nothing: only the value counts."""
    approxs = np.asarray(approxs, f32)
    ov = B.iou_pairwise(np.ascontiguousarray(approxs[:, 0]), gts)
    for a in range(1, approxs.shape[1]):
        u = B.iou_pairwise(np.ascontiguousarray(approxs[:, a]), gts)
        ov = np.where(u > ov, u, ov)
    return ov


def assign_overlaps(iou_all, part, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, gt_max_assign_all=True, info=None):
    """target_ref.assign_image's steps on a given (N, G) overlap matrix; rows off ``part`` do not take part."""
    n, G = iou_all.shape
    assigned = np.full((n,), -1, np.int32)
    max_ov = np.zeros((n,), f32)
    idx = np.nonzero(part)[0]
    if G == 0:
        assigned[idx] = 0
        return assigned, max_ov
    if idx.shape[0] == 0:
        return assigned, max_ov
    iou = iou_all[idx]
    mx, am = iou.max(axis=1), iou.argmax(axis=1)
    a = np.full((idx.shape[0],), -1, np.int32)
    a[(mx >= f32(0)) & (mx < f32(neg_iou_thr))] = 0
    a[mx >= f32(pos_iou_thr)] = am[mx >= f32(pos_iou_thr)] + 1
    before = a.copy()
    gmax = iou.max(axis=0)
    touched = np.zeros_like(a)
    for j in range(G):
        if gmax[j] >= f32(min_pos_iou):
            hit = np.nonzero(iou[:, j] == gmax[j])[0]
            if info is not None:
                info["col_ties"] = info.get("col_ties", 0) + int(hit.shape[0] > 1)
            if not gt_max_assign_all:
                hit = hit[:1]
            a[hit] = j + 1
            touched[hit] += 1
    if info is not None:
        info["only_step6"] = info.get("only_step6", 0) + int(((before <= 0) & (a > 0)).sum())
        info["step6_ties"] = info.get("step6_ties", 0) + int((touched > 1).sum())
    assigned[idx] = a
    max_ov[idx] = mx
    return assigned, max_ov


def shape_target(approxs, squares, valid_flags, gt_bboxes, gt_counts, img_shapes, pos_iou_thr=0.7, neg_iou_thr=0.3,
                 min_pos_iou=0.3, num=256, pos_fraction=0.5, neg_pos_ub=-1, allowed_border=0, keys=None, seed=0,
                 gt_max_assign_all=True, sampling=True, info=None):
    approxs = np.asarray(approxs, f32)
    squares = np.asarray(squares, f32)
    gt = np.asarray(gt_bboxes, f32)
    N, A, _ = approxs.shape
    Bn = gt.shape[0]
    flat = approxs.reshape(N * A, 4)
    assigned, max_ov = [], []
    for b in range(Bn):
        ok = np.ones((N * A,), bool)
        if valid_flags is not None:
            v = np.asarray(valid_flags)
            ok &= (v if v.ndim == 1 else v[b]) != 0
        if allowed_border >= 0:
            ok &= TR.inside_border(flat, img_shapes[b], allowed_border)
        okl = ok.reshape(N, A)
        part = okl.any(axis=1)
        if info is not None:
            info["single"] = info.get("single", 0) + int((okl.sum(axis=1) == 1).sum())
            if valid_flags is not None and allowed_border >= 0:      # every flag set, a single approx inside the image
                v = np.asarray(valid_flags)
                allset = ((v if v.ndim == 1 else v[b]) != 0).reshape(N, A).all(axis=1)
                info["single_inside"] = info.get("single_inside", 0) + int((allset & (okl.sum(axis=1) == 1)).sum())
            info["out"] = info.get("out", 0) + int((~part).sum())
        gts = gt[b, :int(gt_counts[b])]
        ov = approx_overlaps(approxs, gts) if gts.shape[0] else np.zeros((N, 0), f32)
        if info is not None and gts.shape[0] and A > 1:
            per = np.stack([B.iou_pairwise(np.ascontiguousarray(approxs[:, a]), gts) for a in range(A)])
            info["approx_ties"] = info.get("approx_ties", 0) + int((((per == ov[None]) & (ov[None] > 0)).sum(0) > 1).sum())
        a, m = assign_overlaps(ov, part, pos_iou_thr, neg_iou_thr, min_pos_iou, gt_max_assign_all, info)
        assigned.append(a)
        max_ov.append(m)
    assigned, max_ov = np.stack(assigned), np.stack(max_ov)
    if sampling:
        pm, nm, num_pos, num_neg = TR.sample_assigned(assigned, num, pos_fraction, neg_pos_ub, keys, seed)
        if info is not None:
            info["cut"] = info.get("cut", 0) + int((num_pos < (assigned > 0).sum(1)).sum() +
                                                   (num_neg < (assigned == 0).sum(1)).sum())
    else:
        pm, nm = (assigned > 0).astype(np.uint8), (assigned == 0).astype(np.uint8)
        num_pos, num_neg = pm.sum(1).astype(np.int32), nm.sum(1).astype(np.int32)
    an, gs, w = np.zeros((Bn, N, 4), f32), np.zeros((Bn, N, 4), f32), np.zeros((Bn, N, 4), f32)
    for b in range(Bn):
        ip = np.nonzero(pm[b])[0]
        an[b, ip] = squares[ip]
        gs[b, ip] = gt[b, assigned[b, ip] - 1]
        w[b, ip] = 1
    return an, gs, w, num_pos, num_neg, assigned, max_ov


# ---- guided anchors -------------------------------------------------------------------------------------------------------
def rows(t):
    """(B, Ch, H, W) -> (B, H*W, Ch), location h*W + w."""
    t = np.asarray(t)
    Bn, Ch, H, W = t.shape
    return t.reshape(Bn, Ch, H * W).transpose(0, 2, 1)


def unrows(y, H, W):
    Bn, _, Ch = y.shape
    return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(Bn, Ch, H, W)


def loc_threshold(thr):
    return f32(np.log(float(thr) / (1.0 - float(thr))))


def guided_anchors(shape_preds, squares, loc_preds=None, loc_filter_thr=None, means=(0, 0, 0, 0),
                   stds=(0.07, 0.07, 0.14, 0.14)):
    """Stored head values as float32 arrays -> (anchors (B, N, 4) float32, loc_mask (B, N) uint8, tol (B, N, 4): §4b's
    decode bound 4 spacing(max(|gx|, gw, 1)) per axis)."""
    sq = np.asarray(squares, f32)
    s = np.concatenate([rows(np.asarray(p, f32)) for p in shape_preds], 1)                 # (B, N, 2)
    Bn, N, _ = s.shape
    d = np.concatenate([np.zeros((Bn, N, 2), f32), s], 2)
    anchors = np.stack([PR.delta2bbox(sq, d[b], means, stds, None, CLIP) for b in range(Bn)])
    mr = float(PR.max_ratio(CLIP))
    tol = np.empty((Bn, N, 4), f32)
    for ax in (0, 1):
        pw = ((sq[:, 2 + ax] - sq[:, ax]) + 1).astype(np.float64)[None]
        dd = np.clip(s[..., ax].astype(np.float64) * float(f32(stds[2 + ax])) + float(f32(means[2 + ax])), -mr, mr)
        gw = pw * np.exp(dd)
        gx = np.abs((sq[:, ax] + sq[:, 2 + ax]).astype(np.float64)[None] * 0.5 + pw * float(f32(means[ax])))
        t = 4 * np.spacing(np.maximum(np.maximum(gx, gw), 1.0).astype(f32))
        tol[..., ax], tol[..., 2 + ax] = t, t
    if loc_preds is None:
        return anchors, np.ones((Bn, N), np.uint8), tol
    z = np.concatenate([rows(np.asarray(p, f32)) for p in loc_preds], 1)[..., 0]
    return anchors, (z >= loc_threshold(loc_filter_thr)).astype(np.uint8), tol


# ---- guided RPN proposals -------------------------------------------------------------------------------------------------
def rpn_proposals(cls_scores, bbox_preds, anchors, loc_mask, img_shapes, nms_pre=2000, nms_post=2000, max_num=2000,
                  nms_thr=0.7, min_bbox_size=0, target_means=(0, 0, 0, 0), target_stds=(1, 1, 1, 1), decode=None,
                  info=None):
    """proposal_ref.rpn_proposals (§4b) with one anchor per location, ``anchors`` (B, N, 4) of each image and
    ``loc_mask`` (B, N): a level's candidates are its locations that are in.  ``decode(rois, deltas, (h, w))`` replaces
    delta2bbox (e.g. by the GPU's own) when given."""
    if decode is None:
        def decode(r, d, shape):
            return PR.delta2bbox(r, d, target_means, target_stds, shape)
    rows_ = [PR.level_rows(c, d) for c, d in zip(cls_scores, bbox_preds)]
    anchors, loc_mask = np.asarray(anchors, f32), np.asarray(loc_mask)
    Bn = rows_[0][0].shape[0]
    props = np.zeros((Bn, max_num, 5), f32)
    aidx = np.full((Bn, max_num), -1, np.int64)
    counts = np.zeros((Bn,), np.int32)
    for b in range(Bn):
        shape = (int(img_shapes[b][0]), int(img_shapes[b][1]))
        c_logit, c_aidx, c_box = [np.zeros(0, f32)], [np.zeros(0, np.int64)], [np.zeros((0, 4), f32)]
        aoff = 0
        for logits, deltas in rows_:
            x = logits[b]
            n = x.shape[0]
            inside = np.nonzero(loc_mask[b, aoff:aoff + n] != 0)[0]
            order = inside[PR.key_order(x[inside])]              # ties: the lower location first
            if info is not None:
                info["empty_levels"] = info.get("empty_levels", 0) + int(inside.shape[0] == 0)
                info["cut_levels"] = info.get("cut_levels", 0) + int(0 < nms_pre < inside.shape[0])
                info["short_levels"] = info.get("short_levels", 0) + int(0 < inside.shape[0] < min(n, nms_pre or n))
            if 0 < nms_pre < order.shape[0]:
                order = order[:nms_pre]
            if order.shape[0] == 0:                              # nothing of this level is in
                aoff += n
                continue
            boxes = np.asarray(decode(anchors[b, aoff + order], deltas[b][order], shape), f32).reshape(-1, 4)
            if min_bbox_size > 0:
                w = (boxes[:, 2] - boxes[:, 0]) + PR.ONE
                h = (boxes[:, 3] - boxes[:, 1]) + PR.ONE
                ok = ~((w < f32(min_bbox_size)) | (h < f32(min_bbox_size)))
                order, boxes = order[ok], boxes[ok]
            m = order.shape[0]
            _, kept, cnt = B.nms(boxes, np.arange(m, 0, -1).astype(f32), nms_thr) if m else (None, np.zeros(0, np.int64), 0)
            kept = kept[:min(cnt, nms_post)]
            c_logit.append(x[order[kept]])
            c_aidx.append(aoff + order[kept].astype(np.int64))
            c_box.append(boxes[kept])
            aoff += n
        lg, ai, bx = np.concatenate(c_logit), np.concatenate(c_aidx), np.concatenate(c_box)
        sel = np.lexsort((ai, -lg))[:max_num]
        k = sel.shape[0]
        props[b, :k, :4] = bx[sel]
        props[b, :k, 4] = PR.sigmoid(lg[sel])
        aidx[b, :k] = ai[sel]
        counts[b] = k
    return props, aidx, counts


# ---- loss -----------------------------------------------------------------------------------------------------------------
def delta2bbox_t(rois, deltas, means, stds, max_ratio):
    """mmdetection v1's delta2bbox without max_shape, torch float64."""
    d = deltas * stds + means
    dx, dy = d[:, 0], d[:, 1]
    dw, dh = d[:, 2].clamp(min=-max_ratio, max=max_ratio), d[:, 3].clamp(min=-max_ratio, max=max_ratio)
    px, py = (rois[:, 0] + rois[:, 2]) * 0.5, (rois[:, 1] + rois[:, 3]) * 0.5
    pw, ph = rois[:, 2] - rois[:, 0] + 1.0, rois[:, 3] - rois[:, 1] + 1.0
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = torch.addcmul(px, pw, dx), torch.addcmul(py, ph, dy)
    return torch.stack([gx - gw * 0.5 + 0.5, gy - gh * 0.5 + 0.5, gx + gw * 0.5 - 0.5, gy + gh * 0.5 - 0.5], -1)


def bounded_iou_t(pred, target, beta, eps, raw=False):
    """mmdetection v1's bounded_iou_loss per element (P, 4), torch float64; ``raw``: the terms before the smooth-L1
    shaping instead."""
    pcx, pcy = (pred[:, 0] + pred[:, 2]) * 0.5, (pred[:, 1] + pred[:, 3]) * 0.5
    pw, ph = pred[:, 2] - pred[:, 0] + 1, pred[:, 3] - pred[:, 1] + 1
    with torch.no_grad():
        tcx, tcy = (target[:, 0] + target[:, 2]) * 0.5, (target[:, 1] + target[:, 3]) * 0.5
        tw, th = target[:, 2] - target[:, 0] + 1, target[:, 3] - target[:, 1] + 1
    dx, dy = tcx - pcx, tcy - pcy
    ldx = 1 - torch.max((tw - 2 * dx.abs()) / (tw + 2 * dx.abs() + eps), torch.zeros_like(dx))
    ldy = 1 - torch.max((th - 2 * dy.abs()) / (th + 2 * dy.abs() + eps), torch.zeros_like(dy))
    ldw = 1 - torch.min(tw / (pw + eps), pw / (tw + eps))
    ldh = 1 - torch.min(th / (ph + eps), ph / (th + eps))
    comb = torch.stack([ldx, ldy, ldw, ldh], -1)
    if raw:
        return comb
    return torch.where(comb < beta, 0.5 * comb * comb / beta, comb - 0.5 * beta)


class _Seq(object):
    """The rounded operations of a computation: ``r(v)`` marks v as the result of one rounded fp32 operation."""

    def __init__(self):
        self.eps, self.cost = [], []

    def r(self, v, cost=1.0):
        e = torch.zeros_like(v, requires_grad=True)
        self.eps.append(e)
        self.cost.append(cost)
        return v * (1 + e)

    def bound(self, out):
        """u * MARGIN * sum over the operations of cost |d out / d eps|, per row."""
        grads = torch.autograd.grad(out.sum(), self.eps, allow_unused=True)
        tot = torch.zeros_like(out)
        for c, g in zip(self.cost, grads):
            if g is not None:
                tot = tot + c * g.abs()
        return (U * MARGIN * tot).detach().numpy()


def _knee(q, l, beta, grad):
    if grad:
        return torch.where(l < beta, q.r(l / beta), torch.ones_like(l))
    return torch.where(l < beta, q.r(q.r(0.5 * l * l) / beta), q.r(l - 0.5 * beta))


def _axis_kernel(q, a0, a1, g0, g1, d, mean_c, mean, std, max_ratio, w_c, w_s, beta, eps, grad):
    """The kernel's operation sequence for one axis (csrc/guided.hip: decode_box, ga_axis), every rounded operation
    marked; -> the weighted loss of the axis, or with ``grad`` its derivative with respect to d."""
    r = q.r
    ds = r(r(d * std) + mean)
    dcl = ds.clamp(min=-max_ratio, max=max_ratio)
    pc, ps = r(a0 + a1) * 0.5, r(r(a1 - a0) + 1.0)
    gs = r(ps * r(dcl.exp(), EXP_COST))
    gc = r(pc + r(ps * mean_c))
    hs = gs * 0.5
    o0, o1 = r(r(gc - hs) + 0.5), r(r(gc + hs) - 0.5)
    pctr, psz = r(o0 + o1) * 0.5, r(r(o1 - o0) + 1.0)
    tctr, tsz = r(g0 + g1) * 0.5, r(r(g1 - g0) + 1.0)
    pe, te = r(psz + eps), r(tsz + eps)
    ra, rb = r(tsz / pe), r(psz / te)
    ls = r(1 - torch.where(ra.detach() <= rb.detach(), ra, rb))
    if grad:
        da, db = -r(ra / pe), r(1 / te)
        tie = ra.detach() == rb.detach()
        dmin = torch.where(tie, r(da + db) * 0.5, torch.where(ra.detach() < rb.detach(), da, db))
        inr = ((ds.detach() >= -max_ratio) & (ds.detach() <= max_ratio)).to(d.dtype)
        return r(r(r(w_s * _knee(q, ls, beta, True)) * -dmin) * r(gs * std)) * inr
    ad2 = 2 * r(tctr - pctr).abs()
    lc = r(1 - torch.clamp(r(r(tsz - ad2) / r(r(tsz + ad2) + eps)), min=0))
    return r(r(w_c * _knee(q, lc, beta, False)) + r(w_s * _knee(q, ls, beta, False)))


def loss(loc_preds, shape_preds, loc_targets, loc_weights, bbox_anchors, bbox_gts, bbox_weights, loc_avg_factor,
         shape_avg_factor, gamma=2.0, alpha=0.25, beta=0.2, eps=1e-3, means=(0, 0, 0, 0), stds=(0.07, 0.07, 0.14, 0.14),
         g=(1.0, 1.0)):
    """float64 losses and gradients of ``g . losses`` from the stored inputs (head outputs as float arrays holding the
    stored values).  Returns a dict: ``losses`` (2,), ``norm`` (2,), ``dloc`` / ``dshape`` (lists, (B, Ch, H, W)),
    ``bound_losses`` (2,), ``bound_dloc`` / ``bound_dshape`` (lists): the error bounds in absolute terms, margin
    included, WITHOUT the final rounding of the output; ``num_rows``, ``switch_gap`` (the smallest relative distance of
    a row that is not exactly on a tie of ``min`` or an edge of ``clamp`` from one), ``ties``, ``clipped`` (axes beyond the
    clip), ``below_beta`` / ``above_beta`` (4,) (rows whose dx, dy, dw, dh term lies below / not below the knee) and
    ``centre_clamped`` (centre terms whose ``max(., 0)`` took the 0)."""
    sizes = [np.asarray(p).shape[2:] for p in shape_preds]
    x = np.concatenate([rows(np.asarray(p, np.float64)) for p in loc_preds], 1)[..., 0]        # (B, N)
    s = np.concatenate([rows(np.asarray(p, np.float64)) for p in shape_preds], 1)              # (B, N, 2)
    Bn, N = x.shape
    w = np.asarray(loc_weights, f32).astype(np.float64)
    t1 = np.asarray(loc_targets) == 1
    g32 = np.asarray(g, f32)
    d_loc, d_shape = f32(loc_avg_factor), R.divisor(shape_avg_factor)
    s_loc, s_shape = float(g32[0] / d_loc), float(g32[1] / d_shape)
    live = w != 0
    with np.errstate(all="ignore"):
        l, dl = R.cls_elem(x, t1, gamma, alpha)
        Df = float(f32(gamma)) * np.maximum(R.sp(x), R.sp(-x)) + 1.0
    l, dl, Df = np.where(live, l, 0.0), np.where(live, dl, 0.0), np.where(live, Df, 0.0)
    loss_loc = float((w * l).sum()) / float(d_loc)
    b_loss_loc = U * float(((K_FOCAL * Df + 2.0) * w * l).sum()) / float(d_loc)
    dloc = w * dl * s_loc
    b_dloc = U * (K_FOCAL + 3.0) * Df * w * abs(s_loc)

    bw = np.asarray(bbox_weights, f32).astype(np.float64)
    bi, ii = np.nonzero(bw[..., 0] > 0)
    P = bi.shape[0]
    T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    mr = float(PR.max_ratio(CLIP))
    m4, s4 = [float(f32(v)) for v in means], [float(f32(v)) for v in stds]
    bt, ep = float(f32(beta)), float(f32(eps))
    an, gt, wr = T(np.asarray(bbox_anchors, f32)[bi, ii]), T(np.asarray(bbox_gts, f32)[bi, ii]), T(bw[bi, ii])
    sp = T(s[bi, ii]).requires_grad_(True)
    pred = delta2bbox_t(an, torch.cat([torch.zeros(P, 2, dtype=torch.float64), sp], 1), T(m4), T(s4), mr)
    tot = (bounded_iou_t(pred, gt, bt, ep) * wr).sum()
    loss_shape = float(tot.detach()) / float(d_shape)
    if P:
        (tot * s_shape).backward()
    dsr = sp.grad.numpy() if P else np.zeros((0, 2))
    terms = bounded_iou_t(pred.detach(), gt, bt, ep, raw=True).numpy()                        # (P, 4): dx, dy, dw, dh
    below, above = (terms < bt).sum(0), (terms >= bt).sum(0)
    centre_clamped = int((terms[:, :2] == 1.0).sum())                                        # max(., 0) took the 0

    # the bounds: the kernel's sequence, perturbed
    b_rows, b_grad, chk_val, chk_grad = np.zeros(P), np.zeros((P, 2)), np.zeros(P), np.zeros((P, 2))
    gap, ties, clipped = np.inf, 0, 0
    spd = sp.detach()
    for ax in (0, 1):
        args = (an[:, ax], an[:, 2 + ax], gt[:, ax], gt[:, 2 + ax], spd[:, ax], m4[ax], m4[2 + ax], s4[2 + ax], mr,
                wr[:, ax], wr[:, 2 + ax], bt, ep)
        if not P:
            break
        q = _Seq()
        v = _axis_kernel(q, *args, False)
        b_rows += q.bound(v)
        chk_val += v.detach().numpy()
        q = _Seq()
        gv = q.r(_axis_kernel(q, *args, True) * s_shape)
        b_grad[:, ax] = q.bound(gv)
        chk_grad[:, ax] = gv.detach().numpy()
        # distances from the switches of the gradient
        with torch.no_grad():
            ds = spd[:, ax] * s4[2 + ax] + m4[2 + ax]
            psz = pred[:, 2 + ax] - pred[:, ax] + 1
            tsz = gt[:, 2 + ax] - gt[:, ax] + 1
            ra, rb = tsz / (psz + ep), psz / (tsz + ep)
            rel = ((ra - rb).abs() / torch.maximum(ra, rb)).numpy()
            ties += int((rel == 0).sum())
            edge = np.minimum(np.abs(ds.numpy() - mr), np.abs(ds.numpy() + mr)) / mr
            clipped += int((np.abs(ds.numpy()) > mr).sum())
            for arr in (rel[rel != 0], edge):
                if arr.size:
                    gap = min(gap, float(arr.min()))
    assert np.allclose(chk_val.sum(), float(tot.detach()), rtol=1e-12, atol=1e-300), (chk_val.sum(), float(tot.detach()))
    assert np.allclose(chk_grad, dsr, rtol=1e-10, atol=1e-14), np.abs(chk_grad - dsr).max()
    b_loss_shape = float(b_rows.sum()) / float(d_shape)
    dshape, b_dshape = np.zeros((Bn, N, 2)), np.zeros((Bn, N, 2))
    dshape[bi, ii], b_dshape[bi, ii] = dsr, b_grad

    out = dict(losses=np.array([loss_loc, loss_shape]), norm=np.array([float(d_loc), float(d_shape)]),
               bound_losses=np.array([b_loss_loc, b_loss_shape]), num_rows=P, switch_gap=gap, ties=ties, clipped=clipped,
               below_beta=below, above_beta=above, centre_clamped=centre_clamped,
               dloc=[], dshape=[], bound_dloc=[], bound_dshape=[])
    n0 = 0
    for H, W in sizes:
        n1 = n0 + H * W
        out["dloc"].append(unrows(dloc[:, n0:n1, None], H, W))
        out["bound_dloc"].append(unrows(b_dloc[:, n0:n1, None], H, W))
        out["dshape"].append(unrows(dshape[:, n0:n1], H, W))
        out["bound_dshape"].append(unrows(b_dshape[:, n0:n1], H, W))
        n0 = n1
    return out
