"""NumPy oracle of the Libra R-CNN pieces beside the BFP neck: balanced L1 in the RoI box loss
(csrc/loss.hip, ``bbox_head_loss(reg_loss='balanced_l1')``) and, in the second half of the file, IoU-balanced negative
sampling (csrc/target.hip, ``sample_rois(neg_sampler='iou_balanced')``) with an independent set-based restatement.

Balanced L1, per element, d = pred - target, a = |d|, b = e^(gamma / alpha) - 1:

    a <  beta:  l = (alpha / b) (b a + 1) log(b a / beta + 1) - alpha a
                dl = sign(d) (alpha log(b a / beta + 1) + alpha (1 - beta) / (b a + beta))
    a >= beta:  l = gamma a + gamma / b - alpha beta;                      dl = sign(d) gamma

(dl is the derivative of l: its second term vanishes at beta = 1, the knee Libra R-CNN uses, where dl = sign(d) alpha t)

twice, as tests/loss_ref.py does for smooth L1: in float64 for the values, and in float32 with the kernel's operation order
and its host-formed constants for what must match bit for bit (the outer-branch gradients and every exact zero; the inner
branch goes through ``log1pf``, whose last bit is the library's own).
"""
import numpy as np

import loss_ref as L

F32 = np.float32


def balanced_consts(beta, alpha, gamma):
    """(b, alpha / b, gamma / b - alpha beta, alpha (1 - beta)): formed in double from the float32 parameters, rounded
    once to float32."""
    al, ga, be = float(F32(alpha)), float(F32(gamma)), float(F32(beta))
    b = np.exp(ga / al) - 1.0
    return F32(b), F32(al / b), F32(ga / b - al * be), F32(al * (1.0 - be))


def balanced_l1(pred, target, beta, alpha, gamma):
    """(loss, gradient) in float64 on the float32 difference's exact operands."""
    al, ga, be = float(F32(alpha)), float(F32(gamma)), float(F32(beta))
    b = np.exp(ga / al) - 1.0
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    a = np.abs(d)
    with np.errstate(all="ignore"):
        t = np.log1p(b * a / be)
        inner = al / b * (b * a + 1.0) * t - al * a
        outer = ga * a + ga / b - al * be
        dl = al * t + al * (1.0 - be) / (b * a + be)
        return np.where(a < be, inner, outer), np.where(a < be, np.sign(d) * dl, np.sign(d) * ga)


def balanced_l1_32(pred, target, beta, alpha, gamma):
    """(loss, gradient, outer-branch mask) in float32, operation by operation as the kernel does it."""
    be, al, ga = F32(beta), F32(alpha), F32(gamma)
    b, a_over_b, outer_c, knee_c = balanced_consts(beta, alpha, gamma)
    with np.errstate(all="ignore"):
        d = pred.astype(F32) - target.astype(F32)
        a = np.abs(d)
        ba = (b * a).astype(F32)
        t = np.log1p((ba / be).astype(F32)).astype(F32)
        inner = (((a_over_b * (ba + F32(1)).astype(F32)).astype(F32) * t).astype(F32) - (al * a).astype(F32)).astype(F32)
        outer = ((ga * a).astype(F32) + outer_c).astype(F32)
        sgn = np.sign(d).astype(F32)
        din = ((al * t).astype(F32) + (knee_c / (ba + be).astype(F32)).astype(F32)).astype(F32)
        dl = np.where(a < be, sgn * din, sgn * ga).astype(F32)
    return np.where(a < be, inner, outer).astype(F32), dl, ~(a < be)


def bbox_head_loss_balanced(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, avg_factor=None,
                            beta=1.0, alpha=0.5, gamma=1.5, g=(1.0, 1.0)):
    """tests/loss_ref.py's ``bbox_head_loss`` with balanced L1 as the box term: the same dict, plus ``outer`` (R, cols):
    the elements on the outer branch, whose float32 gradient ``dreg32`` the kernel must reproduce bit for bit."""
    out = L.bbox_head_loss(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, avg_factor, beta, g)
    R, C = cls_score.shape
    cols = bbox_pred.shape[1]
    s32 = (np.asarray(g, F32) / out["avg"])[1]
    inside = (labels >= 0) & (labels < C)
    lab = np.where(inside, labels, 0)
    rows = np.arange(R)
    col = (4 * lab[:, None] if cols != 4 else np.zeros((R, 1), np.int64)) + np.arange(4)
    pred = np.asarray(bbox_pred, F32)[rows[:, None], col]
    bw = np.where(inside[:, None], bbox_weights, F32(0)).astype(F32)
    with np.errstate(all="ignore"):
        rl, rdl = balanced_l1(pred, bbox_targets, beta, alpha, gamma)
        wr = L._masked(bw, bw * rl)
        dreg_v = L._masked(bw, (bw.astype(np.float64) * rdl) * float(s32))
        _, dl32, outer = balanced_l1_32(pred, bbox_targets, beta, alpha, gamma)
        d32 = np.where(bw != 0, ((bw * dl32).astype(F32) * s32).astype(F32), F32(0)).astype(F32)
    dreg = np.zeros((R, cols))
    dreg32 = np.zeros((R, cols), F32)
    outer_m = np.zeros((R, cols), bool)
    dreg[rows[:, None], col] = dreg_v
    dreg32[rows[:, None], col] = d32
    outer_m[rows[:, None], col] = outer & (bw != 0)
    out["losses"] = np.array([out["losses"][0], wr.sum() / float(out["avg"])])
    out["mag"] = np.array([out["mag"][0], np.abs(wr).sum() / float(out["avg"])])
    out.update(dreg=dreg, dreg32=dreg32, outer=outer_m)
    return out


# ---- IoU-balanced negative sampling (csrc/target.hip) ------------------------------------------------------
import target_ref as TR                                            # noqa: E402
import proposal_ref as PR                                          # noqa: E402


def _smallest(idx, key, k):
    """the k smallest (key, index) of the candidates ``idx`` (all of them if there are no more)"""
    idx = np.asarray(idx, np.int64)
    return idx[np.lexsort((idx, key[idx]))[:max(int(k), 0)]]


def iou_balanced_negatives(assigned, overlaps, key, n, floor_thr=-1.0, floor_fraction=0.0, num_bins=3):
    """The negatives of ONE image chosen by the spec, as a sorted index array.  ``n``: how many may be kept."""
    o = np.asarray(overlaps, F32)
    neg = np.nonzero(np.asarray(assigned) == 0)[0]
    if neg.shape[0] <= n:
        return neg
    thr = F32(floor_thr)
    if thr > 0:
        in_s, t0 = o >= thr, thr
    elif thr == 0:
        in_s, t0 = o > 0, F32(0)
    else:
        in_s, t0 = np.ones(o.shape, bool), F32(0)
    S, Fl = neg[in_s[neg]], neg[~in_s[neg]]
    n_s = int(float(n) * (1.0 - float(F32(floor_fraction))))
    taken = np.zeros(o.shape, bool)
    if S.shape[0] <= n_s:
        taken[S] = True
    elif num_bins >= 2:
        m = o.max()
        w = F32(F32(m - t0) / F32(num_bins))
        per = n_s // num_bins
        for k in range(num_bins):
            lo, hi = F32(t0 + F32(F32(k) * w)), F32(t0 + F32(F32(k + 1) * w))
            members = S[(o[S] >= lo) & (o[S] < hi) & ~taken[S]]
            taken[_smallest(members, key, per)] = True
        got = int(taken.sum())
        if got < n_s:
            taken[_smallest(S[~taken[S]], key, n_s - got)] = True
    else:
        taken[_smallest(S, key, n_s)] = True
    taken[_smallest(Fl, key, n - int(taken.sum()))] = True
    got = int(taken.sum())
    if got < n:
        taken[_smallest(neg[~taken[neg]], key, n - got)] = True
    return np.nonzero(taken)[0]


def lineage_negatives(assigned, overlaps, key, n, floor_thr=-1.0, floor_fraction=0.0, num_bins=3):
    """An independent restatement with Python sets, following mmdetection v1's ``IoUBalancedNegSampler._sample_neg`` /
    ``sample_via_interval`` line by line, ``random_choice(set, k)`` replaced by the k smallest (key, index)."""
    o = [float(F32(v)) for v in overlaps]
    order = lambda s, k: set(sorted(s, key=lambda i: (int(key[i]), i))[:max(k, 0)])
    neg_inds = [i for i, a in enumerate(assigned) if a == 0]
    if len(neg_inds) <= n:
        return np.array(sorted(neg_inds), np.int64)
    thr = float(F32(floor_thr))
    neg_set = set(neg_inds)
    if thr > 0:
        floor_set = {i for i in neg_set if 0 <= o[i] < thr}
        iou_sampling_set = {i for i in neg_set if o[i] >= thr}
    elif thr == 0:
        floor_set = {i for i in neg_set if o[i] == 0}
        iou_sampling_set = {i for i in neg_set if o[i] > 0}
    else:
        floor_set, iou_sampling_set = set(), set(neg_set)
    t0 = F32(thr) if thr > 0 else F32(0)
    num_expected_iou_sampling = int(n * (1 - float(F32(floor_fraction))))
    if len(iou_sampling_set) > num_expected_iou_sampling:
        if num_bins >= 2:
            # sample_via_interval
            max_iou = F32(max(o))
            iou_interval = F32(F32(max_iou - t0) / F32(num_bins))
            per_num_expected = num_expected_iou_sampling // num_bins
            sampled = set()
            for i in range(num_bins):
                start = F32(t0 + F32(F32(i) * iou_interval))
                end = F32(t0 + F32(F32(i + 1) * iou_interval))
                tmp = {j for j in iou_sampling_set if start <= F32(o[j]) < end}
                sampled |= order(tmp, per_num_expected) if len(tmp) > per_num_expected else tmp
            if len(sampled) < num_expected_iou_sampling:
                sampled |= order(iou_sampling_set - sampled, num_expected_iou_sampling - len(sampled))
            iou_sampled = sampled
        else:
            iou_sampled = order(iou_sampling_set, num_expected_iou_sampling)
    else:
        iou_sampled = set(iou_sampling_set)
    num_expected_floor = n - len(iou_sampled)
    floor_sampled = order(floor_set, num_expected_floor) if len(floor_set) > num_expected_floor else set(floor_set)
    chosen = iou_sampled | floor_sampled
    if len(chosen) < n:
        chosen |= order(neg_set - chosen, n - len(chosen))
    return np.array(sorted(chosen), np.int64)


def sample_assigned_iou_balanced(assigned, max_overlaps, num, pos_fraction, neg_pos_ub=-1, floor_thr=-1.0,
                                 floor_fraction=0.0, num_bins=3, keys=None, seed=0, negatives=iou_balanced_negatives):
    a = np.asarray(assigned)
    Bn, n = a.shape
    pos_mask, neg_mask = np.zeros((Bn, n), np.uint8), np.zeros((Bn, n), np.uint8)
    num_pos, num_neg = np.zeros((Bn,), np.int32), np.zeros((Bn,), np.int32)
    for b in range(Bn):
        key = np.asarray(keys[b], dtype=np.int64) if keys is not None else TR.target_key(seed, b, np.arange(n))
        ip, ineg = np.nonzero(a[b] > 0)[0], np.nonzero(a[b] == 0)[0]
        n_pos_exp = int(num * pos_fraction)
        pos = min(ip.shape[0], n_pos_exp)
        n_neg_exp = num - pos
        if neg_pos_ub >= 0:
            n_neg_exp = min(n_neg_exp, int(neg_pos_ub * max(1, pos)))
        pos_mask[b, ip[np.lexsort((ip, key[ip]))[:pos]]] = 1
        chosen = negatives(a[b], max_overlaps[b], key, max(n_neg_exp, 0), floor_thr, floor_fraction, num_bins)
        neg_mask[b, chosen] = 1
        num_pos[b], num_neg[b] = pos, chosen.shape[0]
    return pos_mask, neg_mask, num_pos, num_neg


def sample_rois_iou_balanced(proposals, counts, gt_bboxes, gt_labels, gt_counts, pos_iou_thr=0.5, neg_iou_thr=0.5,
                             min_pos_iou=0.5, num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True,
                             target_means=(0, 0, 0, 0), target_stds=(0.1, 0.1, 0.2, 0.2), keys=None, seed=0,
                             gt_max_assign_all=True, floor_thr=-1.0, floor_fraction=0.0, num_bins=3):
    """tests/target_ref.py's ``sample_rois`` with the negatives chosen by ``iou_balanced_negatives``; also returns the
    candidates' max_overlaps per image (a list) as a ninth value."""
    props = np.asarray(proposals, dtype=F32)
    gt = np.asarray(gt_bboxes, dtype=F32)
    Bn = gt.shape[0]
    rois = np.zeros((Bn * num, 5), F32)
    rois[:, 0] = -1
    labels = np.zeros((Bn * num,), np.int64)
    label_weights = np.zeros((Bn * num,), F32)
    bbox_targets, bbox_weights = np.zeros((Bn * num, 4), F32), np.zeros((Bn * num, 4), F32)
    pos_gt = np.full((Bn * num,), -1, np.int32)
    num_pos, num_neg = np.zeros((Bn,), np.int32), np.zeros((Bn,), np.int32)
    overlaps = []
    for b in range(Bn):
        g = gt[b, :int(gt_counts[b])]
        cand = props[b, :int(counts[b]), :4]
        if add_gt_as_proposals:
            cand = np.concatenate([g, cand])
        a, mo = TR.assign_image(cand, np.ones((cand.shape[0],), bool), g, pos_iou_thr, neg_iou_thr, min_pos_iou,
                                gt_max_assign_all)
        overlaps.append(mo)
        kk = np.asarray(keys[b])[:cand.shape[0]] if keys is not None else TR.target_key(seed, b, np.arange(cand.shape[0]))
        pm, nm, npos, nneg = sample_assigned_iou_balanced(a[None], mo[None], num, pos_fraction, neg_pos_ub, floor_thr,
                                                          floor_fraction, num_bins, [kk])
        ip, ineg = np.nonzero(pm[0])[0], np.nonzero(nm[0])[0]
        r0 = b * num
        r1, r2 = r0 + ip.shape[0], r0 + ip.shape[0] + ineg.shape[0]
        rois[r0:r1, 0], rois[r0:r1, 1:] = b, cand[ip]
        rois[r1:r2, 0], rois[r1:r2, 1:] = b, cand[ineg]
        labels[r0:r1] = np.asarray(gt_labels)[b, a[ip] - 1]
        label_weights[r0:r2] = 1
        bbox_targets[r0:r1] = PR.bbox2delta(cand[ip], g[a[ip] - 1], target_means, target_stds)
        bbox_weights[r0:r1] = 1
        pos_gt[r0:r1] = a[ip] - 1
        num_pos[b], num_neg[b] = npos[0], nneg[0]
    return rois, labels, label_weights, bbox_targets, bbox_weights, pos_gt, num_pos, num_neg, overlaps
