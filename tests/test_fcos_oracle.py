"""CPU: the oracle of the FCOS spec (tests/fcos_ref.py) against independent statements — torch float64
autograd over a plain composition for the losses and gradients, per-point Python loops with their own IoU and greedy
NMS for targets and detections — and hand cases; every host refusal of the wrappers and of the C queries by its
message; the workspace and plan queries against the layout written out; the ctypes mirrors of the new structs against
gcc."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import fcos_cases as K
import fcos_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd
    return torch_detection_amd


# ---- points and targets -------------------------------------------------------------------------------------------------
def test_points_by_hand():
    p = F.points([(2, 3), (1, 1)], [8, 64])
    assert p.dtype == f32 and p.tolist() == [[4, 4, 8, 0], [12, 4, 8, 0], [20, 4, 8, 0], [4, 12, 8, 0], [12, 12, 8, 0],
                                             [20, 12, 8, 0], [32, 32, 64, 1]]
    assert F.points([(1, 2)], [7])[:, :2].tolist() == [[3, 3], [10, 3]]          # s // 2


def target_loop(sizes, strides, ranges, gt, gt_labels, counts, radius):
    """fcos_target point by point and ground truth by ground truth, in numpy float32 scalars."""
    Bn = gt.shape[0]
    out = []
    for b in range(Bn):
        rows = []
        for (H, W), s, (lo, hi) in zip(sizes, strides, ranges):
            for h in range(H):
                for w in range(W):
                    x, y = f32(w * s + s // 2), f32(h * s + s // 2)
                    best = None
                    for j in range(int(counts[b])):
                        x1, y1, x2, y2 = (f32(v) for v in gt[b, j])
                        dist = (x - x1, y - y1, x2 - x, y2 - y)
                        if radius is None:
                            near = min(dist)
                        else:
                            rs = f32(radius) * f32(s)
                            cx, cy = (x1 + x2) * f32(0.5), (y1 + y2) * f32(0.5)
                            near = min(x - max(cx - rs, x1), y - max(cy - rs, y1), min(cx + rs, x2) - x,
                                       min(cy + rs, y2) - y)
                        area = ((x2 - x1) + f32(1)) * ((y2 - y1) + f32(1))
                        if near > 0 and f32(lo) <= max(dist) <= f32(hi) and (best is None or area < best[0]):
                            best = (area, j, dist)
                    rows.append((0, (0, 0, 0, 0), 0) if best is None else
                                (1 if gt_labels is None else int(gt_labels[b, best[1]]), best[2], best[1] + 1))
        out.append(rows)
    return out


@pytest.mark.parametrize("radius", [None, 1.5])
@pytest.mark.parametrize("with_labels", [True, False])
def test_target_oracle_matches_the_loop(radius, with_labels):
    gt, labels, counts = K.gt_case(3, 7, (7, 0, 5), 4)
    labels = labels if with_labels else None
    info = {}
    got = F.target(K.sizes(K.LEVELS), K.strides(K.LEVELS), K.RANGES, gt, labels, counts, radius, info)
    mine = target_loop(K.sizes(K.LEVELS), K.strides(K.LEVELS), K.RANGES, gt, labels, counts, radius)
    assert info["edge"] >= 1 and info["ties"] >= 1
    assert got[3].tolist() == [sum(r[2] > 0 for r in rows) for rows in mine] and got[3][1] == 0 and got[3][0] > 0
    for b, rows in enumerate(mine):
        for i, (lab, dist, a) in enumerate(rows):
            assert got[0][b, i] == lab and got[2][b, i] == a, (b, i)
            assert np.array_equal(got[1][b, i].view(np.uint32), np.asarray(dist, f32).view(np.uint32)), (b, i)


def _one(gt, ranges=((-1, INF),), sizes=((4, 4),), strides=(8,), radius=None, labels=None):
    gt = np.asarray(gt, f32).reshape(1, -1, 4)
    return F.target(sizes, strides, ranges, gt, labels, [gt.shape[1]], radius)


def test_target_hand_cases():
    # points at 4, 12, 20, 28.  A point exactly on a box edge is not inside: min = 0
    lab, bt, a, n = _one([[12, 0, 28, 31]])
    assert a.reshape(4, 4)[:, 1].tolist() == [0] * 4 and a.reshape(4, 4)[:, 2].tolist() == [1] * 4 and n[0] == 4
    assert bt.reshape(4, 4, 4)[0, 2].tolist() == [8, 4, 8, 27]
    # max(l, t, r, b) equal to lo and to hi passes; one beyond does not.  Box (0, 0, 24, 24): point (4, 4) has max 20,
    # point (12, 12) has max 12
    assert _one([[0, 0, 24, 24]], ranges=((20, 20),))[2].reshape(4, 4)[0, 0] == 1
    assert _one([[0, 0, 24, 24]], ranges=((12, 20),))[2].reshape(4, 4)[:3, :3].tolist() == [[1] * 3] * 3
    ring = [[1, 1, 1], [1, 0, 1], [1, 1, 1]]
    assert _one([[0, 0, 24, 24]], ranges=((12.5, 20),))[2].reshape(4, 4)[:3, :3].tolist() == ring
    assert (1 - _one([[0, 0, 24, 24]], ranges=((12, 19.5),))[2].reshape(4, 4)[:3, :3]).tolist() == ring
    # two ground truths of equal area: the lowest index wins; nested boxes: the smaller wins whatever its index
    assert set(_one([[0, 0, 30, 30], [1, 1, 31, 31]])[2][0].tolist()) == {1}
    lab, bt, a, n = _one([[0, 0, 31, 31], [8, 8, 24, 24]], labels=np.array([[3, 5]]))
    assert a.reshape(4, 4).tolist() == [[1, 1, 1, 1], [1, 2, 2, 1], [1, 2, 2, 1], [1, 1, 1, 1]]
    assert lab.reshape(4, 4)[1, 1] == 5 and lab.reshape(4, 4)[0, 0] == 3
    # centre sampling: box (2, 2, 30, 14), centre (16, 8), radius 1.5 * 8 = 12: the centre box (4, 2, 28, 14) is cut by the
    # true box in y only; the point (4, 4) lies on its left edge, (12, 4) and (20, 4) inside; targets stay the true box's
    lab, bt, a, n = _one([[2, 2, 30, 14]], radius=1.5)
    assert a.reshape(4, 4)[0].tolist() == [0, 1, 1, 0] and a.reshape(4, 4)[1].tolist() == [0, 1, 1, 0] and n[0] == 4
    assert bt.reshape(4, 4, 4)[0, 1].tolist() == [10, 2, 18, 10]
    assert _one([[2, 2, 30, 14]])[3][0] == 8                                         # without: the whole box
    # no ground truth at all
    lab, bt, a, n = F.target([(4, 4)], [8], ((-1, INF),), np.zeros((2, 0, 4), f32), None, [0, 0])
    assert not lab.any() and not bt.any() and not a.any() and n.tolist() == [0, 0]


# ---- loss -----------------------------------------------------------------------------------------------------------------
def torch_loss(cls, reg, ctr, labels, bt, scales, giou, gamma, alpha, eps, g):
    """The three losses as a plain torch composition in float64; min / max written with their masks."""
    Bn, C = cls[0].shape[:2]
    flat = lambda ts: torch.cat([t.permute(0, 2, 3, 1).reshape(Bn, -1, t.shape[1]) for t in ts], 1)
    x, r, z = flat(cls), flat(reg), flat(ctr)[..., 0]
    lev = torch.cat([torch.full((t.shape[2] * t.shape[3],), l) for l, t in enumerate(cls)])
    lab = torch.from_numpy(labels)
    pos = lab > 0
    npos = int(pos.sum())
    a = float(f32(alpha))
    onehot = lab[..., None] == torch.arange(1, C + 1)
    p = torch.sigmoid(x)
    ls, lns = torch.nn.functional.logsigmoid(x), torch.nn.functional.logsigmoid(-x)
    focal = torch.where(onehot, -a * (1 - p) ** gamma * ls, -float(f32(1) - f32(alpha)) * p ** gamma * lns)
    loss_cls = focal.sum() / (npos + Bn)
    bi, ii = torch.nonzero(pos, as_tuple=True)
    s = torch.ones(len(cls), dtype=torch.float64) if scales is None else scales
    d = torch.exp(s[lev[ii]][:, None] * r[bi, ii])
    t = torch.from_numpy(bt).double()[bi, ii]
    c = torch.sqrt(torch.minimum(t[:, 0], t[:, 2]) / torch.maximum(t[:, 0], t[:, 2]) *
                   torch.minimum(t[:, 1], t[:, 3]) / torch.maximum(t[:, 1], t[:, 3]))
    mn, mx = torch.where(d <= t, d, t), torch.where(d >= t, d, t)
    area = lambda q: (q[:, 0] + q[:, 2] + 1) * (q[:, 1] + q[:, 3] + 1)
    inter, enc = area(mn), area(mx)
    union = area(d) + area(t) - inter
    iou = inter / union
    if giou:
        lb = 1 - (iou - (enc - union) / enc)
    else:
        lb = -torch.log(torch.where(iou >= eps, iou, torch.full_like(iou, eps)))
    loss_box = (c * lb).sum() / c.sum() if npos else x.sum() * 0
    zz = z[bi, ii]
    loss_ctr = torch.nn.functional.binary_cross_entropy_with_logits(zz, c, reduction="sum") / max(npos, 1)
    losses = torch.stack([loss_cls, loss_box, loss_ctr])
    (losses * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return losses.detach().numpy()


def _loss_inputs(levels, Bn, C, seed, counts=(7, 3), ranges=K.RANGES):
    gt, gl, cn = K.gt_case(Bn, 7, counts, seed)
    labels, bt, _, num_pos = F.target(K.sizes(levels), K.strides(levels), ranges, gt, gl, cn)
    return labels, bt, K.loss_case(levels, Bn, C, labels, bt, seed + 1)


@pytest.mark.parametrize("loss_type,with_scales,eps", [("iou", False, 1e-6), ("iou", True, 1e-3), ("giou", True, 1e-6),
                                                       ("giou", False, 1e-6)])
def test_loss_oracle_matches_torch_autograd(loss_type, with_scales, eps):
    Bn, C = 2, 5
    labels, bt, arrs = _loss_inputs(K.LEVELS, Bn, C, 11)
    scales = np.array([1.25, 0.75, 1.0], f32) if with_scales else None
    g = (1.5, 0.75, 2.0)
    ref = F.loss([a[0] for a in arrs], [a[1] for a in arrs], [a[2] for a in arrs], labels, bt, scales, loss_type, 2.0,
                 0.25, eps, g)
    assert ref["num_pos"] >= 20
    pos_r = np.concatenate([F.rows(a[1]) for a in arrs], 1)[labels > 0]
    assert (np.exp(pos_r) == bt[labels > 0]).sum() >= 1, "a min / max tie"
    if eps == 1e-3:
        assert (ref["iou"] < eps).sum() >= 2 and np.abs(ref["iou"] / eps - 1).min() > 1e-3
    leaf = [[torch.from_numpy(np.nan_to_num(a[k], nan=0.5, posinf=0.5, neginf=0.5)).double().requires_grad_()
             for a in arrs] for k in range(3)]
    ts = None if scales is None else torch.from_numpy(scales).double().requires_grad_()
    losses = torch_loss(leaf[0], leaf[1], leaf[2], labels, bt, ts, loss_type == "giou", 2.0, 0.25, float(f32(eps)), g)
    np.testing.assert_allclose(ref["losses"], losses, rtol=1e-12, atol=0)
    # the oracle rounds g / (positives + B) and g / max(positives, 1) to float32 once, as the kernel does: 2^-24 relative
    for k, (name, rtol) in enumerate((("dcls", 2.0 ** -23), ("dreg", 1e-10), ("dctr", 2.0 ** -23))):
        for l in range(len(arrs)):
            np.testing.assert_allclose(ref[name][l], leaf[k][l].grad.numpy(), rtol=rtol, atol=1e-15, err_msg=name)
    pos = labels > 0
    for l, n0 in enumerate(np.cumsum([0] + [h * w for (h, w), _ in K.LEVELS])[:-1]):
        h, w = K.LEVELS[l][0]
        m = pos[:, n0:n0 + h * w].reshape(Bn, 1, h, w)
        assert not ref["dreg"][l][np.broadcast_to(~m, ref["dreg"][l].shape)].any() and not ref["dctr"][l][~m].any()
    if scales is not None:
        np.testing.assert_allclose(ref["dscale"], ts.grad.numpy(), rtol=1e-10)
        assert np.all(ref["bound_dscale"][ref["dscale"] != 0] > 0) and np.count_nonzero(ref["dscale"]) >= 2
    # the bounds are bounds on something: positive wherever a value is
    assert np.all(ref["bound_losses"] > 0)
    for l in range(len(arrs)):
        assert np.all(ref["bound_dreg"][l][ref["dreg"][l] != 0] > 0)


def test_loss_hand_cases():
    one = lambda v, ch=1: np.full((1, ch, 1, 1), v, f32)
    # no positive at all: loss_cls divides by 0 + B, the other two are exactly 0 with all-zero gradients
    ref = F.loss([one(0.0, 2)], [one(np.nan, 4)], [one(np.nan)], np.zeros((1, 1), np.int64), np.zeros((1, 1, 4), f32))
    focal0 = 0.75 * 0.25 * math.log(2)                                  # (1 - alpha) sigma(0)^2 softplus(0)
    assert ref["losses"][0] == pytest.approx(2 * focal0, rel=1e-12) and ref["losses"][1:].tolist() == [0, 0]
    assert ref["norm"].tolist() == [1, 0, 1] and not ref["dreg"][0].any() and not ref["dctr"][0].any()
    # a perfect prediction: iou 1, both box losses 0; c* of a centred point is 1 and the centre-ness loss softplus(z) - z
    t = np.array([[[4, 4, 4, 4]]], f32)
    lab = np.ones((1, 1), np.int64)
    x = one(math.log(4), 4)
    for kind in ("iou", "giou"):
        ref = F.loss([one(0.0)], [x], [one(1.0)], lab, t, None, kind)
        assert abs(ref["losses"][1]) < 1e-6 and ref["norm"].tolist() == [2, 1, 1]      # log(4) is rounded to fp32
        assert ref["losses"][2] == pytest.approx(math.log1p(math.exp(-1.0)), rel=1e-12)
    # c* = sqrt(1/3 * 2/4); d = (1, 1, 1, 1) against (1, 2, 3, 4): inter 3 * 3, areas 3 * 3 and 5 * 7, enclosing 5 * 7
    t = np.array([[[1, 2, 3, 4]]], f32)
    ref = F.loss([one(0.0)], [one(0.0, 4)], [one(0.0)], lab, t, None, "iou")
    assert ref["norm"][1] == pytest.approx(math.sqrt(1 / 6), rel=1e-12)
    assert ref["losses"][1] == pytest.approx(-math.log(9 / 35), rel=1e-12)
    ref = F.loss([one(0.0)], [one(0.0, 4)], [one(0.0)], lab, t, None, "giou")
    assert ref["losses"][1] == pytest.approx(1 - 9 / 35, rel=1e-12)                      # union == enclosing
    # GIoU with disjoint extents: the prediction reaches 1 left / up, the target 1 right / down (both hold the point, so
    # the '+1' intersection is 2 x 2): areas 3.5 * 4.5 each, enclosing 5 * 7
    t = np.array([[[0.5, 0.5, 2, 3]]], f32)
    x = np.log(np.array([2, 3, 0.5, 0.5], f32)).reshape(1, 4, 1, 1)
    ref = F.loss([one(0.0)], [x], [one(0.0)], lab, t, None, "giou")
    inter, union, enc = 2 * 2, 3.5 * 4.5 * 2 - 4, 5 * 7
    assert ref["losses"][1] == pytest.approx(1 - (inter / union - (enc - union) / enc), rel=1e-6)
    # iou < eps: the loss is -log(eps) and the box gradient exactly 0
    t = np.array([[[40, 40, 40, 40]]], f32)
    ref = F.loss([one(0.0)], [one(-8.0, 4)], [one(0.0)], lab, t, None, "iou", eps=1e-3)
    assert ref["iou"][0] < 1e-3 and ref["losses"][1] == pytest.approx(-math.log(float(f32(1e-3))), rel=1e-12)
    assert not ref["dreg"][0].any() and ref["dctr"][0].any()


# ---- detections -----------------------------------------------------------------------------------------------------------
def _iou1(a, b):
    area = lambda r: ((r[2] - r[0]) + f32(1)) * ((r[3] - r[1]) + f32(1))
    w = max((min(a[2], b[2]) - max(a[0], b[0])) + f32(1), f32(0))
    h = max((min(a[3], b[3]) - max(a[1], b[1])) + f32(1), f32(0))
    inter = w * h
    return inter / ((area(a) + area(b)) - inter)


def restatement(cls, reg, ctr, strides, shapes, scales, scale, nms_pre, score_thr, nms_thr, max_per_img):
    """get_bboxes image by image with Python floats: scores times centre-ness first, their maximum, the top nms_pre of
    it, the decode, the rescale, NMS class by class on the float32 rows, one final sort."""
    Bn, C = cls[0].shape[:2]
    sig = lambda v: 1.0 / (1.0 + math.exp(-float(v)))
    out = []
    for b in range(Bn):
        rws, poff = [], 0
        for l, (c, r, z, s) in enumerate(zip(cls, reg, ctr, strides)):
            H, W = c.shape[2:]
            level = []
            for h in range(H):
                for w in range(W):
                    zc = sig(z[b, 0, h, w])
                    sc = [sig(c[b, k, h, w]) * zc for k in range(C)]
                    level.append((max(sc), h * W + w, sc, (w * s + s // 2, h * s + s // 2), r[b, :, h, w]))
            if 0 < nms_pre < len(level):
                level = sorted(sorted(level, key=lambda t: (-t[0], t[1]))[:nms_pre], key=lambda t: t[1])
            for _, i, sc, (px, py), x in level:
                d = [math.exp(float(1.0 if scales is None else f32(scales[l])) * float(v)) for v in x]
                ih, iw = shapes[b]
                box = [min(max(px - d[0], 0), iw - 1), min(max(py - d[1], 0), ih - 1), min(max(px + d[2], 0), iw - 1),
                       min(max(py + d[3], 0), ih - 1)]
                if scale is not None:
                    box = [v / float(f32(scale[b])) for v in box]
                rws.append((poff + i, [f32(v) for v in sc], [f32(v) for v in box]))
            poff += H * W
        found = []
        for k in range(C):
            cand = sorted([(n, r) for n, r in enumerate(rws) if r[1][k] > f32(score_thr)],
                          key=lambda t: (-float(t[1][1][k]), t[0]))
            keep = []
            for n, r in cand:
                if all(not _iou1(q[2], r[2]) > f32(nms_thr) for _, q in keep):
                    keep.append((n, r))
            found += [(float(r[1][k]), k, n, r[0], r[2]) for n, r in keep]
        out.append(sorted(found, key=lambda t: (-t[0], t[1], t[2]))[:max_per_img])
    return out


@pytest.mark.parametrize("nms_pre,scale,with_scales,C", [(10, None, False, 3), (0, (2.0, 0.5), True, 1),
                                                         (7, (1.5, 1.5), True, 2)])
def test_detection_oracle_matches_the_plain_python_restatement(nms_pre, scale, with_scales, C):
    levels = [((3, 4), 8), ((2, 2), 16)]
    Bn = 2
    arrs = K.det_case(levels, Bn, C, 3 + C)
    cls, reg, ctr = ([a[k] for a in arrs] for k in range(3))
    scales = np.array([1.125, 0.875], f32) if with_scales else None
    shapes = [(30, 40), (28, 37)]
    ref = F.detections(cls, reg, ctr, K.strides(levels), shapes, scales, scale, nms_pre, 0.05, 0.5, 6)
    mine = restatement(cls, reg, ctr, K.strides(levels), shapes, scales, scale, nms_pre, 0.05, 0.5, 6)
    dets, labels, pidx, counts = ref[:4]
    k, off, Ktot = F.plan([h * w for (h, w), _ in levels], nms_pre)
    assert counts.tolist() == [len(m) for m in mine] and min(counts) >= 2
    for b, m in enumerate(mine):
        for j, (s, c, n, i, box) in enumerate(m):
            assert labels[b, j] == c and pidx[b, j] == i and ref[8][b, j] == b * Ktot + n
            assert np.array_equal(dets[b, j].view(np.uint32), np.asarray(box + [s], f32).view(np.uint32)), (b, j)
        assert not dets[b, len(m):].any() and (labels[b, len(m):] == -1).all() and (pidx[b, len(m):] == -1).all()
    assert ref[4].shape == (Bn * Ktot, C + 1) and not ref[4][:, 0].any()
    for b in range(Bn):
        for kl, o in zip(k, off):
            assert (np.diff(ref[7][b * Ktot + o:b * Ktot + o + kl]) > 0).all()   # ascending point order


def test_nms_pre_cuts_through_a_tie():
    """Five points with two distinct keys: the cut takes the first ties in point order."""
    c = np.array([2.0, 1.0, 2.0, 1.0, 1.0], f32).reshape(1, 1, 1, 5)
    z = np.zeros((1, 1, 1, 5), f32)
    r = np.zeros((1, 4, 1, 5), f32)
    info = {}
    d = F.dense([c], [r], [z], [8], [(64, 64)], None, None, 3, info)
    assert d["point_idx"].tolist() == [0, 1, 2] and info["cuts"] == [dict(cut=float(F.sg(1.0) * 0.5), above=2, ties=3,
                                                                          taken=1)]
    assert d["scores"][:, 1].tolist() == (F.sg(np.array([2.0, 1.0, 2.0])) * 0.5).tolist()
    assert d["boxes"][1].tolist() == [11, 3, 13, 5]                                    # point (12, 4) -+ exp(0)
    assert F.dense([c], [r], [z], [8], [(64, 64)], None, None, 5)["point_idx"].tolist() == [0, 1, 2, 3, 4]
    # the clip and the scale factor: image 4 wide -> x in [0, 3]; boxes divided by 2
    d = F.dense([c], [r], [z], [8], [(64, 4)], None, 2.0, 0)
    assert d["boxes"][0].tolist() == [1.5, 1.5, 1.5, 2.5] and d["boxes"][4].tolist() == [1.5, 1.5, 1.5, 2.5]


def test_the_gpu_detection_cases_are_decided_by_the_oracle():
    """The grids give exact key ties, and distinct keys lie further apart than the fp32 keys can err."""
    arrs = K.det_case(K.LEVELS, 3, 5, 21)
    info = {}
    F.dense([a[0] for a in arrs], [a[1] for a in arrs], [a[2] for a in arrs], K.strides(K.LEVELS), K.img_shapes(3), None,
            None, 50, info)
    assert any(c["above"] > 0 and c["ties"] > c["taken"] for c in info["cuts"])
    distinct = equal = 0
    for keys, mag in info["keys"]:
        o = np.argsort(keys)
        k, m = keys[o], mag[o]
        gap = np.diff(k) / k[1:]
        live = gap > 0
        distinct, equal = distinct + int(live.sum()), equal + int((~live).sum())
        assert np.all(gap[live] > 2 * (33 + np.maximum(m[1:], m[:-1])[live]) * F.U)
    assert distinct >= 20 and equal >= 20


# ---- host refusals --------------------------------------------------------------------------------------------------------
def _heads(Bn=2, C=3, sizes=((4, 6), (2, 3)), dtype=torch.float32):
    mk = lambda ch: [torch.zeros(Bn, ch, h, w, dtype=dtype) for h, w in sizes]
    return mk(C), mk(4), mk(1)


def test_wrapper_refusals_need_no_gpu(T):
    gt, cnt = torch.zeros(2, 3, 4), torch.zeros(2, dtype=torch.int32)
    sz, st, rg = [(4, 6), (2, 3)], [8, 16], [(-1, 32), (32, INF)]
    for args, msg in [(([], [], []), "1..8 levels"), (([(1, 1)] * 9, [1] * 9, [(0, 1)] * 9), "1..8 levels"),
                      ((sz, [8], rg), "2 featmap_sizes but 1 strides"), ((sz, [8, 0], rg), r"strides\[1\] must be in"),
                      ((sz, st, rg[:1]), "1 regress_ranges"), ((sz, st, [(-1, 32), (40, 32)]), "lo <= hi"),
                      ((sz, st, [(-1, 32), (32, float("nan"))]), "lo <= hi"),
                      (([(1024, 1025)], [8], [(0, 1)]), "points per image"),
                      (([(4, 0)], [8], [(0, 1)]), "level 0 width"), (([(1, 1024)], [1 << 15], [(0, 1)]), "below 2\\^24")]:
        with pytest.raises(ValueError, match=msg):
            T.fcos_target(args[0], args[1], args[2], gt, None, cnt)
    with pytest.raises(ValueError, match="1..8 levels"):
        T.fcos_points([], [])
    for kw, msg in [(dict(gt_bboxes=gt.double()), "gt_bboxes must be"), (dict(gt_bboxes=torch.zeros(2, 257, 4)), "max 256"),
                    (dict(gt_counts=cnt.long()), "gt_counts must be"), (dict(gt_labels=torch.zeros(2, 3)), "gt_labels"),
                    (dict(center_sample_radius=0.0), "center_sample_radius must be finite and > 0"),
                    (dict(), "gt_bboxes must be a CUDA tensor")]:
        a = dict(gt_bboxes=gt, gt_labels=None, gt_counts=cnt)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.fcos_target(sz, st, rg, **a)

    cls, reg, ctr = _heads()
    N = 30
    lab, bt = torch.zeros(2, N, dtype=torch.int64), torch.zeros(2, N, 4)
    bad_layout = torch.zeros(2, 4, 3, 6).permute(0, 2, 1, 3)
    for a, kw, msg in [(_heads(sizes=((1, 1),) * 9), {}, "one cls_score, one bbox_pred and one centerness each"),
                       ((cls, [r.half() for r in reg], ctr), {}, r"bbox_preds\[0\] must be a float32"),
                       ((cls, [torch.zeros(2, 8, 4, 6), reg[1]], ctr), {}, r"bbox_preds\[0\]"),
                       ((cls, reg, [torch.zeros(2, 2, 4, 6), ctr[1]]), {}, r"centernesses\[0\]"),
                       (([bad_layout, cls[1]], reg, ctr), {}, "NCHW-contiguous or channels_last"),
                       ((_heads(65)), {}, "batch size"), ((cls, reg, ctr), dict(labels=lab[:, :29]), "N = 30 points"),
                       ((cls, reg, ctr), dict(bbox_targets=bt.double()), "bbox_targets must be"),
                       ((cls, reg, ctr), dict(loss_type="diou"), "loss_type must be 'iou' or 'giou'"),
                       ((cls, reg, ctr), dict(gamma=-1.0), "gamma >= 0"), ((cls, reg, ctr), dict(alpha=1.5), "alpha in"),
                       ((cls, reg, ctr), dict(eps=0.0), r"eps must be in \(0, 1\)"),
                       ((cls, reg, ctr), dict(scales=torch.ones(3)), "scales must be"),
                       ((cls, reg, ctr), {}, "must be a CUDA tensor")]:
        k = dict(labels=lab, bbox_targets=bt)
        k.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.fcos_loss(a[0], a[1], a[2], **k)
    with pytest.raises(ValueError, match="2 cls_scores, 1 bbox_preds"):
        T.fcos_loss(cls, reg[:1], ctr, lab, bt)

    shp = torch.zeros(2, 2, dtype=torch.int32)
    for kw, msg in [(dict(nms_pre=4097), "nms_pre must be in 0..4096"), (dict(max_per_img=0), "max_per_img must be in"),
                    (dict(img_shapes=shp.long()), "img_shapes must be"), (dict(scale_factors=-1.0), "scale_factors must be"),
                    (dict(scale_factors=torch.ones(3)), "scale_factors must be"), (dict(score_thr=INF), "score_thr"),
                    (dict(strides=[8]), "featmap_sizes but 1 strides"), (dict(scales=torch.ones(2, 1)), "scales must be"),
                    (dict(), "must be a CUDA tensor")]:
        k = dict(strides=st, img_shapes=shp)
        k.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.fcos_detections(cls, reg, ctr, **k)
    big = _heads(64, 1, ((65, 64),))                                   # 64 * 4160 rows > 2^18
    with pytest.raises(ValueError, match="dense rows"):
        T.fcos_detections(*big, [8], torch.zeros(64, 2, dtype=torch.int32), nms_pre=0)
    with pytest.raises(ValueError, match="dense rows"):
        T.fcos_detections_plan([(512, 513)], 1, 1, 0)
    with pytest.raises(ValueError, match="num_classes must be in 1..1023"):
        T.fcos_detections_plan([(4, 4)], 1, 1024, 0)


def _table(sizes, strides=None, ranges=None, nhwc=0):
    from torch_detection_amd import _lib
    arr = (_lib.FcosLevel * len(sizes))()
    for l, (H, W) in enumerate(sizes):
        arr[l].H, arr[l].W, arr[l].stride = H, W, strides[l] if strides else 1
        arr[l].lo, arr[l].hi = ranges[l] if ranges else (0, 1)
        arr[l].cls_nhwc = arr[l].reg_nhwc = nhwc
    return arr


def _a256(n):
    return (n + 255) // 256 * 256


def test_c_queries_and_refusals(T):
    from torch_detection_amd import _lib
    lib = _lib.load()
    err = lambda: lib.tdn_last_error().decode()
    sz = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
    N = sum(h * w for h, w in sz)
    arr = _table(sz)
    # targets: one count word per workgroup of 256 points and image
    assert lib.tdn_fcos_target_workspace_bytes(arr, 5, 2, 20) == _a256(4 * 2 * -(-N // 256))
    assert lib.tdn_fcos_target_workspace_bytes(arr, 5, 2, 257) == -1 and "ground truths per image" in err()
    assert lib.tdn_fcos_target_workspace_bytes(arr, 5, 65, 2) == -1 and "out of 1..64" in err()
    assert lib.tdn_fcos_target_workspace_bytes(arr, 9, 1, 2) == -1 and "levels" in err()
    assert lib.tdn_fcos_target_workspace_bytes(_table(sz, ranges=[(2, 1)] * 5), 5, 1, 2) == -1 and "regress range" in err()
    assert lib.tdn_fcos_target_workspace_bytes(_table(sz, strides=[0] * 5), 5, 1, 2) == -1 and "stride" in err()
    assert lib.tdn_fcos_target_workspace_bytes(_table([(1024, 1025)]), 1, 1, 2) == -1 and "points per image" in err()
    assert lib.tdn_fcos_points(arr, 5, None, None) == -1 and "NULL output" in err()
    assert lib.tdn_fcos_target(arr, 5, 1, None, None, None, 0, -1.0, None, None, None, None, None, 0, None) == -1 and \
        "radius" in err()
    # loss: 16 doubles per workgroup of 1024 chunks (or points), at most 256 workgroups
    cfg = _lib.FcosLossConfig()
    cfg.dtype, cfg.num_classes, cfg.gamma, cfg.alpha, cfg.eps = _lib.TDN_BF16, 80, 2.0, 0.25, 1e-6
    assert lib.tdn_fcos_loss_workspace_bytes(arr, 5, 2, ctypes.byref(cfg)) == 256 * 128
    small = _table([(2, 3)])
    cfg.num_classes, cfg.dtype = 5, _lib.TDN_F32
    assert lib.tdn_fcos_loss_workspace_bytes(small, 1, 1, ctypes.byref(cfg)) == 256       # one workgroup: 128 B
    cfg.num_classes = 1400
    assert lib.tdn_fcos_loss_workspace_bytes(small, 1, 300 // 6, ctypes.byref(cfg)) == -1 and "C=1400" in err()
    cfg.num_classes = 1000                                                                # 50 * 1000 * 6 / 4 chunks
    assert lib.tdn_fcos_loss_workspace_bytes(small, 1, 50, ctypes.byref(cfg)) == _a256(128 * -(-75000 // 1024))
    for field, value, msg in [("eps", 0.0, "eps"), ("eps", 1.0, "eps"), ("gamma", -1.0, "gamma"), ("alpha", 2.0, "alpha"),
                              ("giou", 2, "giou"), ("dtype", 7, "dtype"), ("num_classes", 0, "C=0")]:
        c2 = _lib.FcosLossConfig.from_buffer_copy(cfg)
        setattr(c2, field, value)
        assert lib.tdn_fcos_loss_workspace_bytes(small, 1, 1, ctypes.byref(c2)) == -1 and msg in err(), field
    # detections: key words of the levels that select, then tdn_multiclass_nms's workspace
    dc = _lib.FcosDetConfig()
    dc.dtype, dc.num_classes, dc.nms_pre, dc.max_num, dc.score_thr, dc.nms_thr = _lib.TDN_BF16, 80, 1000, 100, 0.05, 0.5
    out = (ctypes.c_int32 * 16)()
    for nhwc in (1, 0):
        arr = _table(sz, nhwc=nhwc)
        assert lib.tdn_fcos_detections_plan(arr, 5, 2, ctypes.byref(dc), out) == 0, err()
        k, off, Ktot = F.plan([h * w for h, w in sz], 1000)
        ta = min(256, 8192 // 81) if nhwc else 256
        groups = sum(2 * -(-h * w // ta) for h, w in sz if h * w > 1000)
        words = 2 * sum((h * w + 3) // 4 * 4 for h, w in sz)
        assert list(out) == [Ktot, 2 * Ktot, N, 7, groups, 3, words, 0] + k + [0, 0, 0]
        assert lib.tdn_fcos_detections_workspace_bytes(arr, 5, 2, ctypes.byref(dc)) == \
            _a256(4 * words) + lib.tdn_multiclass_nms_workspace_bytes(2 * Ktot, 81, 2)
    dc.nms_pre = 0
    assert lib.tdn_fcos_detections_plan(_table([(8, 12), (1, 1)]), 2, 3, ctypes.byref(dc), out) == 0
    assert list(out)[:8] == [97, 291, 97, 6, 0, 0, 0, 0]
    for field, value, msg in [("nms_pre", 4097, "nms_pre"), ("max_num", 0, "max_num"), ("num_classes", 1024, "C=1024"),
                              ("score_thr", INF, "finite"), ("dtype", 5, "dtype")]:
        c2 = _lib.FcosDetConfig.from_buffer_copy(dc)
        setattr(c2, field, value)
        assert lib.tdn_fcos_detections_plan(arr, 5, 2, ctypes.byref(c2), out) == -1 and msg in err(), field
    assert lib.tdn_fcos_detections_plan(_table([(512, 513)]), 1, 1, ctypes.byref(dc), out) == -1 and "dense rows" in err()


def test_plan_wrapper(T):
    p = T.fcos_detections_plan(K.sizes(K.LEVELS), 3, 5, 50)
    assert p == dict(K=80, rows=240, points=126, launches=7, key_workgroups=3, selecting=1, key_words=3 * 128,
                     kept=[50, 24, 6])
    assert T.fcos_detections_plan(K.sizes(K.LEVELS), 3, 5, 0)["launches"] == 6


def test_new_struct_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of the structs this section adds to include/tdn.h as gcc lays them out == the ctypes mirrors."""
    from torch_detection_amd import _lib
    mirrors = {"tdn_fcos_level": _lib.FcosLevel, "tdn_fcos_loss_config": _lib.FcosLossConfig,
               "tdn_fcos_det_config": _lib.FcosDetConfig}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {']
    for cname, cls in mirrors.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)]).decode().split("\n"):
        if ln:
            cname, fname, val = ln.split()
            cls = mirrors[cname]
            got = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
            assert got == int(val), (cname, fname, got, val)
            seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in mirrors.values())
    hdr = open(os.path.join(ROOT, "include", "tdn.h")).read()
    assert "#define TDN_FCOS_MAX_LEVELS %d\n" % _lib.FCOS_MAX_LEVELS in hdr
