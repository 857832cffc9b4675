"""CPU: the oracle of the single-stage head spec (tests/dense_detect_ref.py) against an independent
plain-Python restatement and hand cases; every host refusal of the two wrappers by its message; the workspace and plan
queries against the layout written out; the ctypes mirrors of the new structs against gcc."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import dense_detect_cases as K
import dense_detect_ref as DD
import proposal_ref as P
from oracle import box_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd
    return torch_detection_amd


# ---- an independent restatement: per-anchor loops, Python's sort, mmdetection's order of operations -----------------
def _decode1(anchor, delta, means, stds, shape, clip):
    d = [f32(f32(delta[j]) * f32(stds[j])) + f32(means[j]) for j in range(4)]
    mr = f32(abs(math.log(clip)))
    dw, dh = min(max(d[2], -mr), mr), min(max(d[3], -mr), mr)
    px, py = (anchor[0] + anchor[2]) * f32(0.5), (anchor[1] + anchor[3]) * f32(0.5)
    pw, ph = (anchor[2] - anchor[0]) + f32(1), (anchor[3] - anchor[1]) + f32(1)
    gw, gh = pw * f32(math.exp(dw)), ph * f32(math.exp(dh))
    gx, gy = px + pw * d[0], py + ph * d[1]
    hw, hh = gw * f32(0.5), gh * f32(0.5)
    box = [(gx - hw) + f32(0.5), (gy - hh) + f32(0.5), (gx + hw) - f32(0.5), (gy + hh) - f32(0.5)]
    lim = [f32(shape[1] - 1), f32(shape[0] - 1)] * 2
    return [min(max(v, f32(0)), m) for v, m in zip(box, lim)]


def _iou1(a, b):
    area = lambda r: ((r[2] - r[0]) + f32(1)) * ((r[3] - r[1]) + f32(1))
    w = max((min(a[2], b[2]) - max(a[0], b[0])) + f32(1), f32(0))
    h = max((min(a[3], b[3]) - max(a[1], b[1])) + f32(1), f32(0))
    inter = w * h
    return inter / ((area(a) + area(b)) - inter)


def restatement(cls_scores, bbox_preds, anchors, shapes, scale, nms_pre, score_thr, nms_thr, max_per_img, means, stds,
                clip=16 / 1000):
    """get_bboxes image by image: sigmoid first, then the maximum over the classes, the top nms_pre of it, the decode,
    the rescale, the zero column, NMS class by class, one final sort."""
    Bn = cls_scores[0].shape[0]
    A = bbox_preds[0].shape[1] // 4
    C = cls_scores[0].shape[1] // A
    out = []
    for b in range(Bn):
        rows = []                                             # (pyramid anchor, scores[C], box)
        aoff = 0
        for cls, reg, anc in zip(cls_scores, bbox_preds, anchors):
            H, W = cls.shape[2:]
            level = []
            for h in range(H):
                for w in range(W):
                    for a in range(A):
                        x = [f32(cls[b, a * C + c, h, w]) for c in range(C)]
                        s = [f32(1) / (f32(1) + f32(math.exp(-float(v)))) for v in x]
                        i = (h * W + w) * A + a
                        level.append((max(s), i, s, [reg[b, 4 * a + j, h, w] for j in range(4)]))
            if 0 < nms_pre < len(level):
                level = sorted(level, key=lambda t: (-float(t[0]), t[1]))[:nms_pre]
            for _, i, s, d in level:
                box = _decode1(anc[i], d, means, stds, shapes[b], clip)
                if scale is not None:
                    box = [v / f32(scale[b]) for v in box]
                rows.append((aoff + i, s, box))
            aoff += H * W * A
        found = []
        for c in range(C):
            cand = sorted([r for r in rows if r[1][c] > f32(score_thr)], key=lambda r: (-float(r[1][c]), r[0]))
            keep = []
            for r in cand:
                if all(not _iou1(k[2], r[2]) > f32(nms_thr) for k in keep):
                    keep.append(r)
            found += [(float(r[1][c]), c, r[0], r[2]) for r in keep]
        found = sorted(found, key=lambda t: (-t[0], t[1], t[2]))[:max_per_img]
        out.append(found)
    return out


@pytest.mark.parametrize("nms_pre,scale,C", [(10, None, 3), (0, (2.0, 0.5), 1), (7, (1.5, 1.5), 2)])
def test_oracle_matches_the_plain_python_restatement(nms_pre, scale, C):
    levels = [((3, 4), 8), ((2, 2), 16)]
    A, Bn = 2, 2
    anchors = K.pyramid(levels, A)
    g = np.random.default_rng(3 + C)
    cls = [g.choice(K.GRID32, (Bn, A * C, h, w)).astype(f32) for (h, w), _ in levels]
    reg = [g.normal(0, 0.4, (Bn, 4 * A, h, w)).astype(f32) for (h, w), _ in levels]
    shapes = [(30, 40), (28, 37)]
    ref = DD.anchor_head_detections(cls, reg, anchors, shapes, scale, nms_pre, 0.05, 0.5, 6, K.MEANS, K.STDS)
    mine = restatement(cls, reg, anchors, shapes, scale, nms_pre, 0.05, 0.5, 6, K.MEANS, K.STDS)
    dets, labels, aidx, counts = ref[:4]
    assert counts.tolist() == [len(m) for m in mine] and min(counts) >= 2
    for b, m in enumerate(mine):
        for j, (s, c, i, box) in enumerate(m):
            assert labels[b, j] == c and aidx[b, j] == i
            assert np.array_equal(dets[b, j].view(np.uint32), np.asarray(box + [s], f32).view(np.uint32)), (b, j)
        assert not dets[b, len(m):].any() and (labels[b, len(m):] == -1).all() and (aidx[b, len(m):] == -1).all()
    # the dense tensors reproduce the selection, and are laid out as step 2 says
    k, off, Ktot = DD.plan([h * w * A for (h, w), _ in levels], nms_pre)
    assert ref[4].shape == (Bn * Ktot, C + 1) and not ref[4][:, 0].any()
    assert ref[6].tolist() == sorted(ref[6].tolist())
    for b in range(Bn):
        for kl, o in zip(k, off):
            seg = ref[7][b * Ktot + o:b * Ktot + o + kl]
            assert (np.diff(seg) > 0).all()                  # ascending anchor order inside (image, level)
    again = DD.select(ref[5], ref[4], ref[6], ref[7], Bn, 0.05, 0.5, 6)
    for a, r in zip(again, (dets, labels, aidx, counts, ref[8])):
        assert np.array_equal(a, r)


# ---- hand cases ------------------------------------------------------------------------------------------------------
def _one_level(keys, C=1, W=None):
    """A (1, C, 1, n) level (A = 1) whose anchors' class maxima are ``keys`` (class 0 carries them)."""
    n = len(keys)
    cls = np.full((1, C, 1, n), -6.0, f32)
    cls[0, 0, 0] = keys
    reg = np.zeros((1, 4, 1, n), f32)
    anchors = np.stack([np.asarray([40 * i, 0, 40 * i + 19, 19], f32) for i in range(n)])     # disjoint
    return [cls], [reg], [anchors], [(64, 40 * n)]


def test_tie_straddling_the_cut_takes_the_lower_anchors():
    keys = f32([1, 3, 2, 2, 0, 2, 5, 2])                    # nms_pre = 4: 5, 3, then the first two of the four 2s
    info = {}
    d = DD.dense(*_one_level(keys), None, 4, info=info)
    assert d["anchor_idx"].tolist() == [1, 2, 3, 6]         # ascending anchor order
    assert info["cuts"] == [dict(cut=2.0, above=2, ties=4, taken=2)]
    out = DD.anchor_head_detections(*_one_level(keys), None, 4, 0.05, 0.5, 10)
    assert out[2][0, :4].tolist() == [6, 1, 2, 3] and out[3].tolist() == [4]    # score desc, then anchor asc
    # -0.0 ties with +0.0
    d = DD.dense(*_one_level(f32([-0.0, 0.0, -1, 0.0])), None, 2)
    assert d["anchor_idx"].tolist() == [0, 1]


@pytest.mark.parametrize("n", [5, 6, 7])
def test_level_sizes_around_nms_pre(n):
    keys = np.arange(n, dtype=f32)[::-1].copy()
    d = DD.dense(*_one_level(keys), None, 6)
    assert d["anchor_idx"].tolist() == list(range(min(n, 6)))      # n = 7 drops the lowest key, the last anchor
    assert DD.plan([n], 6) == ([min(n, 6)], [0], min(n, 6))
    assert DD.plan([n], 0)[2] == n


def test_score_equal_to_the_threshold_is_no_candidate():
    x = f32([0.0, 1.0, -1.0])
    thr = float(P.sigmoid(x)[0])                             # 0.5
    out = DD.anchor_head_detections(*_one_level(x), None, 0, thr, 0.5, 10)
    assert out[3].tolist() == [1] and out[2][0, 0] == 1
    below = float(np.nextafter(f32(thr), f32(0)))
    assert DD.anchor_head_detections(*_one_level(x), None, 0, below, 0.5, 10)[3].tolist() == [2]


def test_one_class_and_background_column():
    out = DD.anchor_head_detections(*_one_level(f32([2.0, -5.0, 0.5])), None, 0, 0.05, 0.5, 10)
    assert out[4].shape == (3, 2) and not out[4][:, 0].any()
    assert out[1][0, :2].tolist() == [0, 0] and out[3].tolist() == [2] and out[2][0, :2].tolist() == [0, 2]


def _hand_targets():
    # anchors: 0 = gt 0; 1 overlaps gt 1 with IoU 70 / 130; 2 far from both; 3 inside gt 0 with IoU 40 / 100 = neg_iou_thr:
    # ignored; 4 leaves the 64 x 64 image
    anchors = f32([[0, 0, 9, 9], [23, 20, 32, 29], [50, 50, 59, 59], [0, 0, 9, 3], [60, 60, 80, 80]])
    gt = f32([[[0, 0, 9, 9], [20, 20, 29, 29], [0, 0, 9, 4]], [[0, 0, 0, 0]] * 3])        # row 2 lies past gt_counts
    return anchors, gt


def test_targets_by_hand():
    anchors, gt = _hand_targets()
    labels = np.asarray([[7, 3, 5], [1, 1, 1]], np.int64)
    counts = np.asarray([2, 0], np.int32)
    shapes = np.asarray([(64, 64), (64, 64)], np.int32)
    info = {}
    out = DD.anchor_target_all(anchors, None, gt, labels, counts, shapes, 0.5, 0.4, 0.0, 0, info=info)
    lab, lw, bt, bw, npos, nneg, a = out
    iou = B.iou_pairwise(anchors, gt[0, :2])
    assert iou[1, 1] == f32(70) / f32(130) and iou[3, 0] == f32(0.4)   # positive; neither negative nor positive
    # image 0: anchor 0 positive (label 7), anchor 1 positive (label 3), 2 negative, 3 ignored, 4 outside the image
    assert a[0].tolist()[0] == 1 and a[0, 1] == 2 and a[0, 2] == 0 and a[0, 3] == -1 and a[0, 4] == -1
    assert lab[0].tolist() == [7, 3, 0, 0, 0] and lw[0].tolist() == [1, 1, 1, 0, 0]
    assert bw[0, :, 0].tolist() == [1, 1, 0, 0, 0] and not bt[0, 0].any() and bt[0, 1].any() and not bt[0, 2:].any()
    assert (npos[0], nneg[0]) == (2, 1)
    # image 1 has no ground truth: every participating anchor is negative
    assert a[1].tolist() == [0, 0, 0, 0, -1] and lab[1].tolist() == [0] * 5 and lw[1].tolist() == [1, 1, 1, 1, 0]
    assert (npos[1], nneg[1]) == (0, 4) and not bt[1].any() and not bw[1].any()
    assert info["outside"] == [1, 1] and info["ignored"] == [1, 0]
    # gt_labels = None: every positive gets 1
    lab1 = DD.anchor_target_all(anchors, None, gt, None, counts, shapes, 0.5, 0.4, 0.0, 0)[0]
    assert lab1[0].tolist() == [1, 1, 0, 0, 0]


def test_anchor_positive_only_through_step_6():
    anchors = f32([[0, 0, 9, 9], [25, 20, 34, 29], [50, 50, 59, 59]])       # IoU(anchor 1, gt 1) = 50 / 150
    gt = f32([[[0, 0, 9, 9], [20, 20, 29, 29]]])
    info = {}
    out = DD.anchor_target_all(anchors, None, gt, np.asarray([[4, 9]], np.int64), np.asarray([2], np.int32), None,
                               0.5, 0.4, 0.0, -1, info=info)
    iou = B.iou_pairwise(anchors, gt[0])
    assert 0 < iou[1, 1] < 0.4                                 # a negative by steps 4-5 ...
    assert info["only_step6"] == [1] and out[6][0].tolist() == [1, 2, 0] and out[0][0].tolist() == [4, 9, 0]
    # ... and it stays one when step 6 is held off by min_pos_iou
    out = DD.anchor_target_all(anchors, None, gt, None, np.asarray([2], np.int32), None, 0.5, 0.4, 0.45, -1)
    assert out[6][0].tolist() == [1, 0, 0] and out[4].tolist() == [1] and out[5].tolist() == [2]


# ---- host refusals, by message (CPU tensors: nothing here reaches the device check but its own case) ---------------
def _det_args(Bn=2, A=2, C=3, dtype=torch.float32):
    levels = [((3, 4), 8), ((2, 2), 16)]
    cls = [torch.zeros(Bn, A * C, h, w, dtype=dtype) for (h, w), _ in levels]
    reg = [torch.zeros(Bn, 4 * A, h, w, dtype=dtype) for (h, w), _ in levels]
    anchors = [torch.from_numpy(a) for a in K.pyramid(levels, A)]
    return cls, reg, anchors, torch.tensor([(30, 40)] * Bn, dtype=torch.int32)


def _refused(fn, msg, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert msg in str(e.value), str(e.value)


def test_detection_refusals(T):
    f = T.anchor_head_detections
    cls, reg, anc, ish = _det_args()
    _refused(f, "1..8 levels", [], [], anc, ish)
    _refused(f, "1..8 levels", cls * 5, reg * 5, anc, ish)
    _refused(f, "one cls_score / bbox_pred each", cls, reg[:1], anc, ish)
    _refused(f, "bbox_preds[0] must be a", cls, [reg[0][0]] + reg[1:], anc, ish)
    _refused(f, "4A channels", cls, [torch.zeros(2, 6, 3, 4)] + reg[1:], anc, ish)
    _refused(f, "A*C channels", [torch.zeros(2, 7, 3, 4)] + cls[1:], reg, anc, ish)
    _refused(f, "cls_scores[0] must be a", [cls[0].double()] + cls[1:], reg, anc, ish)
    _refused(f, "cls_scores[1] must be a", [cls[0], cls[1].half()], reg, anc, ish)
    _refused(f, "bbox_preds[1] must be a", cls, [reg[0], torch.zeros(2, 12, 2, 2)], anc, ish)
    _refused(f, "number of images must be in 1..64", *_det_args(Bn=65))
    big = _det_args(A=1, C=1024)
    _refused(f, "must be in 1..1023", *big)
    _refused(f, "anchors[1] must be a", cls, reg, [anc[0], anc[1][:-1]], ish)
    _refused(f, "anchors must be a", cls, reg, torch.cat(anc)[:-1], ish)
    _refused(f, "one tensor per level", cls, reg, anc[:1], ish)
    _refused(f, "img_shapes must be a", cls, reg, anc, ish.long())
    _refused(f, "img_shapes must be a", cls, reg, anc, [(30, 40)] * 2)
    _refused(f, "scale_factors must be a", cls, reg, anc, ish, torch.ones(3))
    _refused(f, "scale_factors must be finite and > 0", cls, reg, anc, ish, 0.0)
    _refused(f, "nms_pre must be in 0..4096", cls, reg, anc, ish, nms_pre=4097)
    _refused(f, "nms_pre must be in 0..4096", cls, reg, anc, ish, nms_pre=-1)
    _refused(f, "max_per_img must be in 1..8192", cls, reg, anc, ish, max_per_img=0)
    _refused(f, "max_per_img must be in 1..8192", cls, reg, anc, ish, max_per_img=8193)
    _refused(f, "score_thr must be finite", cls, reg, anc, ish, score_thr=float("nan"))
    _refused(f, "nms_thr must be finite", cls, reg, anc, ish, nms_thr=float("inf"))
    _refused(f, "wh_ratio_clip must be in (0, 1)", cls, reg, anc, ish, wh_ratio_clip=1.0)
    _refused(f, "target_stds must have 4 finite entries", cls, reg, anc, ish, target_stds=(1, 1, 1))
    _refused(f, "target_means must have 4 finite entries", cls, reg, anc, ish, target_means=(0, 0, 0, float("nan")))
    # B * K rows: 64 images of one 5000-anchor level, all kept
    c = [torch.zeros(64, 1, 50, 100)]
    r = [torch.zeros(64, 4, 50, 100)]
    _refused(f, "dense rows (max 262144)", c, r, [torch.zeros(5000, 4)], torch.zeros(64, 2, dtype=torch.int32), nms_pre=0)
    # a level of 2^31 logits or more (expanded tensors: no memory behind them)
    c = [torch.zeros(1, 1, 1, 1).expand(8, 1023, 512, 513)]
    r = [torch.zeros(1, 1, 1, 1).expand(8, 4, 512, 513)]
    _refused(f, "fewer than 2^31 elements", c, r, [torch.zeros(1, 4).expand(512 * 513, 4).contiguous()],
             torch.zeros(8, 2, dtype=torch.int32))
    # the device comes last
    _refused(f, "must be a CUDA tensor", cls, reg, anc, ish)


def test_target_refusals(T):
    f = T.anchor_target_all
    anchors = torch.zeros(10, 4)
    gt, lab, cnt = torch.zeros(2, 3, 4), torch.ones(2, 3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    ish = torch.zeros(2, 2, dtype=torch.int32)
    _refused(f, "gt_bboxes must be a", anchors, None, gt[0], lab, cnt, ish)
    _refused(f, "number of images must be in 1..64", anchors, None, torch.zeros(65, 3, 4), lab, cnt, ish)
    _refused(f, "ground truths per image (max 256)", anchors, None, torch.zeros(2, 257, 4), lab, cnt, ish)
    _refused(f, "gt_counts must be a", anchors, None, gt, lab, cnt.long(), ish)
    _refused(f, "anchors must be a", anchors[:, :3], None, gt, lab, cnt, ish)
    _refused(f, "anchors must be a", torch.zeros(3, 10, 4), None, gt, lab, cnt, ish)
    _refused(f, "at least one box", anchors[:0], None, gt, lab, cnt, ish)
    _refused(f, "valid_flags must be a", anchors, torch.ones(9, dtype=torch.uint8), gt, lab, cnt, ish)
    _refused(f, "valid_flags must be a", anchors, torch.ones(2, 10), gt, lab, cnt, ish)
    _refused(f, "gt_labels must be a", anchors, None, gt, lab.int(), cnt, ish)
    _refused(f, "gt_labels must be a", anchors, None, gt, lab[:, :2], cnt, ish)
    _refused(f, "img_shapes must be a", anchors, None, gt, lab, cnt, None, allowed_border=0)
    _refused(f, "img_shapes must be a", anchors, None, gt, lab, cnt, ish[:1])
    _refused(f, "pos_iou_thr must be finite", anchors, None, gt, lab, cnt, ish, pos_iou_thr=float("nan"))
    _refused(f, "neg_iou_thr must be a number", anchors, None, gt, lab, cnt, ish, neg_iou_thr=(0.1, 0.4))
    _refused(f, "target_stds must have 4 finite entries", anchors, None, gt, lab, cnt, ish, target_stds=(1, 1))
    _refused(f, "must be a CUDA tensor", anchors, None, gt, lab, cnt, ish)
    big = torch.zeros(1, 4).expand((1 << 20) + 1, 4)
    _refused(f, "anchors must be a", big, None, gt, lab, cnt, ish)            # not contiguous
    _refused(f, "boxes per image (max 1048576)", torch.zeros((1 << 20) + 1, 4), None, gt, lab, cnt, ish)


# ---- queries against the layout written out ---------------------------------------------------------------------------
def _a256(x):
    return (x + 255) // 256 * 256


def _nms_ws(N, C, Bn):
    """detect.hip's det_layout, written out: per segment row a box, a key, a row, a kept index; per segment three
    ints; per row `pitch` suppression words."""
    cap = min(max(N, 1), 4096)
    S = Bn * (C - 1)
    rows = S * cap
    pitch = (cap + 63) // 64
    return _a256(16 * rows) + _a256(4 * rows) * 2 + _a256(8 * rows) + 3 * _a256(4 * S) + _a256(8 * rows * pitch)


def _table(level_shapes, A, C, channels_last):
    from torch_detection_amd import _lib
    arr = (_lib.DenseLevel * len(level_shapes))()
    for l, (H, W) in enumerate(level_shapes):
        arr[l].H, arr[l].W = H, W
        arr[l].cls_strides[:] = [A * C * H * W, 1, W * A * C, A * C] if channels_last else [A * C * H * W, H * W, W, 1]
        arr[l].reg_strides[:] = [4 * A * H * W, H * W, W, 1]
    return arr


@pytest.mark.parametrize("Bn,C,nms_pre,channels_last", [(1, 80, 1000, True), (2, 80, 1000, False), (3, 5, 100, True),
                                                        (2, 1, 0, True), (1, 1023, 4096, True)])
def test_detection_plan_and_workspace_queries(T, Bn, C, nms_pre, channels_last):
    from torch_detection_amd import _lib
    lib = _lib.load()
    A = 9
    shapes = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)] if C == 80 else [(8, 12), (4, 6), (2, 3), (1, 1)]
    sizes = [h * w * A for h, w in shapes]
    k, off, Ktot = DD.plan(sizes, nms_pre)
    cfg = _lib.DenseConfig()
    cfg.dtype, cfg.num_anchors, cfg.num_classes, cfg.nms_pre, cfg.max_num = _lib.TDN_BF16, A, C, nms_pre, 100
    cfg.wh_ratio_clip, cfg.score_thr, cfg.nms_thr = 16 / 1000, 0.05, 0.5
    arr = _table(shapes, A, C, channels_last)
    out = (ctypes.c_int32 * 16)()
    assert lib.tdn_dense_detections_plan(arr, len(shapes), Bn, ctypes.byref(cfg), out) == 0, lib.tdn_last_error()
    selecting = [n > kk for n, kk in zip(sizes, k)]
    # anchors per workgroup of the class-maximum launch: a 8192-float tile of rows of odd pitch, at most 256
    ta = min(256, 8192 // (C | 1)) if channels_last else 256
    groups = sum(Bn * -(-n // ta) for n, s in zip(sizes, selecting) if s)
    key_words = Bn * sum((n + 3) // 4 * 4 for n in sizes) if any(selecting) else 0
    assert list(out)[:8] == [Ktot, Bn * Ktot, sum(sizes), 7 if any(selecting) else 6, groups, sum(selecting),
                             key_words, 0]
    assert list(out)[8:8 + len(shapes)] == k
    # the launch count depends on none of B, the number of levels and C
    assert out[3] == (7 if any(selecting) else 6)
    want = _a256(4 * key_words) + _nms_ws(Bn * Ktot, C + 1, Bn)
    assert lib.tdn_dense_detections_workspace_bytes(arr, len(shapes), Bn, ctypes.byref(cfg)) == want
    assert lib.tdn_multiclass_nms_workspace_bytes(Bn * Ktot, C + 1, Bn) == _nms_ws(Bn * Ktot, C + 1, Bn)
    # the public query says the same
    p = T.anchor_head_detections_plan(shapes, Bn, A, C, nms_pre)
    assert (p["K"], p["rows"], p["launches"], p["kept"]) == (Ktot, Bn * Ktot, out[3], k)
    if not channels_last:
        assert p["key_workgroups"] == groups and p["key_words"] == key_words


def test_detection_queries_refuse_in_c(T):
    from torch_detection_amd import _lib
    lib = _lib.load()
    cfg = _lib.DenseConfig()
    cfg.dtype, cfg.num_anchors, cfg.num_classes, cfg.nms_pre, cfg.max_num = _lib.TDN_F32, 9, 5, 100, 100
    cfg.wh_ratio_clip, cfg.score_thr, cfg.nms_thr = 16 / 1000, 0.05, 0.5
    arr = _table([(8, 12)], 9, 5, True)
    out = (ctypes.c_int32 * 16)()
    ok = lambda B=2, L=1: lib.tdn_dense_detections_workspace_bytes(arr, L, B, ctypes.byref(cfg))
    assert ok() > 0
    for field, bad, msg in (("num_classes", 1024, b"C=1024 out of 1..1023"), ("num_anchors", 0, b"A=0"),
                            ("nms_pre", 4097, b"nms_pre=4097 out of 0..4096"), ("max_num", 8193, b"max_num=8193"),
                            ("max_num", 0, b"max_num=0"), ("score_thr", float("nan"), b"must be finite"),
                            ("wh_ratio_clip", 1.5, b"wh_ratio_clip must be in (0, 1)"), ("dtype", 7, b"dtype 7")):
        keep = getattr(cfg, field)
        setattr(cfg, field, bad)
        assert ok() == -1 and msg in lib.tdn_last_error(), (field, lib.tdn_last_error())
        setattr(cfg, field, keep)
    assert ok(B=65) == -1 and b"B=65 out of 1..64" in lib.tdn_last_error()
    assert ok(L=9) == -1 and b"9 levels (1..8)" in lib.tdn_last_error()
    assert lib.tdn_dense_detections_plan(arr, 1, 2, ctypes.byref(cfg), None) == -1
    huge = _table([(512, 513)], 9, 5, True)
    cfg.nms_pre = 0
    assert lib.tdn_dense_detections_workspace_bytes(huge, 1, 1, ctypes.byref(cfg)) == -1
    assert b"dense rows" in lib.tdn_last_error()
    cfg.nms_pre, cfg.num_classes = 100, 1023
    assert lib.tdn_dense_detections_workspace_bytes(huge, 1, 1, ctypes.byref(cfg)) == -1
    assert b"2^31 or more" in lib.tdn_last_error()
    with pytest.raises(ValueError, match="lower nms_pre"):
        T.anchor_head_detections_plan([(512, 513)], 1, 9, 5, 0)


@pytest.mark.parametrize("Bn,N,G", [(1, 1, 0), (2, 1134, 4), (3, 201600, 100), (64, 1 << 20, 256)])
def test_target_workspace_query(T, Bn, N, G):
    from torch_detection_amd import _lib
    lib = _lib.load()
    words = (Bn * max(G, 1) + 1) // 2 * 2 + 2 * Bn           # column maxima (even), then one 64-bit count word per image
    assert lib.tdn_anchor_target_all_workspace_bytes(Bn, N, G) == 2 * _a256(4 * words)   # and as many first-indices
    assert lib.tdn_anchor_target_all_workspace_bytes(Bn, 0, G) == -1 and b"boxes per image" in lib.tdn_last_error()
    assert lib.tdn_anchor_target_all_workspace_bytes(Bn, N, 257) == -1
    assert lib.tdn_anchor_target_all_workspace_bytes(65, N, G) == -1


def test_new_struct_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of the structs this section adds to include/tdn.h as gcc lays them out == the ctypes mirrors."""
    from torch_detection_amd import _lib
    mirrors = {"tdn_dense_level": _lib.DenseLevel, "tdn_dense_config": _lib.DenseConfig}
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
    assert "#define TDN_DENSE_MAX_LEVELS %d\n" % _lib.DENSE_MAX_LEVELS in hdr


# ---- the GPU tests' cases are not hollow (their conditions hold on the oracle, whatever device runs them) -----------
def test_the_shared_cases_reach_both_sides():
    cls, reg = K.head_case(K.LEVELS, 2, 9, 5, torch.float32, "nchw", 11)
    info, st = {}, {}
    out = DD.anchor_head_detections(K.stored(cls), K.stored(reg), K.pyramid(K.LEVELS), K.img_shapes(2), None, 100,
                                    0.05, 0.5, 100, K.MEANS, K.STDS, info=info, stats=st)
    assert any(c["above"] > 0 and c["ties"] > c["taken"] for c in info["cuts"]), info
    assert min(st["total"]) > 100 and out[3].tolist() == [100, 100]
    tc = K.target_case(0)
    ti = {}
    t = DD.anchor_target_all(tc["anchors"], tc["valid"], tc["gt_bboxes"], tc["gt_labels"], tc["gt_counts"],
                             tc["img_shapes"], allowed_border=0, info=ti)
    assert t[4][0] > 0 and t[5][0] > 0 and ti["ignored"][0] > 0 and ti["only_step6"][0] >= 1, (t[4], t[5], ti)
