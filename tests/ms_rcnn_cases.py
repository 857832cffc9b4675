"""Inputs and bounds shared by tests/test_ms_rcnn_oracle.py (CPU) and tests/test_gpu_ms_rcnn.py: built once per shape,
never modified.

Bounds, in units of u = 2^-24 of the sum of the absolute terms, counted as DESIGN.md §4g counts them (sigma 5u, every
``__f*_rn`` operation u, an add to an exact 0 nothing), each with one unit on top for the second-order terms:

  K_A = 15        a[co] = sum_9 w P: P carries sigma's 5, the product 1, the nine adds 8 (the first is to 0);
  K_DPRED(Cout)   dP = sum_taps sum_co w gz: the product 1, a lane's Cout / 64 adds Cout / 64 - 1, the xor tree 6, the
                  taps 8; then dP sigma(x) sigma(-x): 5 + 5 + the two products 2 -> 26 + Cout / 64, and the one on top;
  K_DW1 = 8       dw1 = sum gz P: P's 5, the fp32 product 1, the fp64 sums nothing visible, the store to fp32 1;
  K_IOU_LOSS = 4  (p - t)^2: the difference 1 (twice in the square), the product 1, the fp64 sum and quotient nothing
                  visible (the store to fp32 is granted separately);
  K_IOU_GRAD = 5  (p - t) ((2 lw g) / D): 2 lw exact, the product with g 1, the quotient 1, the difference 1, the
                  product 1.
A 16-bit output is granted one ulp of its type on top.
"""
import functools

import numpy as np

import mask_cases as MC
import mask_ref as MR

F32 = np.float32
U = 2.0 ** -24
K_A = 15
K_DW1 = 8
K_IOU_LOSS = 4
K_IOU_GRAD = 5


def K_DPRED(Cout):
    return 27 + Cout // 64


# ---- the target ------------------------------------------------------------------------------------------------------
CANVASES = np.array([[360, 520], [200, 260]], np.int32)
TARGET_C = 5
DEN0_ROW, FULL0_ROW = 19, 23            # the instance without polygons (its logits below thr), the padded slot
BAD_LABEL_ROWS = (4, 12)


@functools.lru_cache(maxsize=None)
def target_case(M, C=TARGET_C):
    """(rois, gt_inds, mask_targets (40, M, M) uint8, pred (40, C, M, M) float32, labels (40,) int64) on
    ``mask_cases.target_rows(M)``: logits of +-2 by the target plus N(0, 2.5) noise on the label's channel; NaN logits on
    every invalid row and on the rows whose label has no channel."""
    g = np.random.default_rng(900 + M + C)
    rois, inds = MC.target_rows(M)
    xy, po, gpo = (t.numpy() for t in _packed())
    targets, weights = MR.mask_target(rois, inds, xy, po, gpo, M)
    R = rois.shape[0]
    labels = g.integers(1, max(C, 2), R).astype(np.int64)
    pred = g.normal(0, 2.5, (R, C, M, M)).astype(F32)
    ch = labels if C > 1 else np.zeros(R, np.int64)
    for r in range(R):
        pred[r, ch[r]] += np.where(targets[r] == 1, F32(2), F32(-2))
    pred[DEN0_ROW] = -3
    labels[BAD_LABEL_ROWS[0]], labels[BAD_LABEL_ROWS[1]] = 0, C
    dead = weights == 0
    if C > 1:
        dead[list(BAD_LABEL_ROWS)] = True
    pred[dead] = np.nan
    for a in (rois, inds, targets, pred, labels):
        a.setflags(write=False)
    return rois, inds, targets, pred, labels


@functools.lru_cache(maxsize=None)
def _packed():
    import torch_detection_amd as T
    return T.pack_polygons(MC.target_polys(), MC.G)


def packed_polys():
    return _packed()


def word_case(w, h=5):
    """One image of canvas (h, w), one rectangle-with-a-notch instance that spans the canvas, and boxes that start and
    end on the 64-pixel word boundaries, off every edge, reversed, saturating and NaN: (polys, rois, gt_inds, img_shapes).
    Vertices on half-integers put crossings exactly on pixel centres (the strict < decides)."""
    x_hi = w + 0.5 if w % 2 else w - 0.5           # past the canvas, or exactly on the last pixel's centre
    poly = [0.5, 0.25, x_hi, 0.25, x_hi, h - 0.75, (w / 2.0), h / 2.0, 0.5, h - 0.75]
    polys = [[[[float(v) for v in poly]]]]
    edges = sorted({0, 1, 62, 63, 64, 65, 127, 128, 129, w - 2, w - 1, w, w + 1})
    boxes = []
    for x1 in edges:
        for x2 in edges:
            boxes.append([x1, 0, x2, h - 1])
    boxes += [[-5, -3, w + 5, h + 5], [-70, 1, 3, 2], [w - 2, h - 2, w + 70, h + 70], [3, 3, 1, 1], [0, h, w, h + 3],
              [w, 0, w + 3, h], [-9, -9, -1, -1], [3e9, -3e9, 3e9, 3e9], [-3e9, -3e9, 3e9, 3e9],
              [np.nan, 0, w, h], [0, np.nan, np.nan, np.nan], [0.9, 0.9, 1.1, 1.1]]
    rois = np.zeros((len(boxes), 5), F32)
    rois[:, 1:] = np.array(boxes, F32)
    return polys, rois, np.zeros(len(boxes), np.int32), np.array([[h, w]], np.int32)


# ---- the loss and the scores -------------------------------------------------------------------------------------------
def loss_case(R, C, seed, none_live=False):
    """(pred (R, C) float32, labels int64, targets float32): NaN / Inf predictions and out-of-range labels on the rows
    that are not live."""
    g = np.random.default_rng(seed)
    pred = g.normal(0.4, 0.5, (R, C)).astype(F32)
    labels = g.integers(1, max(C, 2), R).astype(np.int64)
    targets = np.where(g.random(R) < 0.6, g.uniform(0.001, 0.95, R), 0).astype(F32)
    if R > 2:
        targets[0], targets[1], targets[2] = 0.5, 0, -0.25
    if none_live:
        targets[:] = 0
    bad = g.random(R) < 0.15
    if R > 3:
        bad[3] = True
        targets[3] = 0.7
    bad &= ~((np.arange(R) == 0))
    labels[bad] = g.choice(np.array([-7, 0, C, 1 << 40], np.int64), int(bad.sum()))
    dead = ~((targets > 0) & (labels >= 1) & (labels < C))
    pred[dead] = g.choice(np.array([np.nan, np.inf, -np.inf], F32), (int(dead.sum()), C))
    nan_t = dead & (g.random(R) < 0.2) & (np.arange(R) > 3)
    targets[nan_t] = np.nan
    return pred, labels, targets


def scores_case(C, seed=7):
    """(pred (B N, C), dets (B, N, 5), labels (B, N), counts): B = 3, N = 6; an empty image, a full one, the overflow
    marker; labels without a column (-2, C - 1, huge); label -1 reads column 0."""
    g = np.random.default_rng(seed)
    B, N = 3, 6
    pred = g.normal(0.5, 0.3, (B * N, C)).astype(F32)
    dets = g.random((B, N, 5)).astype(F32)
    labels = g.integers(0, max(C - 1, 1), (B, N)).astype(np.int64)
    labels[1, 0], labels[1, 1], labels[1, 2], labels[1, 3] = -2, C - 1, 1 << 40, -1
    counts = np.array([0, N, -1], np.int32)
    return pred, dets, labels, counts


# ---- the first layer ---------------------------------------------------------------------------------------------------
def stem_case(S, C, seed, R=7, Cf=64, Cout=64):
    """float32 arrays (feats (R, Cf, S, S), pred (R, C, 2S, 2S), labels, weight (Cout, Cf + 1, 3, 3), bias, gy): labels
    for ``label_offset`` 0; rows 2 and 5 have labels without a channel (when C > 1) and NaN logits; planted ties: row 0's
    first window is all +40, its last all -40, and row 1's first window holds its maximum at its second AND third place."""
    g = np.random.default_rng(seed)
    M = 2 * S
    feats = g.normal(0, 1, (R, Cf, S, S)).astype(F32)
    pred = np.clip(g.normal(0, 2.5, (R, C, M, M)), -9, 9).astype(F32)
    labels = g.integers(1, max(C, 2), R).astype(np.int64)
    weight = (g.normal(0, 1, (Cout, Cf + 1, 3, 3)) / np.sqrt(9 * (Cf + 1))).astype(F32)
    weight[:, Cf] *= 4                                  # the mask channel's share is visible in the output
    bias = g.normal(0, 0.1, Cout).astype(F32)
    gy = g.normal(0, 1, (R, Cout, S, S)).astype(F32)
    ch = labels if C > 1 else np.zeros(R, np.int64)
    pred[0, ch[0], 0:2, 0:2] = 40
    pred[0, ch[0], M - 2:, M - 2:] = -40
    pred[1, ch[1], 0:2, 0:2] = np.array([[-1.0, 2.5], [2.5, 0.5]], F32)
    if C > 1:
        labels[2], labels[5] = 0, C
        pred[[2, 5]] = np.nan
    return feats, pred, labels, weight, bias, gy
