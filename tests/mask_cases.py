"""Inputs shared by tests/test_mask_oracle.py (CPU) and tests/test_gpu_mask.py: built once per shape, never modified.

Bounds (DESIGN.md §4g derives them): K_LOSS = 16 units of 2^-24 for the loss and its gradient (§4e's BCE count plus
the divisor's extra rounding: 9 and 6 units, under the 16 that §4e states), K_PASTE = 11 units for the interpolated
probability of the paste.
"""
import functools

import numpy as np

F32 = np.float32
K_LOSS = 16
K_PASTE = 11
U = 2.0 ** -24


def star(cx, cy, r0, r1, n, seed, integer=False):
    """A star-shaped polygon of n vertices around (cx, cy), radii in [r0, r1]: simple, usually concave."""
    g = np.random.default_rng(seed)
    ang = np.sort(g.uniform(0, 2 * np.pi, n))
    rad = g.uniform(r0, r1, n)
    p = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1)
    return (np.round(p) if integer else p).astype(F32)


def flat(poly):
    return [float(v) for v in np.asarray(poly).reshape(-1)]


# the exact-arithmetic instance: integer vertices, concave
EXACT_POLY = np.array([[100, 40], [212, 40], [212, 152], [170, 152], [156, 96], [142, 152], [100, 152]], F32)
G = 3


@functools.lru_cache(maxsize=None)
def target_polys():
    """gt_mask_polys of a batch of two: image 0 has three instances (a 700-vertex star; two disjoint parts; three
    overlapping parts), image 1 two (one without polygons; the exact-arithmetic one) and one padded slot."""
    img0 = [[flat(star(200, 150, 60, 110, 700, 1))],
            [flat(star(90, 300, 20, 40, 9, 2)), flat(star(190, 310, 15, 45, 14, 3))],
            [flat(star(400, 200, 30, 70, 11, 4)), flat(star(430, 220, 30, 60, 5, 5)), flat(star(410, 180, 10, 30, 3, 6))]]
    img1 = [[], [flat(EXACT_POLY)]]
    return [img0, img1]


def _bbox(polys):
    pts = np.concatenate([np.asarray(p, F32).reshape(-1, 2) for p in polys], 0)
    return pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()


@functools.lru_cache(maxsize=None)
def target_rows(M):
    """(rois (40, 5) float32, gt_inds (40,) int32) over ``target_polys()``: boxes around, partly off and wholly off
    their instance, the invalid rows (b = -1, b = B, b = NaN, g = -1, g = G), NaN coordinates, the polygon-free
    instance, the padded slot, and the exact-arithmetic boxes (w, h multiples of 2M on integer corners)."""
    g = np.random.default_rng(40 + M)
    polys = target_polys()
    rois = np.zeros((40, 5), F32)
    inds = np.zeros(40, np.int32)
    for r in range(40):
        b = r % 2
        gi = int(g.integers(0, 3)) if b == 0 else 1
        x1, y1, x2, y2 = _bbox(polys[b][gi])
        w, h = x2 - x1, y2 - y1
        kind = r % 5
        if kind == 0:                                   # around the instance, fractional corners
            box = [x1 - g.uniform(0, 9), y1 - g.uniform(0, 9), x2 + g.uniform(0, 9), y2 + g.uniform(0, 9)]
        elif kind in (1, 2):                            # partly off
            dx, dy = g.uniform(-0.7, 0.7, 2) * (w, h)
            box = [x1 + dx, y1 + dy, x2 + dx - g.uniform(0, 0.3) * w, y2 + dy]
        elif kind == 3:                                 # wholly off
            box = [x2 + 20, y2 + 20, x2 + 20 + w, y2 + 20 + h]
        else:                                           # small, inside
            cx, cy = (x1 + x2) / 2, (y1 + y2) / 2
            box = [cx - 3.5, cy - 2.5, cx + g.uniform(0, 6), cy + g.uniform(0, 6)]
        rois[r] = [b] + box
        inds[r] = gi
    # the exact-arithmetic rows: image 1, instance 1
    for r, (x, y, kw, kh) in zip((1, 11, 21, 31), ((100, 40, 2, 2), (72, 12, 4, 2), (156, 96, 2, 4), (44, 40, 4, 4))):
        rois[r] = [1, x, y, x + kw * 2 * M - 1, y + kh * 2 * M - 1]
        inds[r] = 1
    rois[3, 0] = -1
    rois[5, 0] = 2
    rois[7, 0] = np.nan
    inds[9] = -1
    inds[13] = G
    rois[15, 1:] = np.nan
    rois[17, 3] = np.nan                                # x2 -> 0: w = 1
    rois[19] = [1, 100, 40, 211, 151]
    inds[19] = 0                                        # the instance without polygons
    rois[23] = [1, 100, 40, 211, 151]
    inds[23] = 2                                        # the padded slot
    rois[25, 1:] = [3e9, -3e9, 3e9, 3e9]                # saturating truncation
    return rois, inds


EXACT_ROWS = (1, 11, 21, 31)


def loss_case(R, C, M, seed, all_zero=False):
    """(pred (R, C, M, M) float32, targets uint8, labels int64, weights float32): NaN / Inf logits and out-of-range
    labels on the rows of weight 0."""
    g = np.random.default_rng(seed)
    pred = np.clip(g.normal(0, 2.5, (R, C, M, M)), -9, 9).astype(F32)
    targets = (g.random((R, M, M)) < 0.4).astype(np.uint8)
    labels = g.integers(1, max(C, 2), R).astype(np.int64)
    w = g.choice(np.array([0, 1, 0.5], F32), R, p=[0.3, 0.5, 0.2])
    w[0], w[1] = 1, 0
    if all_zero:
        w[:] = 0
    dead = w == 0
    pred[dead] = g.choice(np.array([np.nan, np.inf, -np.inf], F32), (int(dead.sum()), C, M, M))
    labels[dead] = g.choice(np.array([-7, 0, C, 1 << 40], np.int64), int(dead.sum()))
    return pred, targets, labels, w


CANVAS = (70, 150)
PASTE_B, PASTE_N = 2, 6
PASTE_DETS = np.array([
    [[20.3, 10.9, 60.2, 40.5, 0.9],                     # inside
     [5, 5, 5, 5, 0.8],                                 # w = h = 1
     [30, 20, 25, 15, 0.7],                             # x2 < x1, y2 < y1: w = h = 1
     [-10.5, -7.2, 30, 25, 0.6],                        # over the left and top edges
     [120, 50, 170.8, 90.1, 0.5],                       # over the right and bottom edges
     [-20, -20, 200, 100, 0.4]],                        # over every edge
    [[10, 10, 120, 60, 0.9],                            # clipped by the image's own size
     [0, 0, 149, 69, 0.8],                              # the canvas exactly
     [90.5, 40.2, 99.9, 49.9, 0.7],                     # up to the image's last pixel
     [np.nan, 5, 20, 30, 0.6],                          # NaN truncates to 0
     [10, 10, 40, 40, 0.5],                             # past counts[1]: ignored
     [3e9, 3e9, -3e9, np.nan, 0.4]]], F32)
PASTE_COUNTS = np.array([6, 4], np.int32)
PASTE_LABELS = np.array([[0, 1, 2, 0, 1, 2], [2, 1, 3, 0, 1, 2]], np.int64)     # 3 is outside a C = 4 head
PASTE_IMG_SHAPES = np.array([[70, 150], [50, 100]], np.int32)


@functools.lru_cache(maxsize=None)
def paste_pred(C, M, seed=0):
    """(B*N, C, M, M) float32 logits, smooth enough to give blobs and rough enough to cross the threshold often."""
    g = np.random.default_rng(100 * C + M + seed)
    coarse = g.normal(0, 2.0, (PASTE_B * PASTE_N, C, (M + 3) // 4, (M + 3) // 4))
    up = np.repeat(np.repeat(coarse, 4, 2), 4, 3)[:, :, :M, :M]
    out = (up + g.normal(0, 0.7, (PASTE_B * PASTE_N, C, M, M))).astype(F32)
    out.setflags(write=False)
    return out


def box_pixels(v):
    """Pixels inside the clipped boxes of a ``mask_ref.mask_head_masks`` value array."""
    return int(np.isfinite(v).sum())


def near_threshold(v, thr, K=K_PASTE):
    with np.errstate(invalid="ignore"):
        return np.abs(v - float(F32(thr))) <= K * U
