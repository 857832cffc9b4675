"""Shared inputs of the Guided Anchoring tests (tests/test_ga_oracle.py on the CPU, tests/test_gpu_guided.py on the
GPU): the two pyramids, ground truths with the planted boxes of DESIGN.md §4w, approximating and square anchors with
planted ties, and head outputs with the planted rows of the loss.  numpy only."""
import numpy as np

f32 = np.float32

SMALL = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]          # Nloc = 512
BIG = [(40, 52), (20, 26), (10, 13), (5, 7), (3, 4)]         # Nloc = 2777: past the assign passes' 1024, no multiple
STRIDES = [4, 8, 16, 32, 64]
ANCHOR_SCALE = 1.5           # m = 6: t_k = 72, 288, 1152, 4608
SQUARE_SCALE = 4             # the square of a location has side 4 * stride
MAX_GT = 256


def nloc(sizes):
    return int(sum(h * w for h, w in sizes))


def extent(sizes):
    return sizes[0][0] * STRIDES[0], sizes[0][1] * STRIDES[0]


# The planted ground truths, in this order at the head of image 0 (all inside the 64 x 96 extent of SMALL):
PLANTED = np.array([
    [10, 10, 13, 13],        # lowest level: no lower neighbour
    [5, 0, 90, 63],          # 86 x 64 = 5504 >= 4608: highest level, no upper neighbour, every region clamped
    [20, 20, 27, 28],        # 8 x 9 = 72 = t_1 exactly: the upper level
    [40, 40, 42, 42],        # a centre region of one pixel
    [0, 0, 8, 6],            # level 0, stride 4, ignore_ratio 0.5: x1 = 0.5 -> 0, x2 = 1.5 -> 2
    [30, 30, 41, 41],        # level 1 ...
    [38, 30, 53, 46],        # ... and a later box of level 1 whose ignore region erases part of that one's centre
], f32)


def gt_case(Bn, Gn, counts, seed, sizes, planted=True):
    """(gt (B, G, 4) float32 with zero rows past counts, counts (B,) int32)."""
    g = np.random.default_rng(seed)
    Hh, Ww = extent(sizes)
    gt = np.zeros((Bn, Gn, 4), f32)
    for b in range(Bn):
        n = int(counts[b])
        side = np.exp(g.uniform(np.log(4), np.log(min(Hh, Ww)), (n, 2)))
        x1 = g.uniform(0, 1, n) * np.maximum(Ww - side[:, 0], 1)
        y1 = g.uniform(0, 1, n) * np.maximum(Hh - side[:, 1], 1)
        bx = np.stack([x1, y1, x1 + side[:, 0], y1 + side[:, 1]], 1)
        bx[::2] = np.round(bx[::2])                       # every other box on integers
        gt[b, :n] = bx.astype(f32)
        if planted and b == 0:
            k = min(n, PLANTED.shape[0])
            gt[b, :k] = PLANTED[:k]
    return gt, np.asarray(counts, np.int32)


def squares_of(sizes):
    """(Nloc, 4) float32 integer-valued squares of side SQUARE_SCALE * stride, centred as the anchor generator does."""
    out = []
    for (H, W), s in zip(sizes, STRIDES):
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        cx, cy = xs.reshape(-1) * s + (s - 1) / 2.0, ys.reshape(-1) * s + (s - 1) / 2.0
        h = (SQUARE_SCALE * s - 1) / 2.0
        out.append(np.stack([cx - h, cy - h, cx + h, cy + h], 1))
    return np.concatenate(out).astype(f32)


def approxs_of(sizes, A):
    """(Nloc, A, 4) float32: A = 1 the square itself, 3 the ratios (0.5, 1, 2), 9 those at three octave scales."""
    sq = squares_of(sizes).astype(np.float64)
    if A == 1:
        return sq[:, None].astype(f32)
    cx, cy, side = (sq[:, 0] + sq[:, 2]) / 2, (sq[:, 1] + sq[:, 3]) / 2, sq[:, 2] - sq[:, 0] + 1
    scales = [1.0] if A == 3 else [1.0, 2 ** (1 / 3), 2 ** (2 / 3)]
    out = []
    for sc in scales:
        for ratio in (0.5, 1.0, 2.0):
            w, h = side * sc / np.sqrt(ratio), side * sc * np.sqrt(ratio)
            out.append(np.stack([cx - (w - 1) / 2, cy - (h - 1) / 2, cx + (w - 1) / 2, cy + (h - 1) / 2], 1))
    return np.stack(out, 1).astype(f32)


def shape_case(sizes, A, Bn, Gn, counts, seed, per_image_flags):
    """approxs with planted ties, squares, flags with a location that takes part through a single approx, ground truths
    of which some coincide with approxs, image shapes that leave border locations outside, and keys."""
    g = np.random.default_rng(seed)
    N = nloc(sizes)
    approxs, squares = approxs_of(sizes, A), squares_of(sizes)
    Hh, Ww = extent(sizes)
    mid = (sizes[0][0] // 2) * sizes[0][1] + sizes[0][1] // 2          # a location in the middle of level 0
    if A > 1:
        approxs[mid + 3, 1] = approxs[mid + 3, 0]                      # two approxs of one location tie
    approxs[mid + 5] = approxs[mid + 4]                                # two locations tie on every ground truth
    squares[mid + 5] = squares[mid + 4]
    gt, cn = gt_case(Bn, Gn, counts, seed + 100, sizes, planted=False)
    for b in range(Bn):
        n = int(cn[b])
        pick = g.integers(0, N, n)
        for j in range(0, n, 2):                                       # every other one sits near an approx
            gt[b, j] = approxs[pick[j], g.integers(0, A)] + g.integers(-2, 3, 4).astype(f32)
        if n > 1:
            gt[b, 1] = approxs[mid + 4, 0]                             # IoU 1 with the two tied locations
        if n > 3 and A > 1:
            gt[b, 3] = approxs[mid + 3, 0]
    flags = (g.uniform(0, 1, (Bn, N * A)) < 0.9).astype(np.uint8)
    flags[:, (mid + 7) * A:(mid + 8) * A] = 0
    flags[:, (mid + 7) * A] = 1                                        # takes part through its first approx only
    # location 0 (the top-left corner: every approx reaches outside the image) with every flag set and its first approx
    # moved inside: it takes part through a single INSIDE approx
    approxs[0, 0] = squares[0] = np.array([1, 1, 12, 12], f32)
    flags[:, 0:A] = 1
    if not per_image_flags:
        flags = flags[0]
    img_shapes = np.array([[Hh - 4 - 3 * b, Ww - 6 + b] for b in range(Bn)], np.int32)
    keys = g.integers(0, 1 << 20, (Bn, N)).astype(np.int32)
    keys[:, ::3] = 7                                                   # plenty of key ties
    return dict(approxs=approxs, squares=squares, flags=flags, gt=gt, counts=cn, img_shapes=img_shapes, keys=keys)


# ---- head outputs -----------------------------------------------------------------------------------------------------------
def stored(a, dtype):
    """The float32 values a tensor of ``dtype`` ('f32', 'bf16', 'f16') holds after storing ``a``."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=f32))
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    return t.to(dt).to(torch.float32).numpy()


def head_case(sizes, Bn, dtype, seed, scale=2.0):
    """loc_preds [(B, 1, H, W)], shape_preds [(B, 2, H, W)]: float32 arrays holding values ``dtype`` stores exactly."""
    g = np.random.default_rng(seed)
    loc = [stored(g.normal(0, 3.0, (Bn, 1, h, w)), dtype) for h, w in sizes]
    shape = [stored(g.normal(0, scale, (Bn, 2, h, w)), dtype) for h, w in sizes]
    return loc, shape


def loss_case(sizes, Bn, dtype, seed, rows_per_image, zero_weights=False):
    """Head outputs and targets of a loss call with the planted rows of §4w: image 1 (if there is one) has no rows;
    row 0 of image 0 is the ``min`` tie (zero shape output, a ground truth of the anchor's size), row 1 has dw beyond the
    clip (below it; with an odd seed above it, where the decoded box is 10^6 wide and the centre term ill-conditioned), row 2 a ground truth so far off that the centre term is clamped at 0; the others lie on both sides of beta."""
    g = np.random.default_rng(seed)
    N = nloc(sizes)
    loc, shape = head_case(sizes, Bn, dtype, seed)
    sq = squares_of(sizes)
    an, gts, bw = np.zeros((Bn, N, 4), f32), np.zeros((Bn, N, 4), f32), np.zeros((Bn, N, 4), f32)
    off = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])])
    planted = {}
    for b in range(Bn):
        if b == 1:
            continue
        idx = np.sort(g.choice(N, rows_per_image, replace=False))
        an[b, idx] = sq[idx]
        side = (sq[idx, 2] - sq[idx, 0] + 1)[:, None]
        fac = np.exp(g.uniform(-1.0, 1.0, (rows_per_image, 2)))
        ctr = (sq[idx, :2] + sq[idx, 2:]) / 2 + g.uniform(-0.3, 0.3, (rows_per_image, 2)) * side
        wh = side * fac
        gts[b, idx] = np.concatenate([ctr - (wh - 1) / 2, ctr + (wh - 1) / 2], 1).astype(f32)
        bw[b, idx] = 1
        if b == 0:
            i0, i1, i2 = idx[:3]
            gts[b, i0] = sq[i0] + f32(3)                              # the anchor's size, shifted by integers
            gts[b, i2] = sq[i2] + f32(2) * (sq[i2, 2] - sq[i2, 0] + 1)
            planted = dict(tie=int(i0), clip=int(i1), far=int(i2))
            for i, vals in ((i0, (0.0, 0.0)), (i1, (120.0 if seed % 2 else -120.0, -120.0))):
                l = int(np.searchsorted(off, i, side="right") - 1)
                p = i - off[l]
                W = sizes[l][1]
                shape[l][b, :, p // W, p % W] = vals
    lt = (g.uniform(0, 1, (Bn, N)) < 0.1).astype(np.int64)
    lw = g.choice(np.array([0, 0.1, 1], f32), (Bn, N), p=[0.2, 0.6, 0.2]).astype(f32)
    lw[lt == 1] = 1
    if zero_weights:
        lw[:] = 0
    return dict(loc=loc, shape=shape, loc_targets=lt, loc_weights=lw, bbox_anchors=an, bbox_gts=gts, bbox_weights=bw,
                planted=planted)


def poison_unread(case):
    """NaN / Inf on every element no rule of the loss reads: location logits of weight 0, shape outputs, anchors and
    ground truths off the rows.  Returns a deep copy."""
    c = {k: ([v.copy() for v in case[k]] if isinstance(case[k], list) else
             (case[k].copy() if isinstance(case[k], np.ndarray) else case[k])) for k in case}
    n0 = 0
    row = c["bbox_weights"][..., 0] > 0
    for l, lp in enumerate(c["loc"]):
        Bn, _, H, W = lp.shape
        n1 = n0 + H * W
        dead = (c["loc_weights"][:, n0:n1] == 0).reshape(Bn, 1, H, W)
        lp[dead] = np.nan
        off = ~row[:, n0:n1].reshape(Bn, 1, H, W)
        c["shape"][l][np.broadcast_to(off, c["shape"][l].shape)] = np.inf
        n0 = n1
    c["bbox_anchors"][~row] = np.nan
    c["bbox_gts"][~row] = np.nan
    c["bbox_weights"][~row, 1:] = np.nan
    return c


def proposal_case(sizes, Bn, dtype, seed, mask_kind):
    """cls_scores [(B, 1, H, W)] with ties, bbox_preds [(B, 4, H, W)] (values ``dtype`` stores exactly), per-image
    anchors (B, N, 4), a mask (B, N) and image shapes.  ``mask_kind``: 'ones'; 'random' (about half in; image 0 has no
    location in on level 1; the last image has none at all when B > 1)."""
    g = np.random.default_rng(seed)
    N = nloc(sizes)
    vals = np.array([-1.5, -0.25, 0.0, -0.0, 0.75, 2.0], f32)
    cls = [stored(np.where(g.uniform(0, 1, (Bn, 1, h, w)) < 0.3, vals[g.integers(0, 6, (Bn, 1, h, w))],
                           g.normal(0, 2.0, (Bn, 1, h, w))), dtype) for h, w in sizes]
    reg = [stored(g.normal(0, 0.5, (Bn, 4, h, w)), dtype) for h, w in sizes]
    sq = squares_of(sizes)
    fac = np.exp(g.uniform(-0.7, 0.7, (Bn, N, 2)))
    ctr, side = (sq[:, :2] + sq[:, 2:]) / 2, (sq[:, 2] - sq[:, 0] + 1)[None, :, None]
    wh = side * fac
    anchors = np.concatenate([ctr[None] - (wh - 1) / 2, ctr[None] + (wh - 1) / 2], 2).astype(f32)
    if mask_kind == "ones":
        mask = np.ones((Bn, N), np.uint8)
    else:
        mask = (g.uniform(0, 1, (Bn, N)) < 0.5).astype(np.uint8)
        n0, n1 = sizes[0][0] * sizes[0][1], sizes[0][0] * sizes[0][1] + sizes[1][0] * sizes[1][1]
        mask[0, n0:n1] = 0
        if Bn > 1:
            mask[Bn - 1] = 0
    Hh, Ww = extent(sizes)
    img_shapes = np.array([[Hh - 3 * b, Ww - 5 * b] for b in range(Bn)], np.int32)
    return dict(cls=cls, reg=reg, anchors=anchors, mask=mask, img_shapes=img_shapes)
