"""Shared case generator of the Cascade R-CNN tests (tests/test_cascade_oracle.py, tests/test_gpu_cascade.py).

Everything is generated in NumPy / CPU torch; 16-bit operands are rounded once here, and the reference reads the rounded
values widened to fp32 (exact), so the GPU and the reference see the same numbers.
"""
import numpy as np
import torch

f32 = np.float32
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [(600, 900), (480, 1000), (333, 500)]          # (h, w) of up to three images
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)
G = 5                                                   # ground truths per image (padded)


def widen(t):
    """A torch tensor of any of the three dtypes as the float32 array of its stored values."""
    return t.float().numpy()


def refine_case(R, B, C, agnostic, dt, seed, pad=0.15, gt_frac=0.2, only_images=None):
    """-> dict(rois (R, 5) f32, reg (R, 4C or 4) torch dt, labels (R,) i64, cls (R, C) torch dt, gt (B, G, 4) f32,
    gt_inds (R,) i32, shapes).

    Rows: the images interleaved row by row at random, ``pad`` of them padding (index -1, plus one row of index B and one
    of 0.5, which truncates to image 0); boxes reach past the smallest image, so the clip at w-1 / h-1 acts, and some
    deltas push a box left of 0; every 7th row's log-size deltas are beyond wh_ratio_clip; every 3rd row's are 0 (the
    exp-free rows: exp(0) is exact everywhere).  ``gt_frac`` of the rows are ground truths (their four coordinates are
    those of gt[b, gt_inds[r]]), as many again are positives with a ground-truth index but their own box.  The logits
    come from {0, 0.5, 1}, so nearly every row's maximum is tied."""
    g = np.random.default_rng(seed)
    shapes = SHAPES[:B]
    img = g.integers(0, B, (R,)) if only_images is None else g.choice(np.asarray(only_images), (R,))
    img = img.astype(np.float64)
    img[g.random(R) < pad] = -1
    if R > 3:
        img[1], img[2] = B, 0.5
    xy = g.uniform(0, 700, (R, 2))
    wh = g.uniform(16, 320, (R, 2))
    rois = np.concatenate([img[:, None], xy, xy + wh], 1).astype(f32)
    K = 1 if agnostic else C
    d = g.normal(0, 0.8, (R, K, 4))
    d[::5, :, 0] = -40.0                                 # far left of the image: clipped at 0
    d[::7, :, 2:] = g.choice([-30.0, 30.0], (len(d[::7]), K, 2))
    d[::3, :, 2:] = 0
    reg = torch.from_numpy(d.reshape(R, 4 * K)).to(DTYPES[dt]).contiguous()
    labels = g.integers(0, C, (R,)).astype(np.int64)
    cls = torch.from_numpy(g.choice([0.0, 0.5, 1.0], (R, C))).to(DTYPES[dt]).contiguous()
    gxy = g.uniform(0, 300, (B, G, 2))
    gt = np.concatenate([gxy, gxy + g.uniform(20, 150, (B, G, 2))], -1).astype(f32)
    gt_inds = np.full((R,), -1, np.int32)
    u = g.random(R)
    which = g.integers(0, G, (R,)).astype(np.int32)
    valid = (img >= 0) & (img < B)
    is_gt = valid & (u < gt_frac)
    is_pos = valid & (u >= gt_frac) & (u < 2 * gt_frac)
    b_of = np.where(valid, np.trunc(img), 0).astype(np.int64)
    rois[is_gt, 1:] = gt[b_of[is_gt], which[is_gt]]
    gt_inds[is_gt | is_pos] = which[is_gt | is_pos]
    return dict(rois=rois, reg=reg, labels=labels, cls=cls, gt=gt, gt_inds=gt_inds, shapes=shapes, is_gt=is_gt,
                valid=valid, img=np.where(valid, b_of, -1))


def detect_case(R, B, C, S, agnostic, dt, seed):
    """-> (rois (R, 5) f32, [S logits (R, C) torch dt], reg (R, 4C or 4) torch dt, shapes): one dominant class per row,
    spread over the stages so that no single stage decides, clustered boxes so that NMS has work."""
    g = np.random.default_rng(seed)
    shapes = SHAPES[:B]
    ncl = max(2, R // 8)
    centres = g.uniform(0, 420, (ncl, 2))
    xy = centres[g.integers(0, ncl, R)] + g.uniform(-6, 6, (R, 2))
    wh = g.uniform(40, 80, (R, 2))
    img = g.integers(0, B, (R,)).astype(np.float64)
    img[g.random(R) < 0.15] = -1
    if R > 3:
        img[1], img[2] = B, 0.5
    rois = np.concatenate([img[:, None], xy, xy + wh], 1).astype(f32)
    top = g.integers(0, C, R)
    logits = []
    for s in range(S):
        x = g.normal(0, 1.0, (R, C))
        x[np.arange(R), top] += 6.0 + 2.0 * s
        logits.append(torch.from_numpy(x).to(DTYPES[dt]).contiguous())
    K = 1 if agnostic else C
    d = g.normal(0, 0.5, (R, K, 4))
    d[::3, :, 2:] = 0
    reg = torch.from_numpy(d.reshape(R, 4 * K)).to(DTYPES[dt]).contiguous()
    return rois, logits, reg, shapes
