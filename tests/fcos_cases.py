"""Inputs shared by tests/test_fcos_oracle.py (CPU) and tests/test_gpu_fcos.py: small pyramids, ground truths on integer
and half-integer coordinates (edge hits and area ties really occur), head outputs whose stored values are exact in
every dtype where a test needs an exact coincidence."""
import numpy as np
import torch

f32 = np.float32
INF = float("inf")
# (featmap size, stride) of the 64 x 96 image; one level of 9216 points (more than one compaction chunk of 8192, 36
# workgroups of the target kernel); one 1 x 1 level
LEVELS = [((8, 12), 8), ((4, 6), 16), ((2, 3), 32)]
RANGES = ((-1, 24), (24, 48), (48, INF))
BIG = [((96, 96), 8), ((1, 1), 64)]
BIG_RANGES = ((-1, 64), (64, INF))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def sizes(levels):
    return [fs for fs, _ in levels]


def strides(levels):
    return [s for _, s in levels]


def num_points(levels):
    return sum(h * w for (h, w), _ in levels)


def gt_case(B, G, counts, seed, extent=(64, 96)):
    """(gt_bboxes (B, G, 4) f32, gt_labels (B, G) i64 in 1..5, gt_counts (B,) i32).  Corners lie on multiples of 0.5; box 1
    is box 0 moved by half a stride (equal area, overlapping: ties), box 2 lies inside box 0 (nested), box 3 has its left
    edge on a point column of level 0 and its top edge one pixel above a point row (a distance of exactly 0 and of
    exactly 1); rows past gt_counts hold NaN."""
    g = np.random.default_rng(seed)
    H, W = extent
    gt = np.full((B, max(G, 0), 4), np.nan, f32)
    for b in range(B):
        for j in range(min(int(counts[b]), G)):
            w, h = g.choice([8, 16, 24, 40, 56]), g.choice([8, 16, 24, 40, 56])
            x1 = g.integers(0, max(1, (W - w) * 2)) * 0.5
            y1 = g.integers(0, max(1, (H - h) * 2)) * 0.5
            gt[b, j] = (x1, y1, x1 + w, y1 + h)
        n = min(int(counts[b]), G)
        if n >= 4:
            gt[b, 0] = (10.5, 6.5, 50.5, 46.5)
            gt[b, 1] = gt[b, 0] + f32([4, 0, 4, 0])
            gt[b, 2] = (16.5, 12.5, 36.5, 30.5)
            gt[b, 3] = (12.0, 11.0, 28.0, 27.0)
        elif n >= 1:
            gt[b, 0] = (12.0, 11.0, 28.0, 27.0)
    labels = g.integers(1, 6, (B, max(G, 0))).astype(np.int64)
    return gt, labels, np.asarray(counts, np.int32)


def stored(a, dtype):
    """``a`` rounded to the storage dtype, as float32."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dtype).float().numpy()


def layout(t, nhwc):
    return t.contiguous(memory_format=torch.channels_last) if nhwc else t.contiguous()


def flags(name, l):
    """(cls, reg) channels_last flags of level ``l`` for a layout name."""
    return {"nchw": (False, False), "nhwc": (True, True), "mixed": (l % 2 == 0, l % 2 == 1)}[name]


def to_tensors(arrs, dtype, name):
    """[(cls, reg, ctr) float32 arrays per level] -> three lists of CPU tensors of ``dtype`` in layout ``name``."""
    out = ([], [], [])
    for l, (c, r, z) in enumerate(arrs):
        fc, fr = flags(name, l)
        out[0].append(layout(torch.from_numpy(c).to(dtype), fc))
        out[1].append(layout(torch.from_numpy(r).to(dtype), fr))
        out[2].append(layout(torch.from_numpy(z).to(dtype), fr))
    return out


def loss_case(levels, B, C, labels, bbox_targets, seed, poison=True):
    """Head outputs (float32 arrays per level) for given targets: regression outputs near log(target) so that the IoUs
    spread over (0, 1); on positives whose target distance is exactly 1 the output is 0 in that coordinate (d == d*: the
    min / max tie); every fourth positive predicts e^-8 in all directions (IoU far below 1e-3); NaN / Inf on every
    element that is never read."""
    g = np.random.default_rng(seed)
    out, n0 = [], 0
    for (h, w), _ in levels:
        n1 = n0 + h * w
        lab, bt = labels[:, n0:n1], bbox_targets[:, n0:n1]
        c = np.clip(g.normal(-1.0, 1.5, (B, C, h, w)), -4, 4).astype(f32)
        with np.errstate(all="ignore"):
            r = np.log(np.maximum(bt, 1e-3)) + g.normal(0, 0.4, bt.shape)
        r = np.where(bt == 1, 0.0, r)
        pos = lab > 0
        tiny = pos & (np.cumsum(pos.reshape(-1)).reshape(pos.shape) % 4 == 0)
        r[tiny] = -8.0
        z = g.normal(0, 1.5, (B, h * w)).astype(f32)
        if poison:
            bad = g.choice(np.array([np.nan, np.inf, -np.inf]), r.shape)
            r = np.where(pos[..., None], r, bad)
            z = np.where(pos, z, bad[..., 0]).astype(f32)
        else:
            r = np.where(pos[..., None], r, g.normal(0, 1, r.shape))
        out.append((c, np.ascontiguousarray(r.transpose(0, 2, 1)).reshape(B, 4, h, w).astype(f32),
                    z.reshape(B, 1, h, w)))
        n0 = n1
    return out


# detections: logits and centre-ness from small grids of values that every dtype stores exactly, so that equal (class
# maximum, centre-ness) pairs — exact key ties — are certain; distances from a grid as well
CLS_GRID = np.arange(-20, 13, dtype=f32) * f32(0.1875)          # 33 values in [-3.75, 2.25]
CTR_GRID = np.arange(-5, 6, dtype=f32) * f32(0.4375)            # 11 values in [-2.1875, 2.1875]


def det_case(levels, B, C, seed, n_cls=6, n_ctr=4):
    g = np.random.default_rng(seed)
    cg = g.choice(CLS_GRID, n_cls, replace=False)
    zg = g.choice(CTR_GRID, n_ctr, replace=False)
    out = []
    for (h, w), s in levels:
        c = g.choice(cg, (B, C, h, w)).astype(f32)
        low = g.random((B, 1, h, w)) < 0.6                        # most points are background in every class
        c = np.where(low, np.minimum(c, f32(-3.75)), c).astype(f32)
        r = (np.log(s * 1.5) + g.integers(-4, 5, (B, 4, h, w)) * 0.25).astype(f32)
        z = g.choice(zg, (B, 1, h, w)).astype(f32)
        out.append((c, r, z))
    return out


def img_shapes(B, extent=(64, 96)):
    H, W = extent
    return np.array([(H - 3 * b, W - 5 * b) for b in range(B)], np.int32)
