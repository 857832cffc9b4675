"""Inputs shared by tests/test_dense_detect_oracle.py (CPU) and tests/test_gpu_dense_detect.py: the 64 x 96 pyramid,
head outputs drawn from small grids (so that ties are certain) and ground truths for the targets.  Everything is NumPy /
CPU torch; the GPU tests move it over."""
import numpy as np
import torch

from oracle import box_ref as B

f32 = np.float32
IMG = (64, 96)
LEVELS = [((8, 12), 8), ((4, 6), 16), ((2, 3), 32)]         # 864 + 216 + 54 = 1134 anchors at A = 9
BIG = [((32, 32), 8)]                                      # 9216 anchors: more than one 8192-key selection step
SCALES9, RATIOS = [2.0, 2.5, 3.25], [0.5, 1.0, 2.0]
GRID32 = (np.arange(32) / 4.0 - 6.0).astype(f32)           # for levels of at most 216 anchors
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)


def pyramid(levels, A=9):
    """Per-level (H*W*A, 4) float32 anchors in (y, x, a) order."""
    scales = SCALES9 if A == 9 else [2.0 + i for i in range(A)]
    ratios = RATIOS if A == 9 else [1.0]
    return [B.anchor_grid(B.base_anchors(s, scales, ratios), fs, s)[0] for fs, s in levels]


def fine_draw(g, shape):
    """Logits from the 257-value grid k/16, |x| <= 8 (exact in bf16 and fp16), normally distributed: the tail is thin, so
    the class maximum of many draws does not pile up on the top value, and a cut among the best 100 still meets ties."""
    return (np.clip(np.round(g.normal(0, 1.5, shape) * 16), -128, 128) / 16).astype(f32)


def img_shapes(Bn, levels=LEVELS):
    """Per-image (h, w), none larger than the first level's extent (IMG for LEVELS)."""
    (H, W), s = levels[0]
    return np.asarray([(H * s - 3 * b, W * s - 5 * (b % 2)) for b in range(Bn)], np.int32)


def layouts(kind, L):
    """(cls channels_last, reg channels_last) per level."""
    return {"nchw": [(False, False)] * L, "nhwc": [(True, True)] * L,
            "mixed": [(l % 2 == 0, l % 2 == 1) for l in range(L)]}[kind]


def head_case(levels, Bn, A, C, dtype, layout, seed):
    """-> (cls_scores, bbox_preds): CPU torch tensors of ``dtype`` in the asked memory layout.  Every third anchor has
    dw = dh = 0 (the decode is then free of exp rounding: bit-exact)."""
    g = np.random.default_rng(seed)
    cls, reg = [], []
    for l, (((H, W), _), (cl, rl)) in enumerate(zip(levels, layouts(layout, len(levels)))):
        shape = (Bn, A * C, H, W)
        c = g.choice(GRID32, shape).astype(f32) if H * W * A <= 216 else fine_draw(g, shape)
        d = g.normal(0, 0.5, (Bn, A, 4, H, W)).astype(f32)
        flat = d.transpose(0, 3, 4, 1, 2).reshape(Bn, H * W * A, 4)      # a copy in anchor order
        flat[:, ::3, 2:] = 0
        d = flat.reshape(Bn, H, W, A, 4).transpose(0, 3, 4, 1, 2).reshape(Bn, 4 * A, H, W)
        c, d = torch.from_numpy(np.ascontiguousarray(c)).to(dtype), torch.from_numpy(np.ascontiguousarray(d)).to(dtype)
        cls.append(c.contiguous(memory_format=torch.channels_last) if cl else c.contiguous())
        reg.append(d.contiguous(memory_format=torch.channels_last) if rl else d.contiguous())
    return cls, reg


def stored(ts):
    """The stored values of a list of tensors as float32 arrays."""
    return [t.float().numpy() for t in ts]


def overflow_case(extra, seed=5):
    """Two levels (9216 + 864 anchors, A = 9), C = 2, two images, nms_pre = 4096.  Image 0: class 0 has 5000 positive
    logits on the big level (4096 survive the cut) and ``extra`` on the small one, everything else is -6 (score 0.0025):
    4096 + extra candidates above 0.05.  Image 1 is an ordinary random image."""
    levels = BIG + LEVELS[:1]
    g = np.random.default_rng(seed)
    cls, reg = head_case(levels, 2, 9, 2, torch.float32, "nhwc", seed)
    for l, n_pos in ((0, 5000), (1, extra)):
        c = cls[l]
        H, W = c.shape[2:]
        x = np.full((H * W * 9, 2), -6.0, f32)
        x[g.permutation(H * W * 9)[:n_pos], 0] = g.choice(np.arange(1, 33) / 8.0, n_pos).astype(f32)
        c[0] = torch.from_numpy(x.reshape(H, W, 9 * 2).transpose(2, 0, 1).copy())
        c[1] -= 4                                # about a quarter of image 1's scores stay above 0.05
    return levels, cls, reg


# ---- targets ---------------------------------------------------------------------------------------------------------
def target_case(seed, gt_counts=(4, 2), G=4, C=5):
    """Random 10-60 pixel ground truths inside the image, labels in 1..C, valid flags that drop a few anchors."""
    g = np.random.default_rng(seed)
    Bn = len(gt_counts)
    anchors = np.concatenate(pyramid(LEVELS))
    gt = np.zeros((Bn, G, 4), f32)
    for b, n in enumerate(gt_counts):
        wh = g.integers(10, 61, (n, 2))
        xy = np.stack([g.integers(0, IMG[1] - wh[:, 0]), g.integers(0, IMG[0] - wh[:, 1])], 1)
        gt[b, :n] = np.concatenate([xy, xy + wh - 1], 1)
    labels = g.integers(1, C + 1, (Bn, G)).astype(np.int64)
    valid = (g.random((Bn, anchors.shape[0])) > 0.05).astype(np.uint8)
    return dict(anchors=anchors, gt_bboxes=gt, gt_labels=labels, gt_counts=np.asarray(gt_counts, np.int32),
                img_shapes=img_shapes(Bn), valid=valid)
