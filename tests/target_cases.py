"""Full-size cases of the training-target tests (C4 pyramid, 800 x 1344, 268,569 anchors), built on the CPU from the C
oracle's anchors so that tests/test_target_oracle.py can assert, without a GPU, that the oracle's own output takes
every branch of the spec on them; tests/test_gpu_targets.py then compares the kernels on the same cases."""
import numpy as np

from oracle import box_ref as B

LEVELS = [((200, 336), 4), ((100, 168), 8), ((50, 84), 16), ((25, 42), 32), ((13, 21), 64)]
NUM_ANCHORS = 268569
MAX_GT = 256


def pyramid(img_shape=None):
    """(anchors (268569, 4), valid flags for an un-padded image of ``img_shape`` (None: all valid))."""
    anchors, valid = [], []
    for (fh, fw), st in LEVELS:
        vs = None if img_shape is None else (min(fh, -(-img_shape[0] // st)), min(fw, -(-img_shape[1] // st)))
        a, v = B.anchor_grid(B.base_anchors(st, [8], [0.5, 1.0, 2.0]), (fh, fw), st, vs)
        anchors.append(a)
        valid.append(v)
    return np.concatenate(anchors), np.concatenate(valid)


def ground_truths(anchors, img_shape, count, seed):
    """``count`` boxes inside the image: a duplicate pair in front, exact copies of anchors (IoU 1.0), anchors moved by
    half their level's stride (integer coordinates, ties across neighbouring anchors), and thin random integer boxes
    whose best anchor stays below 0.7."""
    g = np.random.default_rng(seed)
    h, w = img_shape
    inside = np.nonzero((anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < w) & (anchors[:, 3] < h))[0]
    out = []
    for k in range(count):
        kind = k % 4
        a = anchors[inside[g.integers(0, inside.shape[0])]]
        if kind in (0, 1) and k >= 2:
            out.append(a.copy())
        elif kind == 2:
            half = np.float32(max(2.0, np.round((a[2] - a[0] + 1) / 16)))      # half a stride of the anchor's level
            out.append(a + np.array([half, 0, half, 0], np.float32))
        else:
            bw, bh = g.integers(60, 300), g.integers(9, 24)
            x1, y1 = g.integers(0, w - bw), g.integers(0, h - bh)
            out.append(np.array([x1, y1, x1 + bw - 1, y1 + bh - 1], np.float32))
    gt = np.asarray(out, np.float32).reshape(-1, 4)
    if count >= 2:
        gt[1] = gt[0] = anchors[inside[g.integers(0, inside.shape[0])]]        # the duplicate pair
    gt[:, 0::2] = np.clip(gt[:, 0::2], 0, w - 1)
    gt[:, 1::2] = np.clip(gt[:, 1::2], 0, h - 1)
    return gt


def anchor_case(gt_counts, shapes, seed, per_image_boxes=False):
    """dict of numpy inputs of anchor_target for len(gt_counts) images."""
    Bn = len(gt_counts)
    anchors, _ = pyramid()
    G = max(max(gt_counts), 1)
    gt = np.zeros((Bn, G, 4), np.float32)
    valid = np.zeros((Bn, anchors.shape[0]), np.uint8)
    for b in range(Bn):
        valid[b] = pyramid(shapes[b])[1]
        gt[b, :gt_counts[b]] = ground_truths(anchors, shapes[b], gt_counts[b], seed + b)
        gt[b, gt_counts[b]:] = 0
    boxes = anchors
    if per_image_boxes:              # every image its own copy, moved by an integer so that the sets differ
        boxes = np.stack([anchors + np.float32(b) for b in range(Bn)])
    return dict(anchors=boxes, valid_flags=valid, gt_bboxes=gt, gt_counts=np.asarray(gt_counts, np.int32),
                img_shapes=np.asarray(shapes, np.int32))


def caller_keys(Bn, n, seed):
    """Few distinct values: plenty of key ties, which the index must break."""
    return np.random.default_rng(seed).integers(0, 50, (Bn, n)).astype(np.int32)


CASES = {
    "b3": dict(gt_counts=(0, 1, 37), shapes=[(800, 1344), (600, 1000), (800, 1100)], seed=11),
    "b2": dict(gt_counts=(100, MAX_GT), shapes=[(800, 1344), (704, 1216)], seed=23),
}


def assert_coverage(info, num_pos_expected):
    """On the ORACLE's bookkeeping: the case takes every branch of the spec."""
    assert info["only_step6"] >= 1, "no box is positive only through step 6"
    assert info["step6_ties"] >= 1, "no step-6 tie between two ground truths"
    assert any(n > num_pos_expected for n in info["n_pos"]), info["n_pos"]
    assert any(n < num_pos_expected for n in info["n_pos"]), info["n_pos"]
    assert info["by_border"] >= 1 and info["by_valid"] >= 1, info
