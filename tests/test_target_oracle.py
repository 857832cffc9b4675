"""CPU: the training-target oracle (tests/target_ref.py) against an independently written torch
restatement of MaxIoUAssigner / RandomSampler, against hand-worked answers, and on the full-size cases the GPU tests
use (whose branch coverage is asserted here on the oracle alone)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import target_cases as C
import target_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_package_exports_the_four_entry_points_and_mirrors_the_header(tmp_path):
    import torch_detection_amd as T
    from torch_detection_amd import _lib
    for n in ("assign_max_iou", "sample_assigned", "anchor_target", "sample_rois"):
        assert callable(getattr(T, n))
    assert (_lib.TARGET_MAX_GT, _lib.TARGET_MAX_BOXES, _lib.TARGET_MAX_NUM) == (R.MAX_GT, R.MAX_BOXES, R.MAX_NUM)
    hdr = open(os.path.join(ROOT, "include", "tdn.h")).read()
    assert "#define TDN_TARGET_MAX_GT %d\n" % R.MAX_GT in hdr and "#define TDN_TARGET_MAX_NUM %d\n" % R.MAX_NUM in hdr
    # struct layout as gcc sees it == the ctypes mirror
    fields = [f for f, _ in _lib.TargetConfig._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {',
             'printf("%zu\\n", sizeof(tdn_target_config));']
    lines += ['printf("%%zu\\n", offsetof(tdn_target_config, %s));' % f for f in fields] + ['return 0; }']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "l")]).decode().split()]
    assert out[0] == ctypes.sizeof(_lib.TargetConfig)
    assert out[1:] == [getattr(_lib.TargetConfig, f).offset for f in fields]
    # host-side refusals of the library itself (no device is touched before them)
    lib = _lib.load()
    assert lib.tdn_assign_max_iou_workspace_bytes(2, 257) == -1 and lib.tdn_anchor_target_workspace_bytes(65, 10, 4) == -1
    assert lib.tdn_anchor_target_workspace_bytes(2, 268569, 100) == 2 * 1024 + 2 * 537344
    assert lib.tdn_sample_rois_workspace_bytes(2, 2000, 100, 1) > lib.tdn_sample_rois_workspace_bytes(2, 2000, 100, 0) > 0


def test_workspace_sizes_are_the_design_table():
    """DESIGN.md §5d worked by hand: every region rounded up to 256 bytes, in the table's order."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    # assignment, B = 3, G = 70: colmax and first are 210 words = 840 -> 1024 bytes each; G = 0 counts as one column
    assert lib.tdn_assign_max_iou_workspace_bytes(3, 70) == 2 * 1024
    assert lib.tdn_assign_max_iou_workspace_bytes(2, 0) == 2 * 256
    assert lib.tdn_assign_max_iou_workspace_bytes(0, 4) == -1 and lib.tdn_assign_max_iou_workspace_bytes(2, -1) == -1
    # anchor_target, B = 3, N = 1000, G = 70: the assignment words, then two masks of 3000 -> 3072 bytes
    assert lib.tdn_anchor_target_workspace_bytes(3, 1000, 70) == 2 * 1024 + 2 * 3072
    assert lib.tdn_anchor_target_workspace_bytes(2, 0, 0) == 2 * 256 + 2 * 256          # N = 0 counts as one box
    assert lib.tdn_anchor_target_workspace_bytes(2, (1 << 20) + 1, 4) == -1
    assert lib.tdn_anchor_target_workspace_bytes(2, -1, 4) == -1
    # sample_rois, B = 2, P = 2000, G = 100: assignment words 800 -> 1024 each; with the ground truths added Nc = 2100:
    # assigned 4200 * 4 = 16800 -> 16896, masks 4200 -> 4352 each; without, Nc = 2000: 16000 -> 16128, 4000 -> 4096
    assert lib.tdn_sample_rois_workspace_bytes(2, 2000, 100, 1) == 2 * 1024 + 16896 + 2 * 4352
    assert lib.tdn_sample_rois_workspace_bytes(2, 2000, 100, 0) == 2 * 1024 + 16128 + 2 * 4096
    assert lib.tdn_sample_rois_workspace_bytes(2, 0, 0, 1) == 2 * 256 + 256 + 2 * 256   # Nc = 0 counts as one box
    assert lib.tdn_sample_rois_workspace_bytes(2, (1 << 20) - 255, 4, 0) == -1
    assert lib.tdn_sample_rois_workspace_bytes(65, 10, 4, 0) == -1


# ---- an independent restatement in torch (mmdetection's formulation: (G, N) overlaps, max over both axes) ----------
def torch_iou(a, b):
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = ((rb - lt) + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    aa = ((a[:, 2] - a[:, 0]) + 1) * ((a[:, 3] - a[:, 1]) + 1)
    ab = ((b[:, 2] - b[:, 0]) + 1) * ((b[:, 3] - b[:, 1]) + 1)
    return inter / ((aa[:, None] + ab[None, :]) - inter)


def torch_assign(boxes, gts, pos, neg, min_pos, assign_all):
    n = boxes.shape[0]
    assigned = torch.full((n,), -1, dtype=torch.long)
    if gts.shape[0] == 0:
        return assigned.zero_()
    if n == 0:
        return assigned
    ov = torch_iou(gts, boxes)                                     # (G, N)
    max_ov, argmax = ov.max(dim=0)
    gt_max, gt_argmax = ov.max(dim=1)
    pos, neg, min_pos = (torch.tensor(v, dtype=torch.float32) for v in (pos, neg, min_pos))
    assigned[(max_ov >= 0) & (max_ov < neg)] = 0
    sel = max_ov >= pos
    assigned[sel] = argmax[sel] + 1
    for i in range(gts.shape[0]):
        if gt_max[i] >= min_pos:
            if assign_all:
                assigned[ov[i] == gt_max[i]] = i + 1
            else:
                assigned[gt_argmax[i]] = i + 1
    return assigned


def int_boxes(g, n, canvas=200, lo=4, hi=80):
    wh = g.integers(lo, hi, (n, 2))
    xy = g.integers(0, canvas - hi, (n, 2))
    return np.concatenate([xy, xy + wh - 1], 1).astype(np.float32)


@pytest.mark.parametrize("seed", range(6))
def test_assigner_against_torch_restatement(seed):
    g = np.random.default_rng(seed)
    n, G, Bn = int(g.integers(50, 400)), int(g.integers(1, 12)), 3
    boxes = int_boxes(g, n)
    gt = np.stack([int_boxes(g, G) for _ in range(Bn)])
    gt[:, -1] = boxes[:Bn]                                           # an exact copy per image
    counts = np.array([G, max(G - 1, 0), 0], np.int32)
    valid = (g.random(n) > 0.2).astype(np.uint8)
    pos, neg, mp = [(0.5, 0.4, 0.2), (0.7, 0.3, 0.3), (0.5, 0.5, 0.0)][seed % 3]
    for all_ in (True, False):
        a, mo = R.assign_max_iou(boxes, gt, counts, pos, neg, mp, all_, valid)
        for b in range(Bn):
            idx = np.nonzero(valid)[0]
            ta = torch_assign(torch.from_numpy(boxes[idx]), torch.from_numpy(gt[b, :counts[b]]), pos, neg, mp, all_)
            assert np.array_equal(a[b, idx], ta.numpy()), (seed, b, all_)
            assert np.all(a[b, valid == 0] == -1) and np.all(mo[b, valid == 0] == 0)
            if counts[b]:
                tm = torch_iou(torch.from_numpy(boxes[idx]), torch.from_numpy(gt[b, :counts[b]])).max(dim=1)[0]
                assert np.array_equal(mo[b, idx].view(np.uint32), tm.numpy().view(np.uint32))


def test_known_answers():
    box, half = np.array([[0, 0, 9, 9]], np.float32), np.array([[[0, 0, 9, 19]]], np.float32)
    one = np.array([1], np.int32)
    a, mo = R.assign_max_iou(box, half, one, 0.5, 0.3, 0.9)
    assert mo[0, 0] == np.float32(0.5) and a[0, 0] == 1             # exactly on pos_iou_thr: positive
    a, _ = R.assign_max_iou(box, half, one, 0.7, 0.5, 0.9)
    assert a[0, 0] == -1                                             # exactly on neg_iou_thr: not negative
    a, _ = R.assign_max_iou(box, half, one, 0.7, 0.5000001, 0.9)
    assert a[0, 0] == 0
    # duplicated ground truth: argmax -> the lower index, low-quality assignment -> the higher
    boxes = np.array([[0, 0, 9, 9], [0, 0, 9, 11], [100, 100, 120, 120]], np.float32)
    gt = np.array([[[0, 0, 9, 9], [0, 0, 9, 9]]], np.float32)
    a, _ = R.assign_max_iou(boxes, gt, np.array([2], np.int32), 0.7, 0.3, 2.0)
    assert a[0].tolist() == [1, 1, 0]
    a, _ = R.assign_max_iou(boxes, gt, np.array([2], np.int32), 0.7, 0.3, 0.3)
    assert a[0].tolist() == [2, 1, 0]
    # a ground truth whose best box is below pos_iou_thr: positive through step 6 only
    gt = np.array([[[0, 0, 9, 17]]], np.float32)                     # iou 100/180 with box 0, 120/180 with box 1
    a, mo = R.assign_max_iou(boxes, gt, one, 0.7, 0.3, 0.3)
    assert a[0].tolist() == [-1, 1, 0] and mo[0, 1] < np.float32(0.7)
    a, _ = R.assign_max_iou(boxes, gt, one, 0.7, 0.3, 0.7)
    assert a[0].tolist() == [-1, -1, 0]
    # G = 0, N = 0, all boxes invalid
    a, mo = R.assign_max_iou(boxes, np.zeros((1, 3, 4), np.float32), np.array([0], np.int32), 0.7, 0.3)
    assert a[0].tolist() == [0, 0, 0] and np.all(mo == 0)
    a, mo = R.assign_max_iou(np.zeros((0, 4), np.float32), gt, one, 0.7, 0.3)
    assert a.shape == (1, 0) and mo.shape == (1, 0)
    a, mo = R.assign_max_iou(boxes, gt, one, 0.7, 0.3, 0.0, True, np.zeros(3, np.uint8))
    assert a[0].tolist() == [-1, -1, -1] and np.all(mo == 0)
    # padded ground-truth rows are never read
    pad = np.concatenate([gt, np.full((1, 2, 4), np.nan, np.float32)], 1)
    assert np.array_equal(R.assign_max_iou(boxes, pad, one, 0.7, 0.3, 0.3)[0], R.assign_max_iou(boxes, gt, one, 0.7, 0.3, 0.3)[0])


@pytest.mark.parametrize("n_pos,n_neg,num,frac,ub,want", [
    (200, 1000, 256, 0.5, -1, (128, 128)),          # #pos above n_pos_exp
    (128, 1000, 256, 0.5, -1, (128, 128)),          # equal
    (10, 1000, 256, 0.5, -1, (10, 246)),            # below: the negatives fill up
    (10, 1000, 256, 0.5, 3, (10, 30)),              # neg_pos_ub binding
    (0, 1000, 256, 0.5, 3, (0, 3)),                 # max(1, pos)
    (10, 1000, 256, 0.5, 0.25, (10, 2)),            # int() truncates
    (10, 40, 256, 0.5, -1, (10, 40)),               # fewer negatives than asked
    (300, 1000, 512, 0.25, -1, (128, 384)),
    (5, 5, 0, 0.5, -1, (0, 0)),
])
def test_sampler_counts(n_pos, n_neg, num, frac, ub, want):
    assert R.sample_counts(n_pos, n_neg, num, frac, ub) == want
    g = np.random.default_rng(n_pos + num)
    a = np.concatenate([g.integers(1, 5, n_pos), np.zeros(n_neg, int), -np.ones(17, int)]).astype(np.int32)
    g.shuffle(a)
    keys = g.integers(0, 20, (1, a.shape[0])).astype(np.int32)
    for k in (None, keys):
        pm, nm, npos, nneg = R.sample_assigned(a[None], num, frac, ub, k, seed=3)
        assert (int(npos[0]), int(nneg[0])) == want == (int(pm.sum()), int(nm.sum()))
        assert np.all(a[pm[0] == 1] > 0) and np.all(a[nm[0] == 1] == 0)
        key = keys[0].astype(np.int64) if k is not None else R.target_key(3, 0, np.arange(a.shape[0]))
        for mask, cls in ((pm[0], a > 0), (nm[0], a == 0)):          # nothing left out beats anything taken
            if mask.any() and (cls & (mask == 0)).any():
                t = max(zip(key[mask == 1], np.nonzero(mask == 1)[0]))
                r = min(zip(key[cls & (mask == 0)], np.nonzero(cls & (mask == 0))[0]))
                assert t < r


def test_key_hash():
    i = np.arange(1 << 16)
    k = R.target_key(5, 2, i)
    assert np.array_equal(k, R.target_key(5, 2, i)) and k.min() >= 0 and k.max() < 2 ** 31
    assert int(R.target_key(5, 2, 12345)) == int(k[12345])
    assert not np.array_equal(k, R.target_key(6, 2, i)) and not np.array_equal(k, R.target_key(5, 3, i))
    assert np.unique(k).shape[0] >= (1 << 16) - 1                     # a bijection before the top-31-bit cut
    assert R.target_key(5 + 2 ** 32, 2, i)[7] == k[7]                 # the seed counts modulo 2^32
    top = np.bincount((k >> 27).astype(np.int64), minlength=16)       # the 4 top bits: 4096 expected per bin
    assert top.min() > 3700 and top.max() < 4500, top
    # the value the kernel's arithmetic gives, worked by hand in Python integers
    h = (0 ^ (1 * 0x9E3779B9) ^ (7 * 0x85EBCA6B & 0xFFFFFFFF)) & 0xFFFFFFFF
    h ^= h >> 16
    h = h * 0x7FEB352D & 0xFFFFFFFF
    h ^= h >> 15
    h = h * 0x846CA68B & 0xFFFFFFFF
    h ^= h >> 16
    assert int(R.target_key(0, 1, 7)) == h >> 1


def test_full_size_cases_take_every_branch():
    """What tests/test_gpu_targets.py asserts before it compares, here on the CPU: the seeds of target_cases.py are
    good."""
    info = {}
    case = C.anchor_case(**C.CASES["b3"])
    assert case["anchors"].shape == (C.NUM_ANCHORS, 4)
    out = R.anchor_target(info=info, **case)
    C.assert_coverage(info, 128)
    assert out[4].tolist()[0] == 0 and out[5].tolist()[0] == 256      # G = 0: negatives only
    lab, lw, bt, bw = out[:4]
    assert np.all(bt[lab == 0] == 0) and np.all(bw[lab == 1] == 1) and lw.sum() == out[4].sum() + out[5].sum()
    info = {}
    R.anchor_target(info=info, num=2000, **C.anchor_case(**C.CASES["b2"]))
    C.assert_coverage(info, 1000)
    info = {}
    R.anchor_target(info=info, gt_max_assign_all=False, **C.anchor_case(per_image_boxes=True, **C.CASES["b2"]))
    assert info["only_step6"] >= 1 and info["step6_ties"] >= 1, info
    info = {}
    R.anchor_target(info=info, gt_max_assign_all=False, **C.anchor_case(per_image_boxes=True, **C.CASES["b3"]))
    assert info["only_step6"] >= 1 and info["step6_ties"] >= 1, info


def test_sample_rois_layout():
    g = np.random.default_rng(0)
    props = np.zeros((2, 30, 5), np.float32)
    props[:, :, :4] = np.stack([int_boxes(g, 30), int_boxes(g, 30)])
    counts = np.array([30, 12], np.int32)
    gt = np.zeros((2, 4, 4), np.float32)
    gt[0, :3], gt[1, :1] = props[0, [3, 7, 9], :4] + np.float32(1), props[1, 20, :4]     # image 1: a padded proposal
    labels = np.array([[5, 6, 7, 0], [9, 0, 0, 0]], np.int64)
    out = R.sample_rois(props, counts, gt, labels, np.array([3, 1], np.int32), num=16, pos_fraction=0.25)
    rois, lab, lw, bt, bw, pg, npos, nneg = out
    assert rois.shape == (32, 5) and npos.tolist() == [4, 1] and nneg.tolist() == [12, 12]
    assert rois[16, 0] == 1 and np.array_equal(rois[16, 1:], gt[1, 0]) and lab[16] == 9 and pg[16] == 0
    assert np.all(rois[16 + 13:, 0] == -1) and np.all(lw[16 + 13:] == 0) and np.all(pg[17:] == -1)    # 1 + 12 rows used
    assert set(lab[:4].tolist()) <= {5, 6, 7} and np.all(lab[4:16] == 0) and np.all(bw[:4] == 1) and np.all(bw[4:16] == 0)
    assert np.all(bt[16] == 0)                                        # a ground truth against itself


# ---- host refusals (no GPU: shapes, dtypes, limits and scalars come first, the device last) --------------------------
def _refusals():
    import torch_detection_amd as T
    a, gt, cnt = torch.zeros(100, 4), torch.zeros(3, 5, 4), torch.zeros(3, dtype=torch.int32)
    assigned = torch.zeros(3, 100, dtype=torch.int32)
    props, pc, lab = torch.zeros(3, 50, 5), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 5, dtype=torch.int64)
    d = dict(anchors=a, valid_flags=torch.ones(3, 100, dtype=torch.uint8), gt_bboxes=gt, gt_counts=cnt,
             img_shapes=torch.ones(3, 2, dtype=torch.int32))
    return [
        (lambda: T.assign_max_iou(a.double(), gt, cnt, 0.7, 0.3), "boxes must be a contiguous float32"),
        (lambda: T.assign_max_iou(a, gt, cnt.long(), 0.7, 0.3), r"gt_counts must be a contiguous int32 \(3,\)"),
        (lambda: T.assign_max_iou(a, gt, cnt, 0.7, (0.1, 0.3)), "neg_iou_thr must be a number"),
        (lambda: T.assign_max_iou(a, gt, cnt, (0.7,), 0.3), "pos_iou_thr must be a number"),
        (lambda: T.assign_max_iou(a, gt, cnt, float("nan"), 0.3), "pos_iou_thr must be finite"),
        (lambda: T.assign_max_iou(a, torch.zeros(3, 257, 4), cnt, 0.7, 0.3), r"257 ground truths per image \(max 256\)"),
        (lambda: T.assign_max_iou(a, torch.zeros(65, 4, 4), torch.zeros(65, dtype=torch.int32), 0.7, 0.3),
         "batch size: the number of images must be in 1..64"),
        (lambda: T.assign_max_iou(a, gt[..., :3].contiguous(), cnt, 0.7, 0.3),
         r"gt_bboxes must be a contiguous float32 \(B, G, 4\)"),
        (lambda: T.assign_max_iou(torch.zeros(2, 100, 4), gt, cnt, 0.7, 0.3),
         r"boxes must be a contiguous float32 \(3, N, 4\)"),
        (lambda: T.assign_max_iou(a, gt, cnt, 0.7, 0.3, valid=torch.ones(3, 5, dtype=torch.uint8)),
         r"valid must be a contiguous uint8 / bool \(3, 100\)"),
        (lambda: T.assign_max_iou(a, gt, cnt, 0.7, 0.3), "boxes must be a CUDA tensor"),
        (lambda: T.sample_assigned(assigned, 8193, 0.5), "num must be in 0..8192"),
        (lambda: T.sample_assigned(assigned, 256, 1.5), r"pos_fraction must be in \[0, 1\]"),
        (lambda: T.sample_assigned(assigned.long(), 256, 0.5), r"assigned_gt_inds must be a contiguous int32 \(B, N\)"),
        (lambda: T.sample_assigned(assigned, 256, 0.5, keys=torch.zeros(3, 100)),
         r"keys must be a contiguous int32 \(3, 100\)"),
        (lambda: T.sample_assigned(assigned, 256, 0.5), "assigned_gt_inds must be a CUDA tensor"),
        (lambda: T.anchor_target(**dict(d, img_shapes=d["img_shapes"].float())),
         r"img_shapes must be a contiguous int32 \(3, 2\)"),
        (lambda: T.anchor_target(num=8193, **d), "num must be in 0..8192"),
        (lambda: T.anchor_target(neg_iou_thr=(0.0, 0.3), **d), "neg_iou_thr must be a number"),
        (lambda: T.anchor_target(target_stds=(1, 1, 1), **d), "target_stds must have 4 finite entries"),
        (lambda: T.anchor_target(**d), "anchors must be a CUDA tensor"),
        (lambda: T.sample_rois(props, pc, gt, lab, cnt, num=8193), "num must be in 0..8192"),
        (lambda: T.sample_rois(props[..., :4].contiguous(), pc, gt, lab, cnt),
         r"proposals must be a contiguous float32 \(3, P, 5\)"),
        (lambda: T.sample_rois(props, pc, gt, lab.int(), cnt), r"gt_labels must be a contiguous int64 \(3, 5\)"),
        (lambda: T.sample_rois(props, pc, gt, lab, cnt, keys=torch.zeros(3, 50, dtype=torch.int32)),
         r"keys must be a contiguous int32 \(3, 55\)"),                    # the ground truths are candidates too
        (lambda: T.sample_rois(props, pc, gt, lab, cnt), "proposals must be a CUDA tensor"),
    ]


@pytest.mark.parametrize("case", range(26))
def test_host_refusals_need_no_gpu(case):
    fn, msg = _refusals()[case]
    with pytest.raises(ValueError, match=msg):
        fn()


def test_host_refusal_table_is_run_in_full():
    assert len(_refusals()) == 26
