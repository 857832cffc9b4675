"""CPU: known answers of the box-delta / RPN-proposal oracle (tests/proposal_ref.py) and the C-ABI
layout of the new structs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import proposal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def sig(x):
    return f32(1) / (f32(1) + f32(np.exp(-np.float64(x))))


def test_zero_deltas_give_integer_anchors_back_and_encode_of_self_is_zero():
    g = np.random.default_rng(0)
    xy = g.integers(0, 1200, (500, 2))
    a = np.concatenate([xy, xy + g.integers(0, 400, (500, 2))], 1).astype(f32)
    out = R.delta2bbox(a, np.zeros((500, 8), f32))
    assert np.array_equal(out.view(np.uint32), np.tile(a, 2).view(np.uint32))
    assert np.array_equal(R.bbox2delta(a, a), np.zeros((500, 4), f32))
    assert np.array_equal(R.bbox2delta(a, a, (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2)), np.zeros((500, 4), f32))


def test_decode_of_encode_round_trips():
    g = np.random.default_rng(1)
    p = np.concatenate([g.uniform(0, 800, (1000, 2)), g.uniform(0, 800, (1000, 2)) + 900], 1).astype(f32)
    gt = np.concatenate([g.uniform(0, 800, (1000, 2)), g.uniform(0, 800, (1000, 2)) + 900], 1).astype(f32)
    means, stds = (0.1, 0.0, -0.1, 0.05), (0.1, 0.1, 0.2, 0.2)
    back = R.delta2bbox(p, R.bbox2delta(p, gt, means, stds), means, stds)
    assert np.allclose(back, gt, rtol=0, atol=2e-3)


def test_dw_dh_clamp_at_log_of_wh_ratio_clip():
    assert R.max_ratio() == f32(4.1351666) and R.max_ratio(16 / 1000) == f32(abs(np.log(0.016)))
    roi = np.array([[0, 0, 15, 15]], f32)                  # pw = ph = 16, centre 7.5
    big = R.delta2bbox(roi, np.array([[0, 0, 10, 10]], f32))
    at = R.delta2bbox(roi, np.array([[0, 0, 4.1351666, 4.1351666]], f32))
    assert np.array_equal(big, at)                         # clamped to exactly the limit
    gw = f32(16) * f32(np.exp(np.float64(f32(4.1351666))))
    assert abs(float(gw) - 1000.0) < 1e-3
    assert np.array_equal(big[0], np.array([7.5 - gw * f32(0.5) + f32(0.5), 7.5 - gw * f32(0.5) + f32(0.5),
                                            7.5 + gw * f32(0.5) - f32(0.5), 7.5 + gw * f32(0.5) - f32(0.5)], f32))
    small = R.delta2bbox(roi, np.array([[0, 0, -10, -10]], f32))
    assert np.array_equal(small, R.delta2bbox(roi, np.array([[0, 0, -4.1351666, -4.1351666]], f32)))
    assert abs(float(small[0, 2] - small[0, 0]) - (0.256 - 1)) < 1e-5


def test_clip_to_image():
    roi = np.array([[0, 0, 15, 15], [40, 30, 70, 60]], f32)
    d = np.array([[-1, -1, 0, 0], [0.5, 0.5, 0.3, 0.3]], f32)
    out = R.delta2bbox(roi, d, max_shape=(50, 60))
    assert out[:, 0::2].min() >= 0 and out[:, 0::2].max() <= 59 and out[:, 1::2].min() >= 0 and out[:, 1::2].max() <= 49
    assert np.array_equal(out[0], np.array([0, 0, 0, 0], f32))   # [-16, -16, -1, -1] clipped
    assert out[1, 2] == 59 and out[1, 3] == 49
    free = R.delta2bbox(roi, d)
    assert np.array_equal(out, np.minimum(np.maximum(free, 0), np.array([59, 49, 59, 49], f32)))


def _two_levels(l0, l1, a0=((0, 0, 15, 15), (16, 0, 31, 15))):
    cls = [np.array(l0, f32).reshape(1, 1, 1, 2), np.array(l1, f32).reshape(1, 1, 1, 1)]
    reg = [np.zeros((1, 4, 1, 2), f32), np.zeros((1, 4, 1, 1), f32)]
    anchors = [np.array(a0, f32), np.array([[0, 0, 31, 31]], f32)]
    return cls, reg, anchors


def test_hand_built_two_level_case():
    cls, reg, anchors = _two_levels([2.0, 1.0], [1.5])
    p, a, c = R.rpn_proposals(cls, reg, anchors, [(100, 100)], max_num=4)
    assert c.tolist() == [3] and a.tolist() == [[0, 2, 1, -1]]
    assert np.array_equal(p[0], np.array([[0, 0, 15, 15, sig(2.0)], [0, 0, 31, 31, sig(1.5)],
                                          [16, 0, 31, 15, sig(1.0)], [0, 0, 0, 0, 0]], f32))
    # nms_pre = 1: level 0 sends only its best anchor
    p, a, c = R.rpn_proposals(cls, reg, anchors, [(100, 100)], nms_pre=1, max_num=4)
    assert c.tolist() == [2] and a.tolist() == [[0, 2, -1, -1]]
    # max_num = 2 keeps the two best across levels
    p, a, c = R.rpn_proposals(cls, reg, anchors, [(100, 100)], max_num=2)
    assert a.tolist() == [[0, 2]]
    # NMS inside a level: IoU([0,0,15,15], [1,0,16,15]) = 240 / 272 > 0.7, the higher logit survives
    cls, reg, anchors = _two_levels([1.0, 2.0], [1.5], a0=((0, 0, 15, 15), (1, 0, 16, 15)))
    p, a, c = R.rpn_proposals(cls, reg, anchors, [(100, 100)], max_num=4)
    assert c.tolist() == [2] and a.tolist() == [[1, 2, -1, -1]]
    assert np.array_equal(p[0, :2], np.array([[1, 0, 16, 15, sig(2.0)], [0, 0, 31, 31, sig(1.5)]], f32))
    # ... but boxes of different levels never suppress each other (the level-1 box covers both)
    p, a, c = R.rpn_proposals(cls, reg, anchors, [(100, 100)], max_num=4, nms_thr=0.2)
    assert a.tolist() == [[1, 2, -1, -1]]
    # min_bbox_size drops the 16x16 boxes; clipping to a 10 x 20 image
    cls, reg, anchors = _two_levels([2.0, 1.0], [1.5])
    p, a, c = R.rpn_proposals(cls, reg, anchors, [(100, 100)], min_bbox_size=17, max_num=4)
    assert a.tolist() == [[2, -1, -1, -1]]
    p, a, c = R.rpn_proposals(cls, reg, anchors, [(10, 20)], max_num=4)
    assert np.array_equal(p[0, :3, :4], np.array([[0, 0, 15, 9], [0, 0, 19, 9], [16, 0, 19, 9]], f32))


def test_ties_go_to_the_lower_anchor():
    cls, reg, anchors = _two_levels([0.5, 0.5], [0.5])
    _, a, _ = R.rpn_proposals(cls, reg, anchors, [(100, 100)], max_num=3)
    assert a.tolist() == [[0, 1, 2]]                        # equal logits: level, then anchor
    _, a, _ = R.rpn_proposals(cls, reg, anchors, [(100, 100)], nms_pre=1, max_num=3)
    assert a.tolist() == [[0, 2, -1]]                       # the nms_pre cut takes the lower anchor
    _, a, _ = R.rpn_proposals(cls, reg, anchors, [(100, 100)], max_num=2)
    assert a.tolist() == [[0, 1]]
    cls, reg, anchors = _two_levels([-0.0, 0.0], [-1.0])    # -0.0 == +0.0
    _, a, _ = R.rpn_proposals(cls, reg, anchors, [(100, 100)], nms_pre=1, max_num=3)
    assert a.tolist() == [[0, 2, -1]]
    assert R.key_order(np.array([0.0, -0.0, 1.0, -0.0], f32)).tolist() == [2, 0, 1, 3]


def test_batched_nms_oracle_keeps_segments_apart():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60]], f32)
    scores = np.array([0.5, 0.9, 0.9, 0.1], f32)
    keep, kept, counts = R.batched_nms(boxes, scores, [0, 2, 4], 0.5)
    assert keep.tolist() == [0, 1, 1, 1] and kept.tolist() == [1, -1, 2, 3] and counts.tolist() == [1, 2]
    keep, kept, counts = R.batched_nms(boxes, scores, [0, 0, 4], 0.5)
    assert counts.tolist() == [0, 2] and kept.tolist() == [1, 3, -1, -1]


def test_rpn_struct_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of tdn_rpn_level and tdn_rpn_config as gcc lays them out == the ctypes mirrors."""
    from torch_detection_amd import _lib
    mirrors = {"tdn_rpn_level": _lib.RpnLevel, "tdn_rpn_config": _lib.RpnConfig}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {']
    for cname, cls in mirrors.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['printf("const F32 %d\\n", TDN_F32);', 'printf("const SEG %d\\n", TDN_NMS_SEG_MAX);',
              'printf("const LVL %d\\n", TDN_RPN_MAX_LEVELS);', 'printf("const NUM %d\\n", TDN_RPN_MAX_NUM);',
              'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    consts = {"F32": _lib.TDN_F32, "SEG": _lib.NMS_SEG_MAX, "LVL": _lib.RPN_MAX_LEVELS, "NUM": _lib.RPN_MAX_NUM}
    seen = 0
    for ln in subprocess.check_output([str(exe)]).decode().split("\n"):
        if not ln:
            continue
        cname, fname, val = ln.split()
        if cname == "const":
            assert consts[fname] == int(val), (fname, val)
            continue
        cls = mirrors[cname]
        got = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert got == int(val), (cname, fname, got, val)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in mirrors.values())


def test_rpn_host_validation_without_a_gpu():
    """tdn_rpn_proposals_workspace validates on the host: limits are reported through tdn_last_error."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    lv = (_lib.RpnLevel * 2)()
    for v, (h, w) in zip(lv, [(50, 84), (13, 21)]):
        v.dtype, v.H, v.W, v.A = _lib.TDN_BF16, h, w, 3
        v.logits = v.deltas = v.anchors = 256                # never dereferenced on the host
    cfg = _lib.RpnConfig(nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7)
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 2, ctypes.byref(cfg)) > 0
    cfg.nms_pre = 0                                          # 12600 anchors would enter NMS
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 2, ctypes.byref(cfg)) < 0
    assert b"NMS" in lib.tdn_last_error()
    cfg.nms_pre, cfg.max_num = 2000, 8193
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 2, ctypes.byref(cfg)) < 0
    cfg.max_num = 2000
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 65, ctypes.byref(cfg)) < 0
    assert lib.tdn_rpn_proposals_workspace(lv, 0, 2, ctypes.byref(cfg)) < 0
    lv[1].dtype = 1                                          # TDN_F16 is not an input type here
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 2, ctypes.byref(cfg)) < 0
    assert lib.tdn_batched_nms_workspace(10000, 3) > 0 and lib.tdn_batched_nms_workspace(-1, 3) < 0


def test_workspace_sizes_are_the_design_table():
    """DESIGN.md §5d worked by hand: every region rounded up to 256 bytes, in the table's order."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    # batched NMS, N = 1000, S = 5, pitch = ceil(1000 / 64) = 16:
    # order 4000 -> 4096, sboxes 16000 -> 16128, seg_start and seg_count 20 -> 256 each, mask 1000 * 16 * 8 = 128000
    assert lib.tdn_batched_nms_workspace(1000, 5) == 4096 + 16128 + 2 * 256 + 128000
    # the placeholders: N = 0 counts as one row (pitch 1), S = 0 as one segment: five regions of 256
    assert lib.tdn_batched_nms_workspace(0, 3) == 5 * 256 and lib.tdn_batched_nms_workspace(0, 0) == 5 * 256
    assert lib.tdn_batched_nms_workspace(10, -1) == -1
    # RPN, B = 2, levels 50 x 84 and 13 x 21 with A = 3, nms_pre = 2000: cap = (2000, 819), R = 2 * 2819 = 5638 rows,
    # S = 4 segments, pitch = ceil(2000 / 64) = 32:
    # seg_box 90208 -> 90368, seg_key and seg_aidx 22552 -> 22784 each, kept 45104 -> 45312,
    # seg_start / seg_count / num_kept 16 -> 256 each, mask 5638 * 32 * 8 = 1443328
    lv = (_lib.RpnLevel * 2)()
    for v, (h, w) in zip(lv, [(50, 84), (13, 21)]):
        v.dtype, v.H, v.W, v.A = _lib.TDN_BF16, h, w, 3
        v.logits = v.deltas = v.anchors = 256                # never dereferenced on the host
    cfg = _lib.RpnConfig(nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7)
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 2, ctypes.byref(cfg)) == 90368 + 2 * 22784 + 45312 + 3 * 256 + 1443328
    lv[0].H = lv[1].H = 0                                    # every level empty: one placeholder row, pitch 1
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 2, ctypes.byref(cfg)) == 8 * 256
    assert lib.tdn_rpn_proposals_workspace(lv, 2, 0, ctypes.byref(cfg)) == -1


# ---- host refusals (no GPU: shapes, dtypes, limits and scalars come first, the device last) --------------------------
def _refusals():
    import torch
    import torch_detection_amd as T
    cls = [torch.zeros(2, 3, 10, 12), torch.zeros(2, 3, 5, 6)]
    reg = [torch.zeros(2, 12, 10, 12), torch.zeros(2, 12, 5, 6)]
    anchors = [torch.zeros(360, 4), torch.zeros(90, 4)]
    ish = torch.ones(2, 2, dtype=torch.int32)

    def rpn(**kw):
        args = dict(cls_scores=cls, bbox_preds=reg, anchors=anchors, img_shapes=ish)
        args.update(kw)
        return lambda: T.rpn_proposals(**args)

    p, gt, d = torch.zeros(7, 4), torch.zeros(7, 4), torch.zeros(7, 8)
    s, off = torch.zeros(7), torch.tensor([0, 3, 7])
    return [
        (rpn(cls_scores=cls * 5, bbox_preds=reg * 5, anchors=anchors * 5), "rpn_proposals takes 1..8 levels"),
        (rpn(cls_scores=[c.half() for c in cls], bbox_preds=[r.half() for r in reg]),
         r"cls_scores\[0\] must be a float32 / bfloat16"),
        (rpn(bbox_preds=[reg[0][:, :8], reg[1]]), r"bbox_preds\[0\] must be a float32 \(2, 12, 10, 12\)"),
        (rpn(bbox_preds=[reg[0].bfloat16(), reg[1]]), r"bbox_preds\[0\] must be a float32 .* got bfloat16"),
        (rpn(anchors=[anchors[0][:-1], anchors[1]]), r"anchors\[0\] must be a contiguous float32 \(360, 4\)"),
        (rpn(img_shapes=ish[:1]), r"img_shapes must be a contiguous int32 \(2, 2\)"),
        (rpn(img_shapes=ish.float()), r"img_shapes must be a contiguous int32 \(2, 2\)"),
        (rpn(img_shapes=[(8, 8)]), "img_shapes must hold B positive"),
        (rpn(nms_pre=4097), "nms_pre must be in 0..4096"),
        (rpn(nms_pre=-1), "nms_pre must be in 0..4096"),
        (rpn(max_num=8193), "max_num must be in 1..8192"),
        (rpn(max_num=0), "max_num must be in 1..8192"),
        (rpn(nms_post=0), "nms_post must be >= 1"),
        (rpn(min_bbox_size=-1), "min_bbox_size must be >= 0"),
        (rpn(nms_thr=float("nan")), "nms_thr must be finite"),
        (rpn(target_stds=(1, 1, 1)), "target_stds must have 4 finite entries"),
        (rpn(cls_scores=[torch.zeros(1, 3, 70, 70)], bbox_preds=[torch.zeros(1, 12, 70, 70)],
             anchors=[torch.zeros(14700, 4)], img_shapes=[(560, 560)], nms_pre=0), "14700 anchors enter NMS with nms_pre=0"),
        (rpn(cls_scores=[torch.zeros(65, 3, 2, 2)], bbox_preds=[torch.zeros(65, 12, 2, 2)], anchors=[torch.zeros(12, 4)],
             img_shapes=[(8, 8)] * 65), "batch size: the number of images must be in 1..64"),
        (rpn(), r"cls_scores\[0\] must be a CUDA tensor"),
        (lambda: T.batched_nms(torch.zeros(5000, 4), torch.zeros(5000), torch.tensor([0, 5000]), 0.5),
         "a segment holds more than 4096 boxes"),
        (lambda: T.batched_nms(p, s, torch.tensor([0, 8]), 0.5), r"seg_offsets must be non-decreasing within \[0, 7\]"),
        (lambda: T.batched_nms(p, s, off.int(), 0.5), r"seg_offsets must be a int64 \(S\+1,\)"),
        (lambda: T.batched_nms(p, s[:6], off, 0.5), r"scores must be a contiguous float32 \(7,\)"),
        (lambda: T.batched_nms(p, s, off, 0.5), "boxes must be a CUDA tensor"),
        (lambda: T.bbox2delta(p, gt[:6]), r"gt must be a contiguous float32 \(7, 4\)"),
        (lambda: T.bbox2delta(p.double(), gt), r"proposals must be a contiguous float32 \(N, 4\)"),
        (lambda: T.bbox2delta(p, gt, stds=(1, 1, 1, float("inf"))), "stds must have 4 finite entries"),
        (lambda: T.bbox2delta(p, gt), "proposals must be a CUDA tensor"),
        (lambda: T.delta2bbox(p, d[:, :6].contiguous()), "deltas must have 4C columns"),
        (lambda: T.delta2bbox(p, d[:6]), r"deltas must be a contiguous float32 \(7, 4C\)"),
        (lambda: T.delta2bbox(p, d, wh_ratio_clip=1.0), r"wh_ratio_clip must be in \(0, 1\)"),
        (lambda: T.delta2bbox(p, d, max_shape=(0, 10)), "max_shape must be a positive"),
        (lambda: T.delta2bbox(p, d), "rois must be a CUDA tensor"),
    ]


def test_host_refusal_table_is_run_in_full():
    assert len(_refusals()) == 33


@pytest.mark.parametrize("case", range(33))
def test_host_refusals_need_no_gpu(case):
    fn, msg = _refusals()[case]
    with pytest.raises(ValueError, match=msg):
        fn()
