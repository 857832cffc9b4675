"""CPU: the test-time detection oracle (tests/detect_ref.py) against an independent restatement, hand
cases of the specification, and every refusal of the host wrappers, each matched by its message."""
import numpy as np
import pytest
import torch

import detect_ref as D

f32 = np.float32


# ---- an independent restatement: torch float64 softmax, a plain per-class loop with its own sort and its own NMS -----
def _iou(a, b):
    """'+1' IoU in fp32, one rounding per operation (exact for the integer boxes of these tests up to the division)."""
    one = f32(1)
    aa = ((a[2] - a[0]) + one) * ((a[3] - a[1]) + one)
    ab = ((b[2] - b[0]) + one) * ((b[3] - b[1]) + one)
    w = max((min(a[2], b[2]) - max(a[0], b[0])) + one, f32(0))
    h = max((min(a[3], b[3]) - max(a[1], b[1])) + one, f32(0))
    inter = f32(w) * f32(h)
    return inter / ((aa + ab) - inter)


def plain_multiclass_nms(boxes, scores, idx, B, score_thr, nms_thr, max_num):
    out = []
    for b in range(B):
        found = []
        for c in range(1, scores.shape[1]):
            cand = [r for r in range(scores.shape[0]) if idx[r] == b and scores[r, c] > f32(score_thr)]
            cand.sort(key=lambda r: (-float(scores[r, c]), r))
            kept = []
            for r in cand:
                bx = boxes[r] if boxes.shape[1] == 4 else boxes[r, 4 * (c - 1):4 * c]
                if all(not (_iou(k, bx) > f32(nms_thr)) for _, k in kept):
                    kept.append((r, bx))
            found += [(-float(scores[r, c]), c - 1, r, bx) for r, bx in kept]
        found.sort(key=lambda t: t[:3])
        out.append(found[:max_num])
    return out


def rand_case(seed, N, C, B, agnostic):
    g = np.random.default_rng(seed)
    centres = g.integers(0, 300, (6, 2))
    k = g.integers(0, 6, (N, 1 if agnostic else C - 1))
    xy = centres[k] + g.integers(-6, 7, k.shape + (2,))
    wh = g.integers(20, 40, k.shape + (2,))
    boxes = np.concatenate([xy, xy + wh], -1).reshape(N, -1).astype(f32)
    vals = np.concatenate([[0.05], np.arange(1, 50) / 50.0]).astype(f32)
    scores = g.choice(vals, (N, C)).astype(f32)
    idx = g.integers(-1, B, N).astype(np.int64)
    return boxes, scores, idx


@pytest.mark.parametrize("seed,N,C,B,agnostic,max_num", [(1, 40, 4, 2, False, 100), (2, 57, 3, 3, True, 7),
                                                         (3, 30, 2, 1, False, 1)])
def test_oracle_against_plain_loop(seed, N, C, B, agnostic, max_num):
    boxes, scores, idx = rand_case(seed, N, C, B, agnostic)
    st = {}
    dets, labels, rows, counts = D.multiclass_nms(boxes, scores, idx, B, 0.05, 0.5, max_num, st)
    ref = plain_multiclass_nms(boxes, scores, idx, B, 0.05, 0.5, max_num)
    assert sum(st["suppressed"]) > 0
    for b in range(B):
        assert counts[b] == len(ref[b])
        for p, (ns, cl, r, bx) in enumerate(ref[b]):
            assert (labels[b, p], rows[b, p]) == (cl, r)
            assert np.array_equal(dets[b, p, :4], bx) and dets[b, p, 4] == f32(-ns)
        assert not dets[b, len(ref[b]):].any()
        assert (labels[b, len(ref[b]):] == -1).all() and (rows[b, len(ref[b]):] == -1).all()


def test_softmax_against_torch_float64():
    g = np.random.default_rng(5)
    x = (g.normal(0, 3, (33, 81))).astype(f32)
    x[::5, 7] += 20                                            # a dominant class
    p, z = D.softmax64(x)
    ref = torch.softmax(torch.from_numpy(x).double(), dim=1).numpy()
    assert np.allclose(p, ref, rtol=1e-14, atol=0)
    assert np.array_equal(z.max(axis=1), np.zeros(33))


def test_dense_matches_delta2bbox_and_scale():
    import proposal_ref as P
    g = np.random.default_rng(6)
    R, C = 9, 4
    xy = g.uniform(0, 200, (R, 2)).astype(f32)
    rois = np.concatenate([g.integers(-1, 2, (R, 1)).astype(f32), xy, xy + g.uniform(8, 90, (R, 2)).astype(f32)], 1)
    cls, reg = g.normal(0, 1, (R, C)).astype(f32), g.normal(0, 1, (R, 4 * C)).astype(f32)
    shapes = [(210, 260), (180, 300)]
    out = D.bbox_head_detections(rois, cls, reg, shapes, scale_factors=np.asarray([2.0, 0.75], f32), score_thr=0.0)
    scores, boxes = out[4], out[5]
    for r in range(R):
        b = int(rois[r, 0])
        if b < 0:
            assert not scores[r].any() and not boxes[r].any()
            continue
        ref = P.delta2bbox(rois[r:r + 1, 1:], reg[r:r + 1, 4:], (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2), shapes[b])
        assert np.array_equal(boxes[r], (ref[0] / f32([2.0, 0.75][b])).astype(f32))
        assert abs(float(scores[r].sum()) - 1) < 1e-6
    assert (out[2][out[2] >= 0] < R).all() and (rois[out[2][0][:out[3][0]], 0] == 0).all()


# ---- hand cases ----------------------------------------------------------------------------------------------------
BOX = f32([10, 10, 29, 29])


def _run(boxes, scores, idx=None, B=1, thr=0.05, max_num=4):
    return D.multiclass_nms(np.asarray(boxes, f32), np.asarray(scores, f32), idx, B, thr, 0.5, max_num)


def test_score_equal_to_the_threshold_is_no_candidate():
    up = np.nextafter(f32(0.05), f32(1))
    dets, labels, rows, counts = _run([BOX, BOX + 100], [[0, f32(0.05)], [0, up]])
    assert counts.tolist() == [1] and rows[0].tolist() == [1, -1, -1, -1] and dets[0, 0, 4] == up


def test_same_box_two_classes_survive_same_class_leaves_one():
    dets, labels, rows, counts = _run([BOX, BOX], [[0, 0.9, 0.1], [0, 0.1, 0.8]], thr=0.5)
    assert counts.tolist() == [2] and labels[0, :2].tolist() == [0, 1] and rows[0, :2].tolist() == [0, 1]
    dets, labels, rows, counts = _run([BOX, BOX], [[0, 0.9, 0.0], [0, 0.8, 0.0]])
    assert counts.tolist() == [1] and rows[0, 0] == 0 and dets[0, 0, 4] == f32(0.9)


def test_ties_come_out_in_class_then_row_order_and_padding():
    far = [BOX + 100 * i for i in range(3)]
    boxes = np.stack([np.concatenate([far[i], far[i]]) for i in range(3)])      # (3, 8): two foreground classes
    scores = [[0, 0.5, 0.5], [0, 0.5, 0.5], [0, 0.7, 0.5]]
    dets, labels, rows, counts = _run(boxes, scores, max_num=8)
    assert counts.tolist() == [6]
    assert list(zip(labels[0, :6].tolist(), rows[0, :6].tolist())) == [(0, 2), (0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    assert not dets[0, 6:].any() and labels[0, 6:].tolist() == [-1, -1] and rows[0, 6:].tolist() == [-1, -1]
    assert dets.dtype == f32 and labels.dtype == np.int64 and rows.dtype == np.int64 and counts.dtype == np.int32
    # truncation keeps the head of the same order; -0.0 ties with +0.0
    dets, labels, rows, counts = _run(boxes, [[0, -0.0, 0.0], [0, 0.0, -0.0], [0, -1, -1]], thr=-0.5, max_num=3)
    assert list(zip(labels[0].tolist(), rows[0].tolist())) == [(0, 0), (0, 1), (1, 0)] and counts.tolist() == [3]


def test_image_without_rows_and_ignored_rows():
    idx = np.asarray([2, -1, 2, 7])
    dets, labels, rows, counts = _run([BOX, BOX, BOX + 50, BOX], [[0, 0.9]] * 4, idx, B=3)
    assert counts.tolist() == [0, 0, 2] and rows[2, :2].tolist() == [0, 2] and not dets[:2].any()


def test_oversized_segment_empties_its_image_only():
    n = D.SEG_MAX + 1
    boxes = np.zeros((n + 2, 4), f32)
    boxes[:, 0] = boxes[:, 2] = np.arange(n + 2) * 3
    scores = np.zeros((n + 2, 2), f32)
    scores[:, 1] = 0.5
    idx = np.asarray([0] * n + [1, 1])
    dets, labels, rows, counts = D.multiclass_nms(boxes, scores, idx, 2, 0.05, 0.5, 5)
    assert counts.tolist() == [-1, 2] and not dets[0].any() and (rows[0] == -1).all() and rows[1, :2].tolist() == [n, n + 1]
    idx[0] = -1                                               # exactly SEG_MAX candidates is fine
    assert D.multiclass_nms(boxes, scores, idx, 2, 0.05, 0.5, 5)[3].tolist() == [5, 2]


# ---- host refusals (no GPU: shapes and limits come first, the device last) --------------------------------------------
def _mc(**kw):
    a = dict(multi_bboxes=torch.zeros(6, 8), multi_scores=torch.zeros(6, 3), batch_idx=torch.zeros(6, dtype=torch.int64),
             num_imgs=2, score_thr=0.05, nms_thr=0.5, max_num=100)
    a.update(kw)
    return a


MC_REFUSALS = [
    (dict(multi_scores=torch.zeros(6, 3, dtype=torch.float64)), "multi_scores must be a contiguous float32"),
    (dict(multi_scores=torch.zeros(3, 6).t()), "multi_scores must be a contiguous float32"),
    (dict(multi_scores=torch.zeros(6, 1), multi_bboxes=torch.zeros(6, 4)), "C must be in 2..1024"),
    (dict(multi_scores=torch.zeros(1, 1025), multi_bboxes=torch.zeros(1, 4)), "C must be in 2..1024"),
    (dict(multi_scores=torch.zeros((1 << 18) + 1, 2), multi_bboxes=torch.zeros((1 << 18) + 1, 4),
          batch_idx=None, num_imgs=1), r"rows \(max 262144\)"),
    (dict(num_imgs=0), "number of images must be in 1..64"),
    (dict(num_imgs=65), "number of images must be in 1..64"),
    (dict(max_num=0), "max_num must be in 1..8192"),
    (dict(max_num=8193), "max_num must be in 1..8192"),
    (dict(score_thr=float("nan")), "score_thr must be finite"),
    (dict(nms_thr=float("inf")), "nms_thr must be finite"),
    (dict(multi_bboxes=torch.zeros(6, 12)), r"multi_bboxes must be a contiguous float32 \(6, 8 or 4\)"),
    (dict(multi_bboxes=torch.zeros(5, 8)), "multi_bboxes must be a contiguous float32"),
    (dict(batch_idx=None), "batch_idx=None means one image"),
    (dict(batch_idx=torch.zeros(6)), "batch_idx must be a contiguous int32 / int64"),
    (dict(batch_idx=torch.zeros(5, dtype=torch.int32)), "batch_idx must be a contiguous int32 / int64"),
    (dict(), "multi_scores must be a CUDA tensor"),
]


@pytest.mark.parametrize("case", range(len(MC_REFUSALS)))
def test_multiclass_nms_refusals(case):
    import torch_detection_amd as T
    kw, msg = MC_REFUSALS[case]
    with pytest.raises(ValueError, match=msg):
        T.multiclass_nms(**_mc(**kw))


def _bh(**kw):
    a = dict(rois=torch.zeros(6, 5), cls_score=torch.zeros(6, 3), bbox_pred=torch.zeros(6, 12),
             img_shapes=torch.ones(2, 2, dtype=torch.int32))
    a.update(kw)
    return a


BH_REFUSALS = [
    (dict(rois=torch.zeros(6, 4)), r"rois must be a contiguous float32 \(R, 5\)"),
    (dict(cls_score=torch.zeros(6, 3, dtype=torch.float64)), r"cls_score must be a contiguous float32 / bfloat16 / float16 \(6, C\)"),
    (dict(cls_score=torch.zeros(5, 3)), r"cls_score must be a contiguous float32 / bfloat16 / float16 \(6, C\)"),
    (dict(img_shapes=torch.ones(2, 2, dtype=torch.int64)), "img_shapes must be a contiguous int32"),
    (dict(img_shapes=[(4, 4), (4, 4)]), "img_shapes must be a contiguous int32"),
    (dict(img_shapes=torch.ones(65, 2, dtype=torch.int32)), "number of images must be in 1..64"),
    (dict(cls_score=torch.zeros(6, 1), bbox_pred=torch.zeros(6, 4)), "C must be in 2..1024"),
    (dict(rois=torch.zeros((1 << 18) + 1, 5), cls_score=torch.zeros((1 << 18) + 1, 2),
          bbox_pred=torch.zeros((1 << 18) + 1, 4)), r"rows \(max 262144\)"),
    (dict(max_per_img=0), "max_num must be in 1..8192"),
    (dict(score_thr=float("inf")), "score_thr must be finite"),
    (dict(bbox_pred=torch.zeros(6, 8)), r"bbox_pred must be a contiguous float32 \(6, 12 or 4\)"),
    (dict(bbox_pred=torch.zeros(6, 12, dtype=torch.float16)), r"bbox_pred must be a contiguous float32 \(6, 12 or 4\) tensor, got float16"),
    (dict(scale_factors=torch.ones(3)), r"scale_factors must be a contiguous float32 \(2,\)"),
    (dict(scale_factors=0.0), "scale_factors must be finite and > 0"),
    (dict(scale_factors=(1.0, 1.0)), "scale_factors must be a number"),
    (dict(target_stds=(0.1, 0.1, 0.2)), "target_stds must have 4 finite entries"),
    (dict(target_means=(0, 0, 0, float("nan"))), "target_means must have 4 finite entries"),
    (dict(wh_ratio_clip=1.0), r"wh_ratio_clip must be in \(0, 1\)"),
    (dict(), "rois must be a CUDA tensor"),
]


@pytest.mark.parametrize("case", range(len(BH_REFUSALS)))
def test_bbox_head_detections_refusals(case):
    import torch_detection_amd as T
    kw, msg = BH_REFUSALS[case]
    with pytest.raises(ValueError, match=msg):
        T.bbox_head_detections(**_bh(**kw))


def test_ws_bytes_reads_a_negative_answer_as_the_librarys_refusal():
    from torch_detection_amd import _lib
    lib = _lib.load()
    with pytest.raises(ValueError, match=r"^multiclass_nms: .*C=1 out of 2\.\.1024"):
        _lib.ws_bytes(lib.tdn_multiclass_nms_workspace_bytes(10, 1, 1), "multiclass_nms")
    n = lib.tdn_multiclass_nms_workspace_bytes(1000, 81, 2)
    assert n > 0 and _lib.ws_bytes(n, "multiclass_nms") == n


def test_workspace_queries_share_one_layout_and_refuse_like_the_call():
    from torch_detection_amd import _lib
    lib = _lib.load()
    a = lib.tdn_multiclass_nms_workspace_bytes(1000, 81, 2)
    assert a == lib.tdn_bbox_detections_workspace_bytes(1000, 81, 2) > 0 and a % 256 == 0
    # pitch follows the row bound: 1000 rows per segment need 16 mask words a row, not 64
    rows = 2 * 80 * 1000
    assert a == sum(-(-rows * e // 256) * 256 for e in (16, 4, 4, 8, 8 * 16)) + 3 * 256 * -(-160 * 4 // 256)
    assert lib.tdn_multiclass_nms_workspace_bytes(0, 2, 1) > 0            # placeholders: no region is empty
    assert lib.tdn_multiclass_nms_workspace_bytes(10, 1, 1) == -1 and b"C=1 out of 2..1024" in lib.tdn_last_error()
    assert lib.tdn_bbox_detections_workspace_bytes(10, 3, 65) == -1 and b"B=65 out of 1..64" in lib.tdn_last_error()
    assert lib.tdn_multiclass_nms_workspace_bytes((1 << 18) + 1, 3, 1) == -1 and b"rows (max" in lib.tdn_last_error()
