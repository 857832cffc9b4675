"""CPU tests of the soft-NMS oracle tests/soft_nms_ref.py and of everything of the soft path that needs
no GPU: the arg-max formulation against a transcription of mmdetection's swap-based ``soft_nms_cpu`` loop, ``naive``
against the greedy oracle, ``soft_exp`` against float64 ``exp`` within the bound DESIGN.md derives, hand cases at the
edges of every comparison, every refusal (Python and C) by its message, and the workspace query against the layout
written out.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import detect_ref as D
import soft_nms_ref as R

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"linear": dict(type="soft_nms", method="linear", iou_thr=0.3, min_score=0.05),
       "gaussian": dict(type="soft_nms", method="gaussian", sigma=0.5, min_score=0.05),
       "naive": dict(type="soft_nms", method="naive", iou_thr=0.3, min_score=0.05)}


def boxes_scores(n, seed):
    """The issue's prototype draw: xy uniform in [0, 60), sides in [4, 40); tie-free scores in (0.05, 1)."""
    g = np.random.default_rng(seed)
    xy = g.uniform(0, 60, (n, 2))
    wh = g.uniform(4, 40, (n, 2))
    boxes = np.concatenate([xy, xy + wh], 1).astype(f32)
    scores = (0.06 + 0.93 * (g.permutation(n) + g.uniform(0.1, 0.9, n)) / n).astype(f32)
    assert np.unique(scores).shape[0] == n
    return boxes, scores


# ---- against the swap form -------------------------------------------------------------------------------------------
def soft_nms_swap(boxes, scores, method, iou_thr, sigma, min_score):
    """mmdetection v1's soft_nms_cpu, loop for loop: scan for the maximum, swap it to the front, decay the tail,
    swap-remove what falls under min_score.  The arithmetic of one pair is soft_nms_ref.decay's."""
    b, s = boxes.copy(), scores.copy()
    inds = np.arange(s.shape[0])
    N, i = s.shape[0], 0
    while i < N:
        maxpos = i
        for pos in range(i + 1, N):
            if s[maxpos] < s[pos]:
                maxpos = pos
        for a in (b, s, inds):
            a[[i, maxpos]] = a[[maxpos, i]]
        pos = i + 1
        while pos < N:
            touched, new = R.decay(b[i], b[pos:pos + 1], s[pos:pos + 1], method, iou_thr, sigma)
            if touched[0]:
                s[pos] = new[0]
                if s[pos] < min_score:
                    b[pos], s[pos], inds[pos] = b[N - 1], s[N - 1], inds[N - 1]
                    N -= 1
                    pos -= 1
            pos += 1
        i += 1
    return inds[:N], s[:N]


SEEN = {"lowered": 0, "dropped": 0}


@pytest.mark.parametrize("method", sorted(CFG))
@pytest.mark.parametrize("n", [1, 2, 7, 65, 130])
def test_argmax_form_equals_the_swap_form(n, method):
    boxes, scores = boxes_scores(n, 10 * n + len(method))
    m, iou_thr, sigma, min_score = R.normalise(CFG[method])
    order, final = R.soft_nms_segment(boxes, scores, np.arange(n), m, iou_thr, sigma, min_score)
    inds, s = soft_nms_swap(boxes, scores, m, iou_thr, sigma, min_score)
    assert order.tolist() == inds.tolist()
    assert np.array_equal(final[order].view(np.uint32), s.view(np.uint32))
    assert (np.diff(final[order]) <= 0).all(), "final scores are non-increasing in selection order"
    SEEN["lowered"] += int((final[order] < scores[order]).sum())
    SEEN["dropped"] += n - order.shape[0]


def test_the_swap_form_cases_were_not_hollow():
    """Counts what the parametrised test above did IN THIS RUN (run the file as a whole)."""
    assert SEEN["lowered"] > 50 and SEEN["dropped"] > 50, SEEN


# ---- naive is greedy NMS ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_score", [0.05, 0.01, 1e-30])
def test_naive_equals_hard_nms(min_score):
    g = np.random.default_rng(3)
    N, C, B = 400, 4, 2
    xy = g.uniform(0, 120, (N, C - 1, 2))
    wh = g.uniform(8, 50, (N, C - 1, 2))
    boxes = np.concatenate([xy, xy + wh], -1).reshape(N, 4 * (C - 1)).astype(f32)
    scores = g.uniform(0, 1, (N, C)).astype(f32)
    idx = g.integers(-1, B, N)
    st = {}
    ref = D.multiclass_nms(boxes, scores, idx, B, 0.05, 0.4, 50, st)
    assert sum(st["suppressed"]) > 100
    got = R.multiclass_nms(boxes, scores, idx, B, 0.05, dict(type="soft_nms", method="naive", iou_thr=0.4,
                                                             min_score=min_score), 50)
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == f32 else a,
                                                     b.view(np.uint32) if b.dtype == f32 else b)


# ---- soft_exp --------------------------------------------------------------------------------------------------------
def test_soft_exp_within_the_derived_bound():
    """Relative error against float64 exp of the same float32 argument <= 4 * 2^-24 (0.35 u from the
    reduction, 0.18 u truncation, 3.39 u Horner roundings, 0.02 u coefficients), on 2^20 + points of [-64, 0]."""
    x = np.concatenate([np.linspace(-64, 0, (1 << 20) + 1), -np.logspace(-30, 1.8, 4097), [-64.0, 0.0, -0.0],
                        -np.log(2) * (np.arange(0, 93) + 0.5)]).astype(f32)
    x = x[(x >= -64) & (x <= 0)]
    got = R.soft_exp(x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    rel = np.abs(got - ref) / ref
    print("soft_exp: worst relative error %.3f u at x = %r" % (rel.max() / R.U, float(x[rel.argmax()])))
    assert rel.max() <= R.SOFT_EXP_REL_BOUND
    assert R.soft_exp(f32(0)) == f32(1) and R.soft_exp(f32(-64)) > 0
    assert (got >= 2.0 ** -126).all(), "the weight stays normal"
    # outside the range: clamped, a NaN goes to -64
    out = R.soft_exp(np.asarray([1.0, -100.0, np.nan, -np.inf], f32))
    assert out[0] == 1 and out[1] == out[2] == out[3] == R.soft_exp(f32(-64))


def test_soft_exp_constants_are_the_header_s():
    src = open(os.path.join(ROOT, "torch_detection_amd", "csrc", "soft_nms_core.h")).read()
    val = {k: f32(float.fromhex(v)) for k, v in re.findall(r"SOFT_(\w+) = (0x[0-9a-f.]+p[+-]?\d+)f", src)}
    assert sorted(val) == ["C2", "C3", "C4", "C5", "C6", "C7", "LN2_HI", "LN2_LO", "LOG2E"]
    assert [val["C%d" % i] for i in range(7, 1, -1)] == R.COEF[:6] and R.COEF[6:] == [1, 1]
    assert (val["LOG2E"], val["LN2_HI"], val["LN2_LO"]) == (R.LOG2E, R.LN2_HI, R.LN2_LO)
    assert [val["C%d" % i] for i in range(2, 8)] == [f32(1 / np.prod(np.arange(1.0, i + 1))) for i in range(2, 8)]
    assert int(re.search(r"SOFT_WAVE_MAX = 64 \* SOFT_PER", src) is not None) and "SOFT_PER = 4;" in src
    assert R.WAVE_MAX == 64 * 4


# ---- hand cases ------------------------------------------------------------------------------------------------------
A_BOX = f32([0, 0, 9, 9])                    # area 100


def seg(boxes, scores, rows=None, **kw):
    cfg = dict(type="soft_nms")
    cfg.update(kw)
    n = len(scores)
    return R.soft_nms_segment(np.asarray(boxes, f32), np.asarray(scores, f32), np.arange(n) if rows is None else rows,
                              *R.normalise(cfg))


def test_min_score_edge_equal_stays_one_ulp_under_goes():
    b = f32([0, 0, 9, 6])                    # inside A: inter 70, union 100, ov 0.7
    ov = f32(70) / f32(100)
    decayed = f32(f32(1) - ov) * f32(0.8)
    for method, d in (("linear", decayed), ("gaussian", R.soft_exp(-((ov * ov) / f32(0.5))) * f32(0.8))):
        d = f32(d)
        order, final = seg([A_BOX, b], [0.9, 0.8], method=method, iou_thr=0.5, min_score=d)
        assert order.tolist() == [0, 1] and final[1].view(np.uint32) == d.view(np.uint32) and d < f32(0.8)
        order, final = seg([A_BOX, b], [0.9, 0.8], method=method, iou_thr=0.5, min_score=np.nextafter(d, f32(1)))
        assert order.tolist() == [0]


def test_ov_equal_to_iou_thr_gives_weight_one():
    b = f32([0, 0, 9, 4])                    # inter 50, union 100: ov is exactly 0.5
    for method in ("linear", "naive"):
        order, final = seg([A_BOX, b], [0.9, 0.8], method=method, iou_thr=0.5, min_score=0.79)
        assert order.tolist() == [0, 1] and final[1] == f32(0.8)
        order, final = seg([A_BOX, b], [0.9, 0.8], method=method, iou_thr=np.nextafter(f32(0.5), f32(0)),
                           min_score=0.79)
        assert order.tolist() == [0]


def test_touching_boxes_are_left_alone():
    b = f32([10, 0, 19, 9])                  # w = min(9, 19) - max(0, 10) + 1 = 0
    c = f32([9, 0, 18, 9])                   # w = 1: it overlaps
    for method in sorted(R.METHODS):
        order, final = seg([A_BOX, b, c], [0.9, 0.8, 0.7], method=method, iou_thr=0.0, min_score=0.0)
        assert final[1] == f32(0.8), method
        assert final[2] < f32(0.7), method
        # an untouched candidate is not compared with min_score either (soft_nms_cpu's nesting)
        order, _ = seg([A_BOX, b], [0.9, 0.8], method=method, min_score=0.85)
        assert order.tolist() == [0, 1]


def test_tie_of_an_undecayed_and_a_decayed_score_goes_to_the_lower_row():
    b = f32([0, 0, 9, 6])
    far = f32([100, 100, 109, 109])
    d = f32(f32(1) - f32(70) / f32(100)) * f32(0.8)
    order, final = seg([A_BOX, b, far], [0.9, 0.8, d], rows=np.asarray([0, 2, 1]), method="linear", iou_thr=0.5,
                       min_score=0.0)
    assert final[1] == final[2] == d and order.tolist() == [0, 2, 1]
    order, final = seg([A_BOX, b, far], [0.9, 0.8, d], rows=np.asarray([0, 1, 2]), method="linear", iou_thr=0.5,
                       min_score=0.0)
    assert order.tolist() == [0, 1, 2]


def test_equal_scores_in_two_classes_and_an_empty_segment():
    boxes = np.stack([A_BOX, A_BOX + 100, A_BOX + 200]).astype(f32)
    scores = f32([[0, 0.5, 0.0, 0.5], [0, 0.7, 0.0, 0.5], [0, 0.5, 0.0, 0.9]])     # class 2 has no candidate
    dets, labels, rows, counts = R.multiclass_nms(boxes, scores, None, 1, 0.05, CFG["linear"], 10)
    assert counts.tolist() == [6]
    assert labels[0, :6].tolist() == [2, 0, 0, 0, 2, 2] and rows[0, :6].tolist() == [2, 1, 0, 2, 0, 1]
    assert dets[0, :6, 4].tolist() == [f32(0.9), f32(0.7), 0.5, 0.5, 0.5, 0.5]
    assert (labels[0, 6:] == -1).all() and not dets[0, 6:].any()
    # no candidate at all
    dets, labels, rows, counts = R.multiclass_nms(boxes, scores, None, 1, 0.95, CFG["linear"], 4)
    assert counts.tolist() == [0] and not dets.any() and (rows == -1).all()


def test_4096_candidates_run_and_4097_do_not():
    g = np.random.default_rng(5)
    n = 4097
    xy = g.uniform(0, 3000, (n, 2))
    boxes = np.concatenate([xy, xy + g.uniform(8, 60, (n, 2))], 1).astype(f32)
    scores = np.zeros((n, 2), f32)
    scores[:, 1] = g.uniform(0.1, 1, n)
    idx = np.zeros(n, np.int64)
    idx[-1] = 1
    st = {}
    out = R.multiclass_nms(boxes, scores, idx, 2, 0.05, CFG["gaussian"], 100, st)
    assert out[3].tolist() == [100, 1] and st["sizes"] == [4096, 1] and st["lowered"] > 0
    idx[-1] = 0
    out = R.multiclass_nms(boxes, scores, idx, 2, 0.05, CFG["gaussian"], 100)
    assert out[3].tolist() == [-1, 0] and not out[0].any()


# ---- refusals --------------------------------------------------------------------------------------------------------
PY_REFUSALS = [
    (dict(type="softnms"), 0.5, r"unknown type 'softnms'"),
    (dict(iou_thr=0.5), 0.5, r"unknown type None"),
    (dict(type="soft_nms", iou_threshold=0.5), 0.5, r"unknown key 'iou_threshold' for type 'soft_nms'"),
    (dict(type="nms", min_score=0.1), 0.5, r"unknown key 'min_score' for type 'nms'"),
    (dict(type="soft_nms", method="exp"), 0.5, r"method 'exp' is not one of 'linear', 'gaussian', 'naive'"),
    (dict(type="soft_nms", method=1), 0.5, r"method 1 is not one of"),
    (dict(type="soft_nms", iou_thr=float("nan")), 0.5, r"nms\['iou_thr'\] must be finite"),
    (dict(type="soft_nms", min_score=float("inf")), 0.5, r"nms\['min_score'\] must be finite"),
    (dict(type="soft_nms", sigma=float("nan")), 0.5, r"nms\['sigma'\] must be finite"),
    (dict(type="soft_nms", sigma=0.01), 0.5, r"nms\['sigma'\] must lie in \[1/64, 64\], got 0.01"),
    (dict(type="soft_nms", sigma=64.5), 0.5, r"nms\['sigma'\] must lie in \[1/64, 64\], got 64.5"),
    (dict(type="soft_nms", min_score=-0.001), 0.5, r"nms\['min_score'\] must be >= 0"),
    (dict(type="soft_nms"), 0.3, r"either as nms_thr or in nms\['iou_thr'\], not both"),
    (dict(type="nms", iou_thr=0.3), 0.6, r"either as nms_thr or in nms\['iou_thr'\], not both"),
    ("soft_nms", 0.5, r"nms must be None or a dict"),
]


@pytest.mark.parametrize("nms,nms_thr,msg", PY_REFUSALS)
def test_python_refusals_come_before_any_device_is_touched(nms, nms_thr, msg):
    """CPU tensors: a refusal of ``nms`` is raised before the device check, which would refuse these."""
    import torch_detection_amd as T
    with pytest.raises(ValueError, match=msg):
        T.multiclass_nms(torch.zeros(3, 4), torch.zeros(3, 2), None, 1, nms_thr=nms_thr, nms=nms)
    ish = torch.tensor([[64, 64]], dtype=torch.int32)
    with pytest.raises(ValueError, match=msg):
        T.bbox_head_detections(torch.zeros(3, 5), torch.zeros(3, 2), torch.zeros(3, 8), ish, nms_thr=nms_thr, nms=nms)
    with pytest.raises(ValueError, match=msg):
        T.cascade_detections(torch.zeros(3, 5), [torch.zeros(3, 2)], torch.zeros(3, 8), ish, nms_thr=nms_thr, nms=nms)
    with pytest.raises(ValueError, match=msg):
        T.anchor_head_detections([torch.zeros(1, 2, 4, 4)], [torch.zeros(1, 4, 4, 4)], torch.zeros(16, 4), ish,
                                 nms_thr=nms_thr, nms=nms)
    with pytest.raises(ValueError, match=msg):
        T.fcos_detections([torch.zeros(1, 2, 4, 4)], [torch.zeros(1, 4, 4, 4)], [torch.zeros(1, 1, 4, 4)], [8], ish,
                          nms_thr=nms_thr, nms=nms)


def test_accepted_forms_reach_the_device_check():
    import torch_detection_amd as T
    for nms in (None, dict(type="nms", iou_thr=0.3), dict(type="soft_nms"),
                dict(type="soft_nms", method="gaussian", sigma=1 / 64), dict(type="soft_nms", sigma=64, min_score=0)):
        with pytest.raises(ValueError, match="must be a CUDA tensor"):
            T.multiclass_nms(torch.zeros(3, 4), torch.zeros(3, 2), None, 1, nms=nms)
    with pytest.raises(ValueError, match="must be a CUDA tensor"):
        T.multiclass_nms(torch.zeros(3, 4), torch.zeros(3, 2), None, 1, nms_thr=0.3)


C_REFUSALS = [((3, 0.5, 0.5, 0.001), b"soft-NMS method 3 is not naive (0), linear (1) or gaussian (2)"),
              ((-1, 0.5, 0.5, 0.001), b"soft-NMS method -1 is not"),
              ((1, float("nan"), 0.5, 0.001), b"soft-NMS iou_thr / min_score / sigma must be finite"),
              ((1, 0.5, float("inf"), 0.001), b"soft-NMS iou_thr / min_score / sigma must be finite"),
              ((1, 0.5, 0.5, float("-inf")), b"soft-NMS iou_thr / min_score / sigma must be finite"),
              ((2, 0.5, 0.015, 0.001), b"soft-NMS sigma=0.015 outside [1/64, 64]"),
              ((2, 0.5, 65.0, 0.001), b"soft-NMS sigma=65 outside [1/64, 64]"),
              ((1, 0.5, 0.5, -0.5), b"soft-NMS min_score=-0.5 is negative"),
              (None, b"NULL soft-NMS config")]


@pytest.mark.parametrize("fields,msg", C_REFUSALS)
def test_c_entry_points_refuse_before_the_first_launch(fields, msg):
    """Every pointer is NULL and no stream exists: a launch, or any check behind the soft-NMS ones, would not get here."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    soft = None if fields is None else ctypes.byref(_lib.SoftNmsConfig(*fields))
    N = None
    calls = {
        "tdn_multiclass_nms_soft": lambda: lib.tdn_multiclass_nms_soft(N, 4, N, N, 0, 8, 3, 1, 0.05, soft, 10, N, N, N, N,
                                                                       N, 0, N),
        "tdn_bbox_detections_soft": lambda: lib.tdn_bbox_detections_soft(N, N, N, 2, 8, 3, 12, 1, N, N, 0.0, N, N, 0.016,
                                                                         0.05, soft, 10, N, N, N, N, N, N, N, 0, N),
        "tdn_cascade_detections_soft": lambda: lib.tdn_cascade_detections_soft(N, N, 1, N, 2, 8, 3, 12, 1, N, N, 0.0, N, N,
                                                                               0.016, 0.05, soft, 10, N, N, N, N, N, N, N,
                                                                               0, N),
        "tdn_dense_detections_soft": lambda: lib.tdn_dense_detections_soft(N, 1, 1, N, N, N, soft, N, N, N, N, N, N, N, N,
                                                                           N, N, 0, N),
        "tdn_fcos_detections_soft": lambda: lib.tdn_fcos_detections_soft(N, 1, 1, N, N, N, N, soft, N, N, N, N, N, N, N, N,
                                                                         N, N, 0, N),
    }
    for name, call in calls.items():
        assert call() == -1, name
        err = lib.tdn_last_error()
        assert err.startswith(name.encode() + b": ") and msg in err, (name, err)


# ---- workspace -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,B", [(0, 2, 1), (1, 2, 1), (63, 5, 3), (1000, 81, 2), (4096, 81, 1), (5000, 3, 64),
                                   (1 << 18, 1024, 1)])
def test_workspace_query_is_the_layout_written_out(N, C, B):
    from torch_detection_amd import _lib
    lib = _lib.load()
    want = R.workspace_bytes(N, C, B)
    for q in (lib.tdn_multiclass_nms_soft_workspace_bytes, lib.tdn_bbox_detections_soft_workspace_bytes,
              lib.tdn_cascade_detections_soft_workspace_bytes):
        assert q(N, C, B) == want
    hard = lib.tdn_multiclass_nms_workspace_bytes(N, C, B)
    assert hard == R.hard_workspace_bytes(N, C, B)
    assert want <= hard and (N < 64 or want < hard), "no suppression mask: the soft workspace is the smaller one"


def test_workspace_queries_of_the_pyramid_entry_points():
    from torch_detection_amd import _lib, dense_detect_ops, fcos_ops
    lib = _lib.load()
    arr, L, A, C = dense_detect_ops._levels([(8, 8), (4, 4)], 3, 5)
    cfg, _ = dense_detect_ops._config(torch.float32, A, C, 100, 10, 0.05, 0.5, (0, 0, 0, 0), (1, 1, 1, 1), 0.016)
    rows = 2 * (100 + 48)                                         # B * K: the first level selects 100 of 192
    hard = lib.tdn_dense_detections_workspace_bytes(arr, L, 2, ctypes.byref(cfg))
    soft = lib.tdn_dense_detections_soft_workspace_bytes(arr, L, 2, ctypes.byref(cfg))
    assert hard - soft == R.hard_workspace_bytes(rows, C + 1, 2) - R.workspace_bytes(rows, C + 1, 2) > 0
    arr, L, _ = fcos_ops._pyramid([(8, 8), (4, 4)], [8, 16])
    cfg, _ = fcos_ops._det_config(torch.float32, 5, 0, 10, 0.05, 0.5)
    rows = 2 * 80
    hard = lib.tdn_fcos_detections_workspace_bytes(arr, L, 2, ctypes.byref(cfg))
    soft = lib.tdn_fcos_detections_soft_workspace_bytes(arr, L, 2, ctypes.byref(cfg))
    assert hard - soft == R.hard_workspace_bytes(rows, 6, 2) - R.workspace_bytes(rows, 6, 2) > 0
    assert soft == R.workspace_bytes(rows, 6, 2)                 # no level selects: no key words in front
