"""GPU tests of soft-NMS — the ``nms=dict(type='soft_nms', ...)`` path of multiclass_nms,
bbox_head_detections, cascade_detections, anchor_head_detections and fcos_detections — against the CPU oracle
tests/soft_nms_ref.py, bit for bit: selection order, decayed scores, labels, rows and counts.  The four head entry points
are compared with the oracle run on the GPU's own dense scores and boxes (as tests/test_gpu_detect.py does), which are
themselves the greedy path's, bit for bit.

Every multiclass case asserts on the ORACLE's result that it is not hollow: for 'linear' and 'gaussian' at least one
survivor with a lowered score, one candidate dropped by min_score and one segment whose selection order differs from its
input order; 'naive' never lowers a survivor's score (its weights are 0 and 1), so there only the drops are asserted.
"""
import numpy as np
import pytest
import torch

import guard_util as G
import soft_nms_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
THR = 0.05
METHODS = {"linear": dict(type="soft_nms", method="linear", iou_thr=0.3, min_score=0.05),
           "gaussian": dict(type="soft_nms", method="gaussian", sigma=0.5, min_score=0.05),
           "naive": dict(type="soft_nms", method="naive", iou_thr=0.3, min_score=0.05)}


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()       # a copy: the oracle's arrays are read-only


def assert_same(got, ref, what=""):
    names = ("dets", "labels", "row_idx", "counts", "idx")
    for name, g, r in zip(names, got, ref):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.dtype, r.shape)
        if g.dtype == np.float32:
            g, r = g.view(np.uint32), r.view(np.uint32)
        assert np.array_equal(g, r), "%s: %s differs at %s" % (what, name, np.argwhere(g != r)[:4].tolist())


def same_tensors(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


# ---- multiclass_nms ---------------------------------------------------------------------------------------------------
def mc_case(seed, per_img, C, agnostic, exact, p_cand, span):
    """Rows of B images interleaved at random with rows of index -1 and B among them.  Boxes: xy uniform in [0, span),
    sides in [4, 40) (the issue's prototype draw, span scaled to the segment sizes); scores uniform, a fraction p_cand
    of them above the threshold, a few exact duplicates.  ``exact``: {image: n} makes exactly n rows of that image
    candidates of class 1."""
    g = np.random.default_rng(seed)
    B = len(per_img)
    idx = []
    for b, n in enumerate(per_img):
        idx += [b] * n
    idx += [-1] * 5 + [B, -7]
    idx = np.asarray(g.permutation(idx), np.int64)
    N = idx.shape[0]
    K = 1 if agnostic else C - 1
    xy = g.uniform(0, span, (N, K, 2))
    wh = g.uniform(4, 40, (N, K, 2))
    boxes = np.concatenate([xy, xy + wh], -1).reshape(N, 4 * K).astype(f32)
    scores = np.where(g.random((N, C)) < p_cand, g.uniform(0.06, 1.0, (N, C)), g.uniform(0.0, THR, (N, C))).astype(f32)
    scores[g.integers(0, N, N // 8), g.integers(0, C, N // 8)] = f32(0.5)          # ties, decided by the row
    scores[g.integers(0, N, 3), g.integers(0, C, 3)] = f32(THR)                     # at the threshold: no candidate
    for b, n in exact.items():
        rows = np.nonzero(idx == b)[0]
        scores[rows, 1] = f32(THR)
        scores[rows[:n], 1] = g.uniform(0.06, 1.0, n)
    return boxes, scores, idx, B


CUT = R.WAVE_MAX
MC_CASES = {
    # name: (seed, rows per image, C, agnostic, max_num, index dtype, exact class-1 segment sizes, p_cand, span)
    "seg_0_1_2_c5": (1, (60, 60, 60), 5, False, 100, np.int32, {0: 0, 1: 1, 2: 2}, 0.6, 60),
    "seg_63_64_65_c2_top1": (2, (130, 130, 130), 2, True, 1, np.int64, {0: 63, 1: 64, 2: 65}, 0.5, 70),
    "seg_cut_c2": (3, (CUT + 40, CUT + 40, CUT + 40), 2, False, 100, np.int32, {0: CUT - 1, 1: CUT, 2: CUT + 1}, 0.5,
                   150),
    "seg_1000_c81": (4, (1000,), 81, False, 100, np.int64, {0: 1000}, 0.04, 70),
    "seg_1000_c81_agnostic_top1": (5, (1000,), 81, True, 1, np.int32, {0: 1000}, 0.04, 300),
    "seg_4096_4097_c5": (6, (4100, 4200, 70), 5, True, 100, np.int32, {0: 4096, 1: 4097}, 0.01, 900),
}
ORACLE = {}                             # (case, method) -> (inputs, oracle outputs, stats): computed once, never changed


def oracle(name, method):
    if (name, method) not in ORACLE:
        seed, per_img, C, agnostic, max_num, idt, exact, p_cand, span = MC_CASES[name]
        boxes, scores, idx, B = mc_case(seed, per_img, C, agnostic, exact, p_cand, span)
        st = {}
        ref = R.multiclass_nms(boxes, scores, idx, B, THR, METHODS[method], max_num, st)
        for a in (boxes, scores, idx) + ref:
            a.setflags(write=False)
        ORACLE[name, method] = ((boxes, scores, idx.astype(idt), B, max_num), ref, st)
    return ORACLE[name, method]


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("name", sorted(MC_CASES))
def test_multiclass_soft_nms_bit_exact(T, name, method):
    (boxes, scores, idx, B, max_num), ref, st = oracle(name, method)
    exact = MC_CASES[name][6]
    for b, n in exact.items():                        # the segment sizes the case is about, as the oracle saw them
        assert st["sizes"][b * (scores.shape[1] - 1)] == n, (name, b, st["sizes"][:8])
    print("%s %s: lowered %d dropped %d reordered %d total %s" % (name, method, st["lowered"], st["dropped"],
                                                                  st["reordered"], st["total"]))
    assert st["dropped"] >= 1
    if method != "naive":
        assert st["lowered"] >= 1 and st["reordered"] >= 1
    if 4097 in exact.values():
        assert ref[3].tolist()[:2] == [max_num, -1] and ref[3][2] > 0
    args = (_cuda(boxes), _cuda(scores), _cuda(idx), B)
    got = T.multiclass_nms(*args, score_thr=THR, max_num=max_num, nms=METHODS[method])
    assert_same(got, ref, "%s %s" % (name, method))
    again = T.multiclass_nms(*args, score_thr=THR, max_num=max_num, nms=METHODS[method])
    assert same_tensors(got, again), "two eager calls"


@pytest.mark.parametrize("name", sorted(MC_CASES))
def test_naive_at_the_score_threshold_is_the_hard_path(T, name):
    """'naive' with min_score = score_thr against the greedy kernels on the same inputs: all four outputs, bit for bit."""
    (boxes, scores, idx, B, max_num), _, _ = oracle(name, "naive")
    args = (_cuda(boxes), _cuda(scores), _cuda(idx), B)
    hard = T.multiclass_nms(*args, score_thr=THR, nms_thr=0.3, max_num=max_num)
    soft = T.multiclass_nms(*args, score_thr=THR, max_num=max_num,
                            nms=dict(type="soft_nms", method="naive", iou_thr=0.3, min_score=THR))
    assert same_tensors(soft, hard)
    assert (hard[3] != 0).any()


def test_nms_none_and_type_nms_are_the_greedy_path(T):
    (boxes, scores, idx, B, max_num), _, _ = oracle("seg_63_64_65_c2_top1", "naive")
    args = (_cuda(boxes), _cuda(scores), _cuda(idx), B)
    for t in (0.5, 0.3):
        base = T.multiclass_nms(*args, THR, t, 100)
        assert same_tensors(T.multiclass_nms(*args, THR, t, 100, nms=None), base)
        assert same_tensors(T.multiclass_nms(*args, THR, max_num=100, nms=dict(type="nms", iou_thr=t)), base)
    assert not same_tensors(T.multiclass_nms(*args, THR, 0.5, 100), T.multiclass_nms(*args, THR, 0.3, 100))


def test_empty_inputs(T):
    z = torch.zeros(0, 8, device="cuda"), torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda")
    dets, labels, rows, counts = T.multiclass_nms(*z, 2, max_num=3, nms=METHODS["gaussian"])
    assert counts.tolist() == [0, 0] and not dets.any() and (labels == -1).all() and (rows == -1).all()


# ---- the four head entry points ---------------------------------------------------------------------------------------
SHAPES = [(300, 400), (280, 360)]
HEAD_NMS = {m: dict(cfg, min_score=0.3) for m, cfg in METHODS.items()}      # a few RoIs: drops need a higher bar


def head_inputs(R_, C, seed):
    """CPU tensors (rois, cls, reg, img_shapes).  R_ < 64: one tight cluster of one class, all but one row in image 0 (a
    handful of rows must still lower and drop scores); else two images, random classes, a tenth of the rows padding."""
    g = np.random.default_rng(seed)
    B = len(SHAPES)
    small = R_ < 64
    xy = g.uniform(0, 12 if small else 160, (R_, 2))
    wh = g.uniform(40 if small else 20, 60, (R_, 2))
    img = g.integers(0, B, (R_, 1)).astype(np.float64)
    img[g.random((R_, 1)) < 0.1] = -1
    if small:
        img[:] = 0
        img[R_ // 2] = -1
        img[R_ - 1] = 1
    rois = np.concatenate([img, xy, xy + wh], 1).astype(f32)
    x = g.normal(0, 1.0, (R_, C))
    x[np.arange(R_), 1 if small else g.integers(1, C, R_)] += 4.0
    d = g.normal(0, 0.1 if small else 0.3, (R_, 4 * C))
    return (torch.from_numpy(rois), torch.from_numpy(x).float(), torch.from_numpy(d).float(),
            torch.tensor(SHAPES, dtype=torch.int32))


def cascade_stages(cls, seed):
    g = torch.Generator().manual_seed(seed)
    return [cls, cls + 0.5 * torch.randn(cls.shape, generator=g), (cls + 0.25 * torch.randn(cls.shape, generator=g))]


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("R_", [7, 512])
def test_bbox_head_and_cascade_detections(T, R_, method):
    rois, cls, reg, ish = [t.cuda() for t in head_inputs(R_, 5, 40 + R_)]
    nms = HEAD_NMS[method]
    kw = dict(score_thr=THR, max_per_img=30, return_dense=True)
    out = T.bbox_head_detections(rois, cls, reg, ish, 1.25, nms=nms, **kw)
    hard = T.bbox_head_detections(rois, cls, reg, ish, 1.25, **kw)
    assert same_tensors(out[4:], hard[4:]), "the dense scores and boxes are the greedy path's"
    st = {}
    ref = R.select_rois(rois.cpu().numpy(), out[4].cpu().numpy(), out[5].cpu().numpy(), len(SHAPES), THR, nms, 30, st)
    assert_same(out[:4], ref, "bbox_head R%d %s" % (R_, method))
    assert st["dropped"] >= 1 and (method == "naive" or st["lowered"] >= 1) and (out[3] > 0).all()
    assert same_tensors(T.bbox_head_detections(rois, cls, reg, ish, 1.25, score_thr=THR, max_per_img=30, nms=nms), out[:4])
    # the cascade: three stages whose mean is taken on the device; one stage is bbox_head_detections itself
    stages = [t.cuda() for t in cascade_stages(cls.cpu(), R_)]
    cas = T.cascade_detections(rois, stages, reg, ish, 1.25, nms=nms, **kw)
    st = {}
    ref = R.select_rois(rois.cpu().numpy(), cas[4].cpu().numpy(), cas[5].cpu().numpy(), len(SHAPES), THR, nms, 30, st)
    assert_same(cas[:4], ref, "cascade R%d %s" % (R_, method))
    assert same_tensors(cas[4:], T.cascade_detections(rois, stages, reg, ish, 1.25, **kw)[4:])
    assert st["dropped"] >= 1 and (cas[3] > 0).all()
    assert same_tensors(T.cascade_detections(rois, [cls], reg, ish, 1.25, nms=nms, **kw), out)


LEVELS = [(8, 8), (4, 4)]


def anchor_inputs():
    """CPU tensors of a two-level pyramid, B = 2, A = 3, C = 4: (cls_scores, bbox_preds, anchors, img_shapes)."""
    g = np.random.default_rng(7)
    B, A, C = 2, 3, 4
    cls = [torch.from_numpy(g.normal(-1, 1.5, (B, A * C, h, w)).astype(f32)) for h, w in LEVELS]
    reg = [torch.from_numpy(g.normal(0, 0.2, (B, 4 * A, h, w)).astype(f32)) for h, w in LEVELS]
    anchors = []
    for h, w in LEVELS:
        xy = g.uniform(0, 100, (h * w * A, 2))
        anchors.append(torch.from_numpy(np.concatenate([xy, xy + g.uniform(16, 48, (h * w * A, 2))], 1).astype(f32)))
    return cls, reg, anchors, torch.tensor([(160, 160), (150, 170)], dtype=torch.int32)


def fcos_inputs():
    """CPU tensors of a two-level pyramid, B = 2, C = 4: (cls_scores, bbox_preds, centernesses, img_shapes); distances
    around e^2.8 = 16 pixels at strides 8 and 16, so neighbouring points' boxes overlap."""
    g = np.random.default_rng(8)
    B, C = 2, 4
    cls = [torch.from_numpy(g.normal(0, 1.5, (B, C, h, w)).astype(f32)) for h, w in LEVELS]
    reg = [torch.from_numpy(g.normal(2.8, 0.4, (B, 4, h, w)).astype(f32)) for h, w in LEVELS]
    ctr = [torch.from_numpy(g.normal(1, 1.0, (B, 1, h, w)).astype(f32)) for h, w in LEVELS]
    return cls, reg, ctr, torch.tensor([(64, 64), (60, 70)], dtype=torch.int32)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_anchor_head_detections(T, method):
    B = 2
    cls, reg, anchors, ish = anchor_inputs()
    cls, reg, anchors, ish = [t.cuda() for t in cls], [t.cuda() for t in reg], [t.cuda() for t in anchors], ish.cuda()
    nms = METHODS[method]
    kw = dict(nms_pre=100, score_thr=THR, max_per_img=40, return_dense=True)
    out = T.anchor_head_detections(cls, reg, anchors, ish, nms=nms, **kw)
    hard = T.anchor_head_detections(cls, reg, anchors, ish, **kw)
    assert same_tensors(out[4:8], hard[4:8]), "the dense tensors are the greedy path's"
    st = {}
    ref = R.select_dense(out[5].cpu().numpy(), out[4].cpu().numpy(), out[6].cpu().numpy(), out[7].cpu().numpy(), B, THR,
                         nms, 40, st)
    assert_same((out[0], out[1], out[8], out[3], out[2]), (ref[0], ref[1], ref[4], ref[3], ref[2]), "anchor " + method)
    assert st["dropped"] >= 1 and (method == "naive" or (st["lowered"] >= 1 and st["reordered"] >= 1))
    assert (out[3] > 0).all()
    assert same_tensors(T.anchor_head_detections(cls, reg, anchors, ish, nms_pre=100, score_thr=THR, max_per_img=40,
                                                 nms=nms), out[:4])


@pytest.mark.parametrize("method", sorted(METHODS))
def test_fcos_detections(T, method):
    B = 2
    cls, reg, ctr, ish = fcos_inputs()
    cls, reg, ctr, ish = [t.cuda() for t in cls], [t.cuda() for t in reg], [t.cuda() for t in ctr], ish.cuda()
    nms = METHODS[method]
    kw = dict(nms_pre=50, score_thr=THR, max_per_img=40, return_dense=True)
    out = T.fcos_detections(cls, reg, ctr, [8, 16], ish, nms=nms, **kw)
    hard = T.fcos_detections(cls, reg, ctr, [8, 16], ish, **kw)
    assert same_tensors(out[4:8], hard[4:8]), "the dense tensors are the greedy path's"
    st = {}
    ref = R.select_dense(out[5].cpu().numpy(), out[4].cpu().numpy(), out[6].cpu().numpy(), out[7].cpu().numpy(), B, THR,
                         nms, 40, st)
    assert_same((out[0], out[1], out[8], out[3], out[2]), (ref[0], ref[1], ref[4], ref[3], ref[2]), "fcos " + method)
    assert st["dropped"] >= 1 and (method == "naive" or (st["lowered"] >= 1 and st["reordered"] >= 1))
    assert (out[3] > 0).all()
    assert same_tensors(T.fcos_detections(cls, reg, ctr, [8, 16], ish, nms_pre=50, score_thr=THR, max_per_img=40,
                                          nms=nms), out[:4])


def test_heads_forward_the_nms_dict(T):
    """RetinaHead.get_bboxes and FCOSHead.get_bboxes pass ``nms`` on with the rest of the test_cfg."""
    import inspect
    for fn in (T.multiclass_nms, T.bbox_head_detections, T.cascade_detections, T.anchor_head_detections,
               T.fcos_detections, T.CascadeRoIHead.simple_test):
        assert inspect.signature(fn).parameters["nms"].default is None, fn
    from torch_detection_amd import heads
    seen = {}
    real = heads.anchor_head_detections, heads.fcos_detections
    try:
        heads.anchor_head_detections = lambda *a, **k: seen.setdefault("retina", k)
        heads.fcos_detections = lambda *a, **k: seen.setdefault("fcos", k)
        heads.RetinaHead.get_bboxes(type("H", (), dict(target_means=0, target_stds=1))(), [], [], [], None,
                                    nms=METHODS["linear"])

        class F(object):
            strides = [8]
            scale_vector = staticmethod(lambda: torch.ones(1))
        heads.FCOSHead.get_bboxes(F(), [0], [0], [0], None, nms=METHODS["gaussian"])
    finally:
        heads.anchor_head_detections, heads.fcos_detections = real
    assert seen["retina"]["nms"] is METHODS["linear"] and seen["fcos"]["nms"] is METHODS["gaussian"]


# ---- graph capture ------------------------------------------------------------------------------------------------------
def test_graph_replay_on_new_inputs_equals_eager(T):
    """Captured once, replayed on new boxes and scores: no host synchronisation, no allocation inside the library."""
    def new(seed):
        b, s, i, _ = mc_case(seed, (300, 90), 7, False, {0: CUT + 20}, 0.3, 120)
        return [torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(i)]
    bufs = [t.cuda() for t in new(1)]

    def step():
        out = []
        for m in sorted(METHODS):
            out += list(T.multiclass_nms(bufs[0], bufs[1], bufs[2], 2, THR, max_num=40, nms=METHODS[m]))
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    seen = []
    for seed in (2, 3):
        with torch.no_grad():
            for dst, src in zip(bufs, new(seed)):
                dst.copy_(src)
        graph.replay()
        eager = step()
        torch.cuda.synchronize()
        assert same_tensors(captured, eager)
        seen.append(captured[0].clone())
    assert not torch.equal(seen[0], seen[1])


# ---- under the guard ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["seg_0_1_2_c5", "seg_cut_c2", "seg_4096_4097_c5"])
def test_guarded_soft_multiclass_nms(T, monkeypatch, name):
    """Poisoned outputs (the unused rows and the oversized image's rows must have been WRITTEN) and a workspace of
    exactly the queried size, both between guard bands."""
    from torch_detection_amd import _lib, detect_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, detect_ops, g)
    for method in sorted(METHODS):
        test_multiclass_soft_nms_bit_exact(T, name, method)
    log = list(g.ws_log)
    found = g.check()
    torch.cuda.synchronize()
    assert not found, "\n".join(found)
    (boxes, scores, idx, B, _), _, _ = oracle(name, "linear")
    want = _lib.load().tdn_multiclass_nms_soft_workspace_bytes(scores.shape[0], scores.shape[1], B)
    assert want == R.workspace_bytes(scores.shape[0], scores.shape[1], B)
    assert len(log) == 6 and all(op == "multiclass_nms" and asked == want and 0 <= given - asked < 256
                                 for op, asked, given in log), log
