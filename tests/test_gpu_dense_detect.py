"""GPU tests of the single-stage head operations (anchor_head_detections, anchor_target_all) against the
CPU oracle tests/dense_detect_ref.py.

Detections: batch_idx, anchor_idx and the background column exactly; the dense sigmoid within (16 + |x|)·2^-24·p64 +
2^-149 of float64 (derivable: (4 + |x|)u; 16 is §4f's margin); the dense boxes within §4b's decode tolerance and
bit-exact where dw = dh = 0; every final output bit-equal to the oracle's selection run on the GPU's own dense values;
multiclass_nms on the dense tensors reproduces them.  Targets: everything exactly but dw / dh, which are held to
test_gpu_targets' comparison.  Then the two with anchor_head_loss, graph capture, and both wrappers under the guard of
tests/guard_util.py.

Every case asserts on the ORACLE's result that it is not hollow; the last test of the file counts what ran IN THIS RUN
(run the file as a whole).
"""
import inspect

import numpy as np
import pytest
import torch

import dense_detect_cases as K
import dense_detect_ref as DD
import guard_util as G
import test_gpu_losses as TL
import test_gpu_targets as TG

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24
THR, NMS_THR = 0.05, 0.5
SEEN = {"over": 0, "under": 0, "cut": 0}     # cases with survivors above / below max_per_img, with a straddled cut
ENTERED, WS_SEEN = set(), {}                  # what ran under the guard in this run
ONE = [((1, 1), 64)]


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, ref, names, what):
    for name, g, r in zip(names, got, ref):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.dtype, r.shape)
        if g.dtype == np.float32:
            g, r = g.view(np.uint32), r.view(np.uint32)
        assert np.array_equal(g, r), "%s: %s differs at %s" % (what, name, np.argwhere(g != r)[:4].tolist())


# ---- detections --------------------------------------------------------------------------------------------------------
DET_CASES = {
    # name: (levels, A, C, B, dtype, layout, nms_pre, max_per_img, scale, seed)
    "c5_b3_f32_nchw_pre100": (K.LEVELS, 9, 5, 3, "f32", "nchw", 100, 100, "none", 1),
    "c5_b1_bf16_nhwc_pre100_top20": (K.LEVELS, 9, 5, 1, "bf16", "nhwc", 100, 20, "number", 1),
    "c5_b3_f16_mixed_pre216_all": (K.LEVELS, 9, 5, 3, "f16", "mixed", 216, 8192, "tensor", 1),
    "c1_b1_f32_mixed_pre100_top1": (K.LEVELS, 9, 1, 1, "f32", "mixed", 100, 1, "tensor", 1),
    "c1_b3_bf16_nchw_pre0": (K.LEVELS, 9, 1, 3, "bf16", "nchw", 0, 100, "none", 1),
    "c80_b1_f16_nhwc_pre4096": (K.LEVELS, 9, 80, 1, "f16", "nhwc", 4096, 100, "number", 1),
    "c80_b3_bf16_nhwc_pre100_top20": (K.LEVELS, 9, 80, 3, "bf16", "nhwc", 100, 20, "none", 1),
    "c80_b1_f32_nchw_pre216_all": (K.LEVELS, 9, 80, 1, "f32", "nchw", 216, 8192, "tensor", 1),
    "c5_b3_bf16_mixed_pre215": (K.LEVELS, 9, 5, 3, "bf16", "mixed", 215, 100, "number", 1),
    "c5_b1_f16_nchw_pre217": (K.LEVELS, 9, 5, 1, "f16", "nchw", 217, 100, "none", 1),
    # every level selects; the 54-anchor level's tile ends inside a 16-byte vector, odd images start off a boundary
    "c5_b3_bf16_nhwc_pre50": (K.LEVELS, 9, 5, 3, "bf16", "nhwc", 50, 100, "none", 1),
    "c5_b3_f32_nhwc_pre50": (K.LEVELS, 9, 5, 3, "f32", "nhwc", 50, 100, "number", 1),
    # 9216 anchors: more than one 8192-key step of the selection
    "big_c5_b1_bf16_nhwc_pre100": (K.BIG, 9, 5, 1, "bf16", "nhwc", 100, 100, "none", 1),
    "big_c5_b3_f32_nchw_pre4096": (K.BIG, 9, 5, 3, "f32", "nchw", 4096, 100, "number", 1),
    "big_c1_b1_f16_nhwc_pre1000": (K.BIG, 9, 1, 1, "f16", "nhwc", 1000, 100, "none", 1),
    # one 1 x 1 level with one anchor
    "one_c5_b3_f32": (ONE, 1, 5, 3, "f32", "nchw", 100, 100, "none", 1),
    "one_c1_b1_bf16": (ONE, 1, 1, 1, "bf16", "nhwc", 0, 1, "tensor", 1),
}


def det_inputs(name):
    levels, A, C, Bn, dt, layout, nms_pre, max_per_img, scale_kind, seed = DET_CASES[name]
    cls, reg = K.head_case(levels, Bn, A, C, K.DTYPES[dt], layout, seed)
    scale = {"none": None, "number": 1.25, "tensor": np.linspace(0.8, 1.6, Bn).astype(f32)}[scale_kind]
    return dict(cls=cls, reg=reg, anchors=K.pyramid(levels, A), shapes=K.img_shapes(Bn, levels), scale=scale, nms_pre=nms_pre,
                max_per_img=max_per_img, A=A, C=C, B=Bn, sizes=[h * w * A for (h, w), _ in levels])


def det_oracle(case):
    """The oracle's dense tensors and the conditions that make the case worth running."""
    info = {}
    d = DD.dense(K.stored(case["cls"]), K.stored(case["reg"]), case["anchors"], case["shapes"], case["scale"],
                 case["nms_pre"], K.MEANS, K.STDS, info=info)
    if any(0 < case["nms_pre"] < n for n in case["sizes"]):
        assert len(info["cuts"]) == case["B"] * sum(0 < case["nms_pre"] < n for n in case["sizes"])
        if max(case["sizes"]) > 1:
            good = [c for c in info["cuts"] if c["above"] > 0 and c["ties"] > c["taken"]]
            assert good, "no level with keys above the cut and a straddled tie: %s" % info["cuts"]
            SEEN["cut"] += 1
    return d


def decode_tolerance(rois, deltas):
    """§4b: 4·spacing(max(|gx|, gw, 1)) per x coordinate (y alike), from float64 stand-ins."""
    dd = deltas.astype(np.float64) * np.asarray(K.STDS) + np.asarray(K.MEANS)
    tol = np.empty(dd.shape, np.float64)
    for ax in (0, 1):
        pw = ((rois[:, 2 + ax] - rois[:, ax]) + 1).astype(np.float64)
        gw = pw * np.exp(np.clip(dd[:, 2 + ax], -4.1351666, 4.1351666))
        gx = np.abs((rois[:, ax] + rois[:, 2 + ax]) * 0.5 + pw * dd[:, ax])
        t = 4 * np.spacing(np.maximum(np.maximum(gx, gw), 1.0).astype(f32)).astype(np.float64)
        tol[:, ax], tol[:, 2 + ax] = t, t
    return tol


def run_det(T, name, case=None):
    case = case or det_inputs(name)
    d = det_oracle(case)
    Bn, C = case["B"], case["C"]
    scale = case["scale"]
    args = ([t.cuda() for t in case["cls"]], [t.cuda() for t in case["reg"]], [_cuda(a) for a in case["anchors"]],
            _cuda(case["shapes"]), _cuda(scale) if isinstance(scale, np.ndarray) else scale)
    for t, s in zip(args[0] + args[1], case["cls"] + case["reg"]):
        assert t.stride() == s.stride()
    kw = dict(nms_pre=case["nms_pre"], score_thr=THR, nms_thr=NMS_THR, max_per_img=case["max_per_img"],
              target_means=K.MEANS, target_stds=K.STDS)
    out = T.anchor_head_detections(*args, return_dense=True, **kw)
    assert len(out) == 9
    scores, boxes, bidx, aidx = (t.cpu().numpy() for t in out[4:8])
    # 1. what is exact
    _same((bidx, aidx), (d["batch_idx"], d["anchor_idx"]), ("batch_idx", "dense_anchor_idx"), name)
    assert scores.dtype == f32 and scores.shape == d["scores"].shape and not scores[:, 0].any()
    assert np.array_equal(scores[:, 0].view(np.uint32), np.zeros(scores.shape[0], np.uint32)), "column 0 is +0"
    # 2. dense scores against float64
    x = d["logits"].astype(np.float64)
    assert np.abs(x).max() <= 64
    p64 = 1.0 / (1.0 + np.exp(-x))
    err = np.abs(scores[:, 1:].astype(np.float64) - p64)
    bound = (16 + np.abs(x)) * U * p64 + 2.0 ** -149
    print("%s: scores worst error / bound %.3g" % (name, (err / bound).max()))
    assert (err <= bound).all(), "scores: worst error / bound %.3g" % (err / bound).max()
    # 3. dense boxes
    assert boxes.dtype == f32 and boxes.shape == d["boxes"].shape
    tol = decode_tolerance(d["rois"], d["deltas"])
    ref = d["boxes_unscaled"].astype(np.float64)
    if d["scale"] is not None:
        ref = ref / d["scale"][:, None].astype(np.float64)
        tol = tol / d["scale"][:, None] + np.spacing(np.abs(ref).astype(f32))
    berr = np.abs(boxes.astype(np.float64) - ref)
    print("%s: boxes worst error / tolerance %.3g" % (name, (berr / np.maximum(tol, 1e-300)).max()))
    assert (berr <= tol).all(), "boxes: worst error / tolerance %.3g" % (berr / np.maximum(tol, 1e-300)).max()
    flat = (d["deltas"][:, 2:] == 0).all(axis=1)
    assert flat.sum() >= flat.shape[0] // 4 or flat.shape[0] < 4
    assert np.array_equal(boxes[flat].view(np.uint32), d["boxes"][flat].view(np.uint32)), "exp-free rows are bit-exact"
    # 4. final outputs: the oracle's selection on the GPU's own dense values
    st = {}
    ref_out = DD.select(boxes, scores, bidx, aidx, Bn, THR, NMS_THR, case["max_per_img"], st)
    names = ("dets", "labels", "anchor_idx", "counts", "row_idx")
    _same((out[0], out[1], out[2], out[3], out[8]), ref_out, names, name)
    SEEN["over"] += any(t > case["max_per_img"] for t in st["total"])
    SEEN["under"] += any(0 <= t < case["max_per_img"] for t in st["total"])
    # 5. the selection does not depend on return_dense, and multiclass_nms on the dense tensors reproduces it
    plain = T.anchor_head_detections(*args, **kw)
    assert len(plain) == 4
    for a, b in zip(plain, out[:4]):
        assert torch.equal(a, b)
    mc = T.multiclass_nms(out[5], out[4], out[6], Bn, THR, NMS_THR, case["max_per_img"])
    for a, b in zip(mc, (out[0], out[1], out[8], out[3])):
        assert torch.equal(a, b)
    return out, st, d


@pytest.mark.parametrize("name", sorted(DET_CASES))
def test_anchor_head_detections(T, name):
    out, st, d = run_det(T, name)
    levels = DET_CASES[name][0]
    if levels is not ONE:
        assert sum(st["suppressed"]) >= 1 and (out[3] > 0).all(), (st, out[3])
    k, off, Ktot = DD.plan(det_inputs(name)["sizes"], DET_CASES[name][6])
    assert out[4].shape[0] == DET_CASES[name][3] * Ktot


def test_anchors_as_one_tensor_and_shared_level_list(T):
    case = det_inputs("c5_b3_f32_nchw_pre100")
    a = [t.cuda() for t in case["cls"]], [t.cuda() for t in case["reg"]]
    kw = dict(nms_pre=100, target_means=K.MEANS, target_stds=K.STDS)
    one = T.anchor_head_detections(*a, _cuda(np.concatenate(case["anchors"])), _cuda(case["shapes"]), **kw)
    per = T.anchor_head_detections(*a, [_cuda(x) for x in case["anchors"]], _cuda(case["shapes"]), **kw)
    for x, y in zip(one, per):
        assert torch.equal(x, y)


@pytest.mark.parametrize("extra", [0, 1])
def test_more_than_4096_candidates_empty_one_image_only(T, extra):
    levels, cls, reg = K.overflow_case(extra)
    case = dict(cls=cls, reg=reg, anchors=K.pyramid(levels), shapes=K.img_shapes(2, levels), scale=None, nms_pre=4096,
                max_per_img=100, A=9, C=2, B=2, sizes=[9216, 864])
    out, st, d = run_det(T, "overflow+%d" % extra, case)
    cand = (d["scores"][d["batch_idx"] == 0, 1] > f32(THR)).sum()
    assert cand == 4096 + extra and not (d["scores"][d["batch_idx"] == 0, 2] > f32(THR)).any()
    counts = out[3].tolist()
    assert counts[1] > 0 and st["total"][1] > 0
    if extra:
        assert counts[0] == -1
        assert not out[0][0].any() and (out[1][0] == -1).all() and (out[2][0] == -1).all()
    else:
        assert counts[0] == min(100, st["total"][0]) and counts[0] > 0


# ---- targets -----------------------------------------------------------------------------------------------------------
TARGET_CASES = {
    # name: (seed, gt_counts, valid, allowed_border, gt_max_assign_all, labels)
    "novalid_border0_all_labels": (0, (4, 2), None, 0, True, True),
    "shared_valid_noborder_first_nolabels": (0, (4, 2), "shared", -1, False, False),
    "valid_border0_first_labels": (0, (4, 2), "per_image", 0, False, True),
    "valid_noborder_all_labels_empty_image": (0, (4, 0), "per_image", -1, True, True),
    "novalid_border0_all_nolabels_three": (0, (4, 2, 0), None, 0, True, False),
}
TMEANS, TSTDS = (0.0, 0.1, 0.0, -0.1), (0.1, 0.1, 0.2, 0.2)


def target_inputs(name):
    seed, counts, valid, border, all_, with_labels = TARGET_CASES[name]
    c = K.target_case(seed, counts)
    v = {None: None, "shared": c["valid"][0], "per_image": c["valid"]}[valid]
    return dict(anchors=c["anchors"], valid_flags=v, gt_bboxes=c["gt_bboxes"],
                gt_labels=c["gt_labels"] if with_labels else None, gt_counts=c["gt_counts"],
                img_shapes=c["img_shapes"]), dict(pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0.0,
                                                  allowed_border=border, gt_max_assign_all=all_,
                                                  target_means=TMEANS, target_stds=TSTDS)


def target_oracle(case, kw):
    info = {}
    ref = DD.anchor_target_all(info=info, **case, **kw)
    a = ref[6][0]                                        # the four-box image
    assert (a > 0).sum() > 0 and (a == 0).sum() > 0 and info["ignored"][0] > 0, info
    assert info["only_step6"][0] >= 1, info
    return ref, info


def run_targets(T, name):
    case, kw = target_inputs(name)
    ref, info = target_oracle(case, kw)
    dev = {k: _cuda(v) for k, v in case.items()}
    got = T.anchor_target_all(**dev, **kw)
    again = T.anchor_target_all(**dev, **kw)
    torch.cuda.synchronize()
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    g = [t.cpu().numpy() for t in got]
    names = ("labels", "label_weights", "bbox_targets", "bbox_weights", "num_pos", "num_neg", "assigned")
    for k in (6, 4, 5, 0, 1, 3):
        assert g[k].dtype == ref[k].dtype and g[k].shape == ref[k].shape, names[k]
        assert np.array_equal(TG._bits(g[k]), TG._bits(ref[k])), "%s: %d differ" % (names[k], (g[k] != ref[k]).sum())
    bi, ii = np.nonzero(ref[6] > 0)
    bx = case["anchors"][ii]
    gt = case["gt_bboxes"][bi, ref[6][bi, ii] - 1]
    TG._compare_targets(g[2], ref[2], None, None, ((bi, ii), bx, gt), TMEANS, TSTDS, name)
    assert np.all(g[2][ref[6] <= 0] == 0)
    return got, ref, info


@pytest.mark.parametrize("name", sorted(TARGET_CASES))
def test_anchor_target_all(T, name):
    got, ref, info = run_targets(T, name)
    counts = TARGET_CASES[name][1]
    for b, n in enumerate(counts):
        if n == 0:                                       # no ground truth: every participating anchor is negative
            assert ref[4][b] == 0 and ref[5][b] == ref[0].shape[1] - info["outside"][b] and ref[5][b] > 0
    if TARGET_CASES[name][5]:
        assert len(set(ref[0][0][ref[0][0] > 0].tolist())) >= 2, "positives of more than one class"


def test_targets_feed_the_focal_loss(T):
    """anchor_target_all -> anchor_head_loss(gamma = 2, avg_factor = num_pos) against loss_ref on the same targets, under
    test_gpu_losses' comparison; its backward runs (run_dense takes the gradients twice)."""
    case, kw = target_inputs("novalid_border0_all_labels")
    C = 5
    tg = T.anchor_target_all(**{k: _cuda(v) for k, v in case.items()}, **kw)
    labels, lw, bt, bw, num_pos = tg[:5]
    assert int(num_pos.sum()) > 0
    cls, reg = K.head_case(K.LEVELS, 2, 9, C, torch.bfloat16, "mixed", 77)
    cls, reg = [t.cuda() for t in cls], [t.cuda() for t in reg]
    TL.run_dense(T, cls, reg, labels.cpu().numpy(), lw.cpu().numpy(), bt.cpu().numpy(), bw.cpu().numpy(), num_pos,
                 num_pos.cpu().numpy(), C, 1.0 / 9.0, 2.0, 0.25, (1.5, 0.75), "targets -> focal loss",
                 targets_gpu=[labels, lw, bt, bw])


# ---- graph capture -------------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(T):
    """Both functions captured once and replayed on new inputs: a host synchronisation or an allocation inside the
    library would break the capture.  Eager and replayed results agree bit for bit, and two replays differ."""
    anchors = [_cuda(a) for a in K.pyramid(K.LEVELS)]
    all_anchors = torch.cat(anchors)

    def new(seed):
        cls, reg = K.head_case(K.LEVELS, 2, 9, 5, torch.bfloat16, "mixed", seed)
        t = K.target_case(seed)
        sh = torch.tensor([(64 - seed, 96), (60, 96 - 2 * seed)], dtype=torch.int32)
        return cls + reg + [sh, torch.from_numpy(t["gt_bboxes"]), torch.from_numpy(t["gt_labels"]),
                            torch.from_numpy(t["gt_counts"])]
    bufs = [t.cuda() for t in new(1)]

    def step():
        a = T.anchor_head_detections(bufs[0:3], bufs[3:6], anchors, bufs[6], 1.5, nms_pre=100, max_per_img=30,
                                     target_means=K.MEANS, target_stds=K.STDS, return_dense=True)
        t = T.anchor_target_all(all_anchors, None, bufs[7], bufs[8], bufs[9], bufs[6], allowed_border=0)
        return list(a) + list(t)

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
                assert dst.stride() == src.stride()
                dst.copy_(src)
        graph.replay()
        eager = step()
        again = step()
        torch.cuda.synchronize()
        for a, b, c in zip(captured, eager, again):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            assert torch.equal(b.view(torch.uint8), c.view(torch.uint8))
        seen.append([captured[0].clone(), captured[9].clone(), captured[13].clone()])
    for x, y in zip(*seen):
        assert not torch.equal(x, y)


# ---- under the guard -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import dense_detect_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, dense_detect_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


@pytest.mark.parametrize("name", ["c5_b3_f32_nchw_pre100", "c80_b3_bf16_nhwc_pre100_top20", "c5_b3_bf16_nhwc_pre50",
                                  "c1_b3_bf16_nchw_pre0", "big_c5_b1_bf16_nhwc_pre100", "one_c1_b1_bf16"])
def test_guarded_detections(T, guard, name):
    """Poisoned outputs and an exact-size workspace: every dense element and every unused row must have been WRITTEN."""
    run_det(T, name)
    _clean(guard, ["anchor_head_detections"])


def test_guarded_overflowing_image(T, guard):
    test_more_than_4096_candidates_empty_one_image_only(T, 1)
    _clean(guard, ["anchor_head_detections"])


@pytest.mark.parametrize("name", sorted(TARGET_CASES))
def test_guarded_targets(T, guard, name):
    run_targets(T, name)
    _clean(guard, ["anchor_target_all"])


def test_guarded_plan_matches_the_call(T, guard):
    case = det_inputs("c5_b3_f32_nchw_pre100")
    p = T.anchor_head_detections_plan([fs for fs, _ in K.LEVELS], 3, 9, 5, 100)
    assert p["launches"] == 7 and p["kept"] == [100, 100, 54] and p["K"] == 254 and p["selecting"] == 2
    assert T.anchor_head_detections_plan([fs for fs, _ in K.LEVELS], 3, 9, 5, 0)["launches"] == 6
    out = T.anchor_head_detections([t.cuda() for t in case["cls"]], [t.cuda() for t in case["reg"]],
                                   [_cuda(a) for a in case["anchors"]], _cuda(case["shapes"]), nms_pre=100,
                                   return_dense=True)
    assert out[4].shape[0] == p["rows"]
    _clean(guard, ["anchor_head_detections_plan"])


def test_every_entry_point_ran_under_the_guard_and_both_sides_ran():
    """Counts what the tests above did IN THIS RUN (run the file as a whole)."""
    from torch_detection_amd import dense_detect_ops
    public = sorted(n for n, v in vars(dense_detect_ops).items()
                    if inspect.isfunction(v) and v.__module__ == dense_detect_ops.__name__ and not n.startswith("_"))
    assert public == ["anchor_head_detections", "anchor_head_detections_plan", "anchor_target_all"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in ("anchor_head_detections", "anchor_target_all"):
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)
    assert SEEN["over"] >= 1 and SEEN["under"] >= 1 and SEEN["cut"] >= 1, SEEN
