"""GPU tests of Cascade R-CNN (refine_bboxes, cascade_detections, CascadeRoIHead) against the CPU oracle
tests/cascade_ref.py.  Every comparison is bitwise.

The one operation of the specification that NumPy and the device do not evaluate alike is ``expf`` (proposal_ref rounds a
float64 exp; §4b bounds the device's fp32 expf against it, tests/test_gpu_proposals.py).  So, as ``rpn_proposals``' tests
do, the oracle takes that part from the library's own, separately tested ops: refine_bboxes is compared with
``cascade_ref.refine_bboxes(decode=T.delta2bbox)`` on every row, and with the pure NumPy oracle on the rows whose log-size
deltas are 0 (exp(0) is exact) and on every count; cascade_detections is compared with the oracle's selection on the
GPU's own dense scores and boxes, and with the library's ``bbox_head_detections`` fed the ORACLE's averaged logits (all
six outputs), which pins the averaging, the softmax and the decode at once.

refine_bboxes takes one row per thread, the compacted mode in chunks of 1024 rows (one workgroup each), the row-aligned
mode in workgroups of 256: R covers 0, 1, one wavefront -1 / +0 / +1, exactly one chunk, one chunk + 1 (five row-aligned
workgroups) and three chunks.
"""
import inspect

import numpy as np
import pytest
import torch

import cascade_cases as K
import cascade_ref as CR
import guard_util as G

pytestmark = pytest.mark.gpu
f32 = np.float32
ENTERED, WS_SEEN = set(), {}
R_GRID = [0, 1, 63, 64, 65, 1024, 1025, 2100]


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _cuda(a):
    if a is None:
        return None
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def _np(t):
    return t.cpu().numpy()


def same(got, ref, what):
    got = _np(got) if torch.is_tensor(got) else got
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    g, r = (got.view(np.uint32), ref.view(np.uint32)) if got.dtype == f32 else (got, ref)
    assert np.array_equal(g, r), "%s differs at %s" % (what, np.argwhere(g != r)[:4].tolist())


def gpu_decode(T, stds):
    def decode(r, d, shape):
        return _np(T.delta2bbox(_cuda(r), _cuda(d), K.MEANS, stds, shape))
    return decode


def run_refine(T, c, stds, P, use_cls, drop_gt=True):
    """Both modes of one case against the oracle -> (rois_out, proposals, counts) of the GPU."""
    B = len(c["shapes"])
    ish = torch.tensor(c["shapes"], dtype=torch.int32).cuda()
    kw = dict(target_means=K.MEANS, target_stds=stds)
    lab = dict(cls_score=_cuda(c["cls"])) if use_cls else dict(labels=_cuda(c["labels"]))
    rlab = dict(cls_score=K.widen(c["cls"])) if use_cls else dict(labels=c["labels"])
    gt = dict(pos_assigned_gt_inds=_cuda(c["gt_inds"]), gt_bboxes=_cuda(c["gt"])) if drop_gt else {}
    rgt = dict(pos_assigned_gt_inds=c["gt_inds"], gt_bboxes=c["gt"]) if drop_gt else {}
    rois, reg = _cuda(c["rois"]), _cuda(c["reg"])
    out = T.refine_bboxes(rois, reg, ish, **lab, **kw)
    props, counts = T.refine_bboxes(rois, reg, ish, max_per_img=P, **lab, **gt, **kw)
    regw = K.widen(c["reg"])
    dec = gpu_decode(T, stds)
    what = "R%d B%d %s" % (c["rois"].shape[0], B, "argmax" if use_cls else "labels")
    same(out, CR.refine_bboxes(c["rois"], regw, c["shapes"], decode=dec, **rlab, **kw), what + " row-aligned")
    rp, rc = CR.refine_bboxes(c["rois"], regw, c["shapes"], max_per_img=P, decode=dec, **rlab, **rgt, **kw)
    same(counts, rc, what + " counts")
    same(props, rp, what + " proposals")
    # the pure NumPy oracle: counts, the batch column, and the boxes of the exp-free rows
    pure = CR.refine_bboxes(c["rois"], regw, c["shapes"], **rlab, **kw)
    same(counts, CR.refine_bboxes(c["rois"], regw, c["shapes"], max_per_img=P, **rlab, **rgt, **kw)[1], what + " pure counts")
    o = _np(out)
    same(o[:, 0], pure[:, 0], what + " pure image column")
    same(o[::3], pure[::3], what + " pure exp-free rows")
    return o, _np(props), _np(counts)


@pytest.mark.parametrize("dt", sorted(K.DTYPES))
@pytest.mark.parametrize("R", R_GRID)
def test_refine_bboxes_bit_exact(T, R, dt):
    seed = 0
    seen_trunc = seen_under = 0
    for B in (1, 3):
        for C, agnostic in ((1, True), (2, False), (2, True), (81, False), (81, True)):
            for use_cls in (False, True):
                seed += 1
                c = K.refine_case(R, B, C, agnostic, dt, 1000 * R + seed)
                P = max(1, R // (2 * B)) if seed % 2 else max(1, R)
                stds = K.STDS if seed % 3 else (0.05, 0.05, 0.1, 0.1)
                o, props, counts = run_refine(T, c, stds, P, use_cls)
                seen_trunc += int((counts == P).any())
                seen_under += int((counts < P).any())
                if R >= 1024 and C == 81:
                    # not hollow: both clips, the ratio clip, ties and ground truths are all in the case
                    w = np.asarray([s[1] for s in c["shapes"]], f32)[np.maximum(c["img"], 0)] - 1
                    v = o[:, 0] >= 0
                    assert (o[v, 1] == 0).any() and (o[v, 3] == w[v]).any()
                    x = K.widen(c["cls"])
                    assert ((x == x.max(1, keepdims=True)).sum(1) > 1).mean() > 0.5
                    assert c["is_gt"].sum() > 50 and (c["gt_inds"][~c["is_gt"]] >= 0).sum() > 50
    if R >= 63:
        assert seen_trunc and seen_under


def test_refine_edge_images(T):
    """Image 1 has no rows at all, image 2 only ground truths, and a third run has nothing but padding."""
    c = K.refine_case(1500, 3, 5, False, "bf16", 77, only_images=[0, 2])
    two = c["img"] == 2
    g = np.random.default_rng(3).integers(0, K.G, two.sum()).astype(np.int32)
    c["rois"][two, 1:] = c["gt"][2, g]
    c["gt_inds"][two] = g
    o, props, counts = run_refine(T, c, K.STDS, 2000, False)
    assert counts[0] > 300 and counts[1:].tolist() == [0, 0] and not props[1:].any()
    o, props, counts = run_refine(T, c, K.STDS, 64, True)
    assert counts.tolist() == [64, 0, 0]
    c = K.refine_case(1100, 2, 3, False, "f32", 78, pad=1.1)
    c["rois"][1:3, 0] = -1
    o, props, counts = run_refine(T, c, K.STDS, 7, True)
    assert counts.tolist() == [0, 0] and not props.any() and (o[:, 0] == -1).all() and not o[:, 1:].any()


def test_refine_drops_a_proposal_that_equals_its_ground_truth_bitwise(T):
    """The documented deviation from pos_is_gt: the test is on the coordinates, so such a proposal goes too; the same
    coordinates under another index, or one ulp away, stay."""
    gt = np.asarray([[[10, 10, 50, 50], [60, 20, 90, 80]]], f32)
    near = np.nextafter(f32(50), f32(60))
    rois = np.asarray([[0, 10, 10, 50, 50], [0, 10, 10, 50, 50], [0, 10, 10, 50, near], [0, 10, 10, 50, 50],
                       [0, 60, 20, 90, 80], [0, 1, 2, 30, 40]], f32)
    gi = np.asarray([0, 1, 0, -1, 1, 0], np.int32)
    ish = torch.tensor([[100, 200]], dtype=torch.int32).cuda()
    reg = torch.zeros(6, 4).cuda()
    lab = torch.zeros(6, dtype=torch.int64).cuda()
    props, counts = T.refine_bboxes(_cuda(rois), reg, ish, labels=lab, pos_assigned_gt_inds=_cuda(gi),
                                    gt_bboxes=_cuda(gt), max_per_img=6)
    rp, rc = CR.refine_bboxes(rois, np.zeros((6, 4), f32), [(100, 200)], labels=np.zeros(6, np.int64),
                              pos_assigned_gt_inds=gi, gt_bboxes=gt, max_per_img=6)
    same(counts, rc, "counts")
    same(props, rp, "proposals")
    assert rc.tolist() == [4] and rp[0, :4, :4].tolist() == [rois[1, 1:].tolist(), rois[2, 1:].tolist(),
                                                            rois[3, 1:].tolist(), rois[5, 1:].tolist()]
    # without the pair nothing but padding is dropped
    props, counts = T.refine_bboxes(_cuda(rois), reg, ish, labels=lab, max_per_img=6)
    assert counts.tolist() == [6]


# ---- cascade_detections ----------------------------------------------------------------------------------------------
def run_detect(T, R, B, C, S, agnostic, dt, seed, scale):
    rois, logits, reg, shapes = K.detect_case(R, B, C, S, agnostic, dt, seed)
    ish = torch.tensor(shapes, dtype=torch.int32).cuda()
    kw = dict(score_thr=0.05, nms_thr=0.5, max_per_img=20, target_means=K.MEANS, target_stds=K.STDS)
    r, x, d = _cuda(rois), [_cuda(v) for v in logits], _cuda(reg)
    out = T.cascade_detections(r, x, d, ish, scale, return_dense=True, **kw)
    assert len(out) == 6
    what = "R%d B%d C%d S%d %s" % (R, B, C, S, dt)
    # 1. the oracle's selection on the GPU's own dense scores and boxes
    st = {}
    ref = CR.cascade_select(rois, _np(out[4]), _np(out[5]), B, 0.05, 0.5, 20, st)
    for name, g, e in zip(("dets", "labels", "row_idx", "counts"), out, ref):
        same(g, e, what + " " + name)
    # 2. the library's bbox_head_detections on the ORACLE's averaged logits (fp32; the deltas widened exactly)
    avg = CR.average_logits([K.widen(v) for v in logits])
    lib = T.bbox_head_detections(r, _cuda(avg), d.float(), ish, scale, return_dense=True, **kw)
    for name, g, e in zip(("dets", "labels", "row_idx", "counts", "scores", "boxes"), out, lib):
        same(g, _np(e), what + " vs bbox_head_detections(mean) " + name)
    # 3. one stage: bbox_head_detections itself, in the stored dtype
    if S == 1:
        lib = T.bbox_head_detections(r, x[0], d, ish, scale, return_dense=True, **kw)
        for name, g, e in zip(("dets", "labels", "row_idx", "counts", "scores", "boxes"), out, lib):
            same(g, _np(e), what + " vs bbox_head_detections " + name)
    plain = T.cascade_detections(r, x, d, ish, scale, **kw)
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, out))
    return out, st


@pytest.mark.parametrize("dt", sorted(K.DTYPES))
@pytest.mark.parametrize("C", [2, 81])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_cascade_detections_bit_exact(T, S, C, dt):
    i = S + C + len(dt)
    for n, R in enumerate((1, 65, 1031)):
        scale = (None, 1.25, torch.tensor([0.8, 1.6, 1.1][:1 + 2 * (n % 2)]).cuda())[(i + n) % 3]
        B = 1 + 2 * (n % 2)
        if torch.is_tensor(scale) and scale.shape[0] != B:
            scale = 1.5
        out, st = run_detect(T, R, B, C, S, bool((i + n) % 2), dt, 50 * i + n, scale)
        if R == 1031:
            assert sum(st["suppressed"]) > 0 and (out[3] > 0).all()


def test_cascade_detections_no_rows(T):
    ish = torch.tensor(K.SHAPES[:2], dtype=torch.int32).cuda()
    z = lambda c: torch.zeros(0, c, device="cuda")
    out = T.cascade_detections(z(5), [z(5), z(5)], z(20), ish, max_per_img=4, return_dense=True)
    assert out[3].tolist() == [0, 0] and not out[0].any() and (out[1] == -1).all() and out[4].shape == (0, 5)
    props, counts = T.refine_bboxes(z(5), z(20), ish, cls_score=z(5), max_per_img=3)
    assert counts.tolist() == [0, 0] and props.shape == (2, 3, 5) and not props.any()
    assert T.refine_bboxes(z(5), z(20), ish, cls_score=z(5)).shape == (0, 5)


# ---- graph capture ---------------------------------------------------------------------------------------------------
def test_graph_capture_and_replay(T):
    """Row-aligned refine -> cascade_detections, and the compacted refine, captured on one stream and replayed twice on
    new inputs: a host synchronisation or an allocation inside the library would break the capture.  Eager and replayed
    bits are identical."""
    def new(seed):
        c = K.refine_case(1300, 2, 21, False, "bf16", seed)
        _, logits, _, _ = K.detect_case(1300, 2, 21, 2, False, "bf16", seed)
        sh = torch.tensor([(600 - seed, 900), (480, 1000 - 3 * seed)], dtype=torch.int32)
        return [torch.from_numpy(c["rois"]), c["reg"], logits[0], logits[1], sh, torch.from_numpy(c["gt_inds"]),
                torch.from_numpy(c["gt"][:2]), torch.from_numpy(c["labels"])]
    bufs = [t.cuda() for t in new(1)]

    def step():
        rois, reg, x0, x1, sh, gi, gt, lab = bufs
        r1 = T.refine_bboxes(rois, reg, sh, cls_score=x0)
        det = T.cascade_detections(r1, [x0, x1], reg, sh, 1.5, max_per_img=30, return_dense=True)
        tr = T.refine_bboxes(rois, reg, sh, labels=lab, pos_assigned_gt_inds=gi, gt_bboxes=gt, max_per_img=400)
        return [r1] + list(det) + list(tr)

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
        for a, b in zip(captured, eager):
            same(a, _np(b), "replay %d" % seed)
        seen.append([captured[0].clone(), captured[1].clone(), captured[7].clone()])
    assert all(not torch.equal(a, b) for a, b in zip(*seen))


# ---- under the guard -------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import cascade_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, cascade_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


@pytest.mark.parametrize("dt", sorted(K.DTYPES))
def test_guarded_refine_bboxes(T, guard, dt):
    """Poisoned outputs: every row of both forms must have been WRITTEN, the zeros past the counts too."""
    for R, B, C, agnostic, P in ((2100, 3, 81, False, 100), (1025, 1, 2, True, 2000), (65, 3, 1, True, 8192), (1, 1, 81, False, 1)):
        for use_cls in (False, True):
            run_refine(T, K.refine_case(R, B, C, agnostic, dt, 400 + R), K.STDS, P, use_cls)
            _clean(guard, ["refine_bboxes"])


@pytest.mark.parametrize("dt", sorted(K.DTYPES))
def test_guarded_cascade_detections(T, guard, dt):
    for R, B, C, S in ((1031, 3, 81, 3), (7, 1, 2, 8), (65, 3, 81, 1)):
        run_detect(T, R, B, C, S, C == 2, dt, 500 + R, None)
        _clean(guard, ["cascade_detections"])


def test_guarded_no_rows(T, guard):
    test_cascade_detections_no_rows(T)
    _clean(guard, [])


def test_every_cascade_entry_point_ran_under_the_guard():
    """Counts what the tests above did IN THIS RUN (run the file as a whole)."""
    from torch_detection_amd import cascade_ops
    public = sorted(n for n, v in vars(cascade_ops).items()
                    if inspect.isfunction(v) and v.__module__ == cascade_ops.__name__ and not n.startswith("_"))
    assert public == ["cascade_detections", "refine_bboxes", "refine_ws_bytes"]
    assert {"cascade_detections", "refine_bboxes"} <= ENTERED, ENTERED
    for op in ("cascade_detections", "refine_bboxes"):
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)


# ---- the module ------------------------------------------------------------------------------------------------------
IMG = (64, 96)
LEVELS = (((16, 24), 4), ((8, 12), 8), ((4, 6), 16))


def _head(T, n, seed):
    torch.manual_seed(seed)
    ext = dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", out_size=7, sample_num=2), out_channels=64,
               featmap_strides=[s for _, s in LEVELS], finest_scale=16)
    bb = dict(type="BBoxHead", num_fcs=2, in_channels=64, fc_out_channels=64, roi_feat_size=7, num_classes=5)
    cfg = [dict(pos_iou_thr=t, neg_iou_thr=t, min_pos_iou=t, num=64, pos_fraction=0.25, add_gt_as_proposals=True)
           for t in (0.5, 0.6, 0.7)[:n]]
    head = T.CascadeRoIHead(num_stages=n, stage_loss_weights=(1, 0.5, 0.25)[:n], bbox_roi_extractor=ext, bbox_head=bb,
                            train_cfg=cfg).cuda()
    with torch.no_grad():                                   # predictors large enough to move boxes and split classes
        for h in head.bbox_head:
            for fc in list(h.shared_fcs) + [h.fc_cls, h.fc_reg]:
                fc.bias.normal_(0, 0.1)
            h.fc_cls.weight.mul_(10)
            h.fc_reg.weight.mul_(100)
    return head


def _scene(seed, P=100):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(2, 64, h, w, generator=g).cuda().bfloat16().contiguous(memory_format=torch.channels_last)
             for (h, w), _ in LEVELS]
    gxy = torch.rand(2, 4, 2, generator=g) * torch.tensor([50.0, 30.0])
    gt = torch.cat([gxy, gxy + torch.rand(2, 4, 2, generator=g) * 30 + 10], -1).contiguous()
    gt_counts = torch.tensor([4, 3], dtype=torch.int32)
    gt[1, 3] = 0
    gt_labels = torch.randint(1, 5, (2, 4), generator=g)
    # proposals: jittered ground truths (positives at every threshold) and random boxes
    j = gt[:, torch.arange(P) % 4] + torch.randn(2, P, 4, generator=g) * torch.linspace(0.5, 6, P).view(1, P, 1)
    xy = torch.rand(2, P, 2, generator=g) * torch.tensor([60.0, 40.0])
    rnd = torch.cat([xy, xy + torch.rand(2, P, 2, generator=g) * 30 + 4], -1)
    box = torch.where((torch.arange(P) % 2 == 0).view(1, P, 1), j, rnd)
    props = torch.cat([box, torch.rand(2, P, 1, generator=g)], -1).contiguous()
    counts = torch.tensor([P, P - 17], dtype=torch.int32)
    ish = torch.tensor([IMG, IMG], dtype=torch.int32)
    return feats, props.cuda(), counts.cuda(), gt.cuda(), gt_labels.cuda(), gt_counts.cuda(), ish.cuda()


def _composed_train(T, head, feats, props, counts, gt, gt_labels, gt_counts, ish, seed):
    losses, n = {}, head.num_stages
    stds = [(0.1, 0.1, 0.2, 0.2), (0.05, 0.05, 0.1, 0.1), (0.033, 0.033, 0.067, 0.067)]
    weights, thr = (1, 0.5, 0.25), (0.5, 0.6, 0.7)
    kept = []
    for i in range(n):
        rois, labels, lw, bt, bw, gi, npos, nneg = T.sample_rois(props, counts, gt, gt_labels, gt_counts, thr[i], thr[i],
                                                             thr[i], num=64, pos_fraction=0.25,
                                                             add_gt_as_proposals=True, target_stds=stds[i], seed=seed + i)
        x = T.roi_align(feats, rois, 7, [s for _, s in LEVELS], 2, 16)
        cls, reg = head.bbox_head[i](x)
        l = T.bbox_head_loss(cls, reg, labels, lw, bt, bw)
        losses["s%d.loss_cls" % i], losses["s%d.loss_bbox" % i] = l[0] * weights[i], l[1] * weights[i]
        kept.append((npos, nneg, counts))
        if i < n - 1:
            props, counts = T.refine_bboxes(rois, reg, ish, labels=labels, pos_assigned_gt_inds=gi, gt_bboxes=gt,
                                            max_per_img=64, target_stds=stds[i])
    return losses, kept


@pytest.mark.parametrize("n", [2, 3])
def test_cascade_roi_head_is_the_composition(T, n):
    head = _head(T, n, seed=n)
    scene = _scene(10 + n)
    losses = head.forward_train(*scene, seed=5)
    assert sorted(losses) == sorted("s%d.loss_%s" % (i, k) for i in range(n) for k in ("cls", "bbox"))
    sum(losses.values()).backward()
    grads = [p.grad.clone() for p in head.parameters()]
    head.zero_grad(set_to_none=True)
    ref, kept = _composed_train(T, head, *scene, seed=5)
    sum(ref.values()).backward()
    for k in ref:
        same(losses[k].detach(), _np(ref[k].detach()), k)
        assert float(ref[k].detach()) > 0
    params = dict(head.named_parameters())
    assert len(params) == 8 * n
    for (name, p), g in zip(params.items(), grads):
        same(g, _np(p.grad), name + ".grad")
        assert p.grad.abs().max() > 0, name
    # not hollow: every stage had positives, and a stage's proposals are the sampled rows of the one before it at most
    for i, (npos, nneg, cnt) in enumerate(kept):
        assert (npos > 0).all() and (cnt > 0).all()
        if i:
            assert (cnt <= kept[i - 1][0] + kept[i - 1][1]).all()
    # test time
    feats, props, counts, _, _, _, ish = scene
    out = head.simple_test(feats, props, counts, ish, scale_factors=1.25, score_thr=0.02, max_per_img=15)
    with torch.no_grad():
        rois = T.rois_from_proposals(props, counts)
        scores = []
        for i in range(n):
            cls, reg = head.bbox_head[i](T.roi_align(feats, rois, 7, [s for _, s in LEVELS], 2, 16))
            scores.append(cls)
            if i < n - 1:
                rois = T.refine_bboxes(rois, reg, ish, cls_score=cls, target_stds=head.target_stds[i])
        ref = T.cascade_detections(rois, scores, reg, ish, 1.25, 0.02, 0.5, 15, target_stds=head.target_stds[n - 1])
    assert len(out) == 4 and (out[3] > 0).all()
    for name, a, b in zip(("dets", "labels", "row_idx", "counts"), out, ref):
        same(a, _np(b), "simple_test " + name)


def test_cascade_roi_head_refuses_mask_stages_in_the_call(T):
    head = T.CascadeRoIHead(bbox_head=dict(num_fcs=1, in_channels=64, fc_out_channels=64, num_classes=5),
                            mask_roi_extractor=dict(type="SingleRoIExtractor"), mask_head=dict(type="FCNMaskHead"))
    scene = _scene(3)
    with pytest.raises(NotImplementedError, match="mask stages"):
        head.forward_train(*scene)
    with pytest.raises(NotImplementedError, match="mask stages"):
        head.simple_test(scene[0], scene[1], scene[2], scene[6])
