"""GPU tests of box-delta encode / decode, batched NMS and the fused RPN proposal pipeline against the CPU oracle
(tests/proposal_ref.py)."""
import numpy as np
import pytest
import torch

import proposal_ref as R

pytestmark = pytest.mark.gpu

LEVELS = [((200, 336), 4), ((100, 168), 8), ((50, 84), 16), ((25, 42), 32), ((13, 21), 64)]
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def rand_boxes(n, seed, lo=4.0, hi=300.0, canvas=(800, 1344)):
    g = np.random.default_rng(seed)
    wh = g.uniform(lo, hi, (n, 2)).astype(np.float32)
    x1 = g.uniform(0, canvas[1] - hi, n).astype(np.float32)
    y1 = g.uniform(0, canvas[0] - hi, n).astype(np.float32)
    return np.stack([x1, y1, x1 + wh[:, 0], y1 + wh[:, 1]], -1).astype(np.float32)


def test_bbox2delta_vs_oracle(T):
    p, gt = rand_boxes(5000, 1), rand_boxes(5000, 2)
    means, stds = (0.1, -0.2, 0.05, 0.0), (0.1, 0.1, 0.2, 0.2)
    got = T.bbox2delta(torch.from_numpy(p).cuda(), torch.from_numpy(gt).cuda(), means, stds).cpu().numpy()
    ref = R.bbox2delta(p, gt, means, stds)
    assert np.array_equal(got[:, :2].view(np.uint32), ref[:, :2].view(np.uint32))     # dx / dy: bit-exact
    raw = R.bbox2delta(p, gt)                                                          # un-normalised log path
    tol = 4 * np.spacing(np.abs(raw[:, 2:])) / np.float32(stds[2]) + np.spacing(np.abs(ref[:, 2:]))
    assert np.all(np.abs(got[:, 2:] - ref[:, 2:]) <= tol)
    same = T.bbox2delta(torch.from_numpy(p).cuda(), torch.from_numpy(p).cuda()).cpu().numpy()
    assert np.array_equal(same, np.zeros_like(same))


def test_delta2bbox_vs_oracle(T):
    n, C = 4000, 3
    rois = rand_boxes(n, 3)
    g = np.random.default_rng(4)
    d = g.normal(0, 1.0, (n, 4 * C)).astype(np.float32)
    d[::7, 2::4] = g.choice([-9.0, 9.0, 4.2, -4.2], (len(d[::7]), C))                 # beyond the clamp
    means, stds = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)
    for shape in (None, (700, 1100)):
        got = T.delta2bbox(torch.from_numpy(rois).cuda(), torch.from_numpy(d).cuda(), means, stds, shape).cpu().numpy()
        ref = R.delta2bbox(rois, d, means, stds, shape)
        dd = d.reshape(n, C, 4).astype(np.float64) * np.asarray(stds)
        tol = np.empty((n, C, 4), np.float32)
        for ax in (0, 1):                                   # x: max(|gx|, gw, 1), y: max(|gy|, gh, 1)
            pw = ((rois[:, 2 + ax] - rois[:, ax]) + 1)[:, None].astype(np.float64)
            gw = pw * np.exp(np.clip(dd[..., 2 + ax], -4.1351666, 4.1351666))
            gx = np.abs((rois[:, ax] + rois[:, 2 + ax])[:, None] * 0.5 + pw * dd[..., ax])
            t = 4 * np.spacing(np.maximum(np.maximum(gx, gw), 1.0).astype(np.float32))
            tol[..., ax], tol[..., 2 + ax] = t, t
        tol = tol.reshape(n, 4 * C)
        assert np.all(np.abs(got - ref) <= tol), np.abs(got - ref).max()
    # the exp-free path (dw = dh = 0) is bit-exact, and zero deltas give integer anchors back
    d0 = d.copy()
    d0[:, 2::4] = 0
    d0[:, 3::4] = 0
    got = T.delta2bbox(torch.from_numpy(rois).cuda(), torch.from_numpy(d0).cuda(), means, stds).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.delta2bbox(rois, d0, means, stds).view(np.uint32))
    ia = np.floor(rois)
    got = T.delta2bbox(torch.from_numpy(ia).cuda(), torch.zeros(n, 4, device="cuda")).cpu().numpy()
    assert np.array_equal(got, ia)


def _segments(sizes, seed):
    boxes = np.concatenate([rand_boxes(s, seed + i, 8, 120, (300, 400)) for i, s in enumerate(sizes)]) \
        if sum(sizes) else np.zeros((0, 4), np.float32)
    g = np.random.default_rng(seed)
    scores = g.choice(np.linspace(0, 1, 50).astype(np.float32), boxes.shape[0])      # plenty of ties
    return boxes.astype(np.float32), scores.astype(np.float32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("sizes", [[1500], [0, 1, 700], [300, 0, 1, 2, 2000, 64, 65, 129, 4096, 17]])
def test_batched_nms_vs_oracle(T, sizes):
    boxes, scores, off = _segments(sizes, len(sizes))
    kref, kiref, cref = R.batched_nms(boxes, scores, off, 0.5)
    for seg in (torch.from_numpy(off).cuda(), torch.from_numpy(off)):
        keep, kept, counts = T.batched_nms(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), seg, 0.5)
        assert np.array_equal(counts.cpu().numpy(), cref)
        assert np.array_equal(keep.cpu().numpy(), kref)
        assert np.array_equal(kept.cpu().numpy(), kiref)


def test_batched_nms_no_host_sync(T):
    """Captured in a graph (a host synchronisation would break the capture), replayed on new scores."""
    boxes, scores, off = _segments([400, 0, 900], 7)
    b, s, o = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(off).cuda()
    T.batched_nms(b, s, o, 0.6)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = T.batched_nms(b, s, o, 0.6)
    s.copy_(torch.from_numpy(scores[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    kref, kiref, cref = R.batched_nms(boxes, scores[::-1].copy(), off, 0.6)
    assert np.array_equal(outs[2].cpu().numpy(), cref)
    assert np.array_equal(outs[1].cpu().numpy(), kiref) and np.array_equal(outs[0].cpu().numpy(), kref)


def _pyramid(T, levels):
    gens = [T.AnchorGenerator(st, [8], [0.5, 1.0, 2.0]) for _, st in levels]
    anchors, _ = T.anchor_pyramid(gens, [fs for fs, _ in levels], [st for _, st in levels], "cuda")
    return anchors


def _head_outputs(B, levels, seed, dtype, channels_last, mode):
    g = torch.Generator().manual_seed(seed)
    cls, reg = [], []
    for (h, w), _ in levels:
        if mode == "ties":
            vals = torch.tensor([-1.5, -0.25, 0.0, -0.0, 0.75])
            c = vals[torch.randint(0, 5, (B, 3, h, w), generator=g)]
        elif mode == "saturated":
            c = torch.randn(B, 3, h, w, generator=g) * 40
        else:
            c = torch.randn(B, 3, h, w, generator=g) * 2
        d = torch.randn(B, 12, h, w, generator=g) * 0.5
        if mode == "saturated":
            d[:, 2::4] *= 20                                 # dw, dh far beyond the clamp
            d[:, 3::4] *= 20
        c, d = c.to(dtype).cuda(), d.to(dtype).cuda()
        if channels_last:
            c, d = c.contiguous(memory_format=torch.channels_last), d.contiguous(memory_format=torch.channels_last)
        cls.append(c)
        reg.append(d)
    return cls, reg


def _check(T, cls, reg, anchors, shapes, **cfg):
    means, stds = cfg.get("target_means", MEANS), cfg.get("target_stds", STDS)
    ish = torch.tensor(shapes, dtype=torch.int32).cuda()
    props, aidx, counts = T.rpn_proposals(cls, reg, anchors, ish, **cfg)
    again = T.rpn_proposals(cls, reg, anchors, ish, **cfg)
    torch.cuda.synchronize()
    for a, b in zip((props, aidx, counts), again):                                       # run to run: bitwise
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)

    def gpu_decode(r, d, shape):
        return T.delta2bbox(torch.from_numpy(np.ascontiguousarray(r)).cuda(),
                            torch.from_numpy(np.ascontiguousarray(d)).cuda(), means, stds, shape).cpu().numpy()

    ref_cfg = {k: v for k, v in cfg.items()}
    pr, ar, cr = R.rpn_proposals([c.float().cpu().numpy() for c in cls], [d.float().cpu().numpy() for d in reg],
                                 [a.cpu().numpy() for a in anchors], shapes, decode=gpu_decode, **ref_cfg)
    p, a, c = props.cpu().numpy(), aidx.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(c, cr)
    assert np.array_equal(a, ar)
    assert np.array_equal(p[..., :4].view(np.uint32), pr[..., :4].view(np.uint32))
    assert np.all(np.abs(p[..., 4] - pr[..., 4]) <= 1e-6)
    for b in range(len(shapes)):
        assert np.all(p[b, c[b]:] == 0)
    return props, aidx, counts


@pytest.mark.parametrize("B,dtype,cl,min_size,mode,cfg", [
    (2, torch.float32, False, 0, "normal", dict(nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7)),
    (2, torch.bfloat16, True, 16, "normal", dict(nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7)),
    (1, torch.bfloat16, False, 0, "ties", dict(nms_pre=2000, nms_post=1500, max_num=3000, nms_thr=0.6)),
    (4, torch.float32, True, 16, "saturated", dict(nms_pre=4096, nms_post=300, max_num=1000, nms_thr=0.5,
                                                   target_means=(0.0, 0.1, 0.0, -0.1),
                                                   target_stds=(0.1, 0.1, 0.2, 0.2))),
])
def test_rpn_proposals_c4_vs_oracle(T, B, dtype, cl, min_size, mode, cfg):
    anchors = _pyramid(T, LEVELS)
    assert sum(a.shape[0] for a in anchors) == 268569
    cls, reg = _head_outputs(B, LEVELS, 11 + B, dtype, cl, mode)
    shapes = [(800, 1344), (600, 1000), (800, 1100), (512, 1344)][:B]
    _, _, counts = _check(T, cls, reg, anchors, shapes, min_bbox_size=min_size, **cfg)
    assert int(counts.min()) > 0


def test_rpn_proposals_small_levels_and_nms_pre_zero(T):
    """nms_pre = 0 (every anchor enters NMS) on levels of at most 4096 anchors; an empty level in the middle."""
    levels = [((20, 30), 8), ((0, 15), 16), ((5, 8), 32)]
    anchors = _pyramid(T, levels)
    cls, reg = _head_outputs(3, levels, 5, torch.float32, False, "normal")
    _check(T, cls, reg, anchors, [(160, 240), (100, 200), (37, 61)], nms_pre=0, nms_post=500, max_num=700,
           nms_thr=0.7, min_bbox_size=4)


def test_rpn_proposals_graph_replay(T):
    anchors = _pyramid(T, LEVELS)
    cls, reg = _head_outputs(2, LEVELS, 3, torch.bfloat16, True, "normal")
    ish = torch.tensor([(800, 1344), (700, 1200)], dtype=torch.int32).cuda()
    eager = T.rpn_proposals(cls, reg, anchors, ish)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed = T.rpn_proposals(cls, reg, anchors, ish)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)
    cls2, _ = _head_outputs(2, LEVELS, 4, torch.bfloat16, True, "normal")
    for c, c2 in zip(cls, cls2):
        c.copy_(c2)
    g.replay()
    eager2 = T.rpn_proposals(cls, reg, anchors, ish)
    torch.cuda.synchronize()
    for a, b in zip(eager2, graphed):
        assert torch.equal(a, b)
    assert not torch.equal(eager[1], eager2[1])


def test_rpn_proposals_errors(T):
    levels = [((10, 12), 8), ((5, 6), 16)]
    anchors = _pyramid(T, levels)
    cls, reg = _head_outputs(2, levels, 1, torch.float32, False, "normal")
    ish = torch.tensor([(80, 96), (80, 96)], dtype=torch.int32).cuda()
    bad = [
        (dict(cls_scores=cls * 5, bbox_preds=reg * 5, anchors=anchors * 5), "takes 1..8 levels"),      # 10 levels
        (dict(cls_scores=[c.half() for c in cls], bbox_preds=[d.half() for d in reg]),
         r"cls_scores\[0\] must be a float32 / bfloat16"),                                              # dtype
        (dict(bbox_preds=[reg[0][:, :8], reg[1]]), r"bbox_preds\[0\] must be a float32 \(2, 12, 10, 12\)"),  # 4A channels
        (dict(bbox_preds=[reg[0].bfloat16(), reg[1]]), r"bbox_preds\[0\] must be a float32 .* got bfloat16"),   # mixed dtypes
        (dict(anchors=[anchors[0][:-1], anchors[1]]), r"anchors\[0\] must be a contiguous float32 \(360, 4\)"),  # anchor rows
        (dict(img_shapes=ish[:1]), r"img_shapes must be a contiguous int32 \(2, 2\)"),
        (dict(img_shapes=ish.float()), r"img_shapes must be a contiguous int32 \(2, 2\)"),
        (dict(nms_pre=4097), "nms_pre must be in 0..4096"),
        (dict(nms_pre=-1), "nms_pre must be in 0..4096"),
        (dict(max_num=8193), "max_num must be in 1..8192"),
        (dict(max_num=0), "max_num must be in 1..8192"),
        (dict(nms_post=0), "nms_post must be >= 1"),
        (dict(min_bbox_size=-1), "min_bbox_size must be >= 0"),
        (dict(target_stds=(1, 1, 1)), "target_stds must have 4 finite entries"),
    ]
    for kw, msg in bad:
        args = dict(cls_scores=cls, bbox_preds=reg, anchors=anchors, img_shapes=ish)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.rpn_proposals(**args)
    big = [((70, 70), 8)]                                                                   # 14700 anchors
    a_big = _pyramid(T, big)
    c_big, r_big = _head_outputs(1, big, 2, torch.float32, False, "normal")
    with pytest.raises(ValueError, match="14700 anchors enter NMS with nms_pre=0"):
        T.rpn_proposals(c_big, r_big, a_big, [(560, 560)], nms_pre=0)
    c65 = [torch.zeros(65, 3, 2, 2, device="cuda")]
    with pytest.raises(ValueError, match="number of images must be in 1..64"):
        T.rpn_proposals(c65, [torch.zeros(65, 12, 2, 2, device="cuda")], [torch.zeros(12, 4, device="cuda")],
                        [(8, 8)] * 65)
    with pytest.raises(NotImplementedError):
        T.rpn_proposals(cls, reg, anchors, ish, use_sigmoid_cls=False)
    with pytest.raises(NotImplementedError):
        T.rpn_proposals(cls, reg, anchors, ish, nms_across_levels=True)
    with pytest.raises(ValueError, match="a segment holds more than 4096 boxes"):
        T.batched_nms(torch.zeros(5000, 4, device="cuda"), torch.zeros(5000, device="cuda"),
                      torch.tensor([0, 5000]), 0.5)
    torch.cuda.synchronize()
