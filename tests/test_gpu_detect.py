"""GPU tests of the test-time detections (multiclass_nms, bbox_head_detections) against the CPU oracle
tests/detect_ref.py: multiclass_nms bit for bit; the dense softmax within (16 + |z_c|)·u·p64 + 2^-149 of the float64
oracle, the dense boxes within §4b's decode tolerance, and the final outputs bit-equal to the oracle run on the GPU's
own dense scores and boxes; the chain from rpn_proposals; graph capture; both wrappers of detect_ops.py under the guard
of tests/guard_util.py.

Every multiclass_nms case asserts on the ORACLE's result that it is not hollow: candidates in at least min(2, C - 1)
classes (C = 2 has one foreground class), at least one box lost to NMS; over the file one case has more survivors than
max_num and one has fewer (the last test of the file counts what ran IN THIS RUN: run the file as a whole).
"""
import inspect

import numpy as np
import pytest
import torch

import detect_ref as D
import guard_util as G

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24
SEEN = {"over": 0, "under": 0}      # multiclass cases with total > max_num / total < max_num, this run
ENTERED, WS_SEEN = set(), {}        # what ran under the guard in this run
THR = 0.05
VALUES = np.concatenate([[THR], np.arange(1, 50) / 50.0]).astype(f32)     # 50 score values, score_thr among them


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, ref, what=""):
    for name, g, r in zip(("dets", "labels", "row_idx", "counts"), got, ref):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape)
        if g.dtype == np.float32:
            g, r = g.view(np.uint32), r.view(np.uint32)
        assert np.array_equal(g, r), "%s: %s differs at %s" % (what, name, np.argwhere(g != r)[:4].tolist())


# ---- multiclass_nms ---------------------------------------------------------------------------------------------------
def mc_case(seed, per_img, C, layout, agnostic, exact=None, p_low=0.5):
    """Clustered integer boxes, scores from VALUES (p_low of the mass at or below the threshold).  ``layout``: "mixed"
    (the images' rows interleaved at random, some rows with index -1 or B among them) or "blocks" (image after image,
    each followed by -1 padding).  ``exact``: {image: n} makes exactly n rows of that image candidates of class 1."""
    g = np.random.default_rng(seed)
    B = len(per_img)
    idx = []
    for b, n in enumerate(per_img):
        idx += [b] * n + ([-1] * 3 if layout == "blocks" else [])
    if layout == "mixed":
        idx += [-1, B, -7]
        idx = list(g.permutation(idx))
    idx = np.asarray(idx, np.int64)
    N = idx.shape[0]
    K = 1 if agnostic else C - 1
    ncl = max(4, N // 12)
    centres = g.integers(0, 1200, (ncl, 2))
    k = g.integers(0, ncl, (N, K))
    xy = centres[k] + g.integers(-8, 9, (N, K, 2))
    wh = g.integers(24, 48, (N, K, 2))
    boxes = np.concatenate([xy, xy + wh], -1).reshape(N, 4 * K).astype(f32)
    low = VALUES <= f32(THR)
    w = np.where(low, p_low / low.sum(), (1 - p_low) / (~low).sum())
    scores = g.choice(VALUES, (N, C), p=w).astype(f32)
    for b, n in (exact or {}).items():
        rows = np.nonzero(idx == b)[0]
        scores[rows, 1] = f32(THR)
        scores[rows[:n], 1] = g.choice(VALUES[~low], n)
    return boxes, scores, idx, B


MC_CASES = {
    # name: (seed, rows per image, C, layout, agnostic, max_num, index dtype (None: no batch_idx), exact)
    "n63_c5": (1, (63,), 5, "blocks", False, 100, None, None),
    "n64_c2": (2, (64,), 2, "mixed", False, 100, np.int32, None),
    "n65_c81_agnostic_top1": (3, (65,), 81, "mixed", True, 1, np.int64, None),
    "n1000_c81": (4, (1000,), 81, "blocks", False, 100, None, None),
    "b3_n1_64_65_c5_all": (5, (1, 64, 65), 5, "mixed", False, 8192, np.int32, None),
    "b3_n63_1000_1_c81_agnostic": (6, (63, 1000, 1), 81, "blocks", True, 100, np.int64, None),
    "n200_c1024": (7, (200,), 1024, "mixed", False, 100, np.int32, None),
    "b3_n65_63_64_c2": (8, (65, 63, 64), 2, "mixed", False, 100, np.int64, None),
    "b3_4096_4097_candidates": (9, (4100, 4200, 65), 3, "blocks", True, 100, np.int32, {0: 4096, 1: 4097}),
}


@pytest.mark.parametrize("name", sorted(MC_CASES))
def test_multiclass_nms_bit_exact(T, name):
    seed, per_img, C, layout, agnostic, max_num, idt, exact = MC_CASES[name]
    boxes, scores, idx, B = mc_case(seed, per_img, C, layout, agnostic, exact)
    if idt is None:                                   # one image, no index: every row belongs to it
        idx = None
    st = {}
    ref = D.multiclass_nms(boxes, scores, idx, B, THR, 0.5, max_num, st)
    # the oracle's own result is not hollow
    assert sum(st["classes"]) >= min(2, C - 1) and max(st["classes"]) >= min(2, C - 1), st["classes"]
    assert sum(st["suppressed"]) >= 1
    assert (scores == f32(THR)).any()
    if exact:
        assert ref[3].tolist()[:2] == [max_num, -1] and ref[3][2] > 0
    SEEN["over"] += any(t > max_num for t in st["total"])
    SEEN["under"] += any(0 <= t < max_num for t in st["total"])
    got = T.multiclass_nms(_cuda(boxes), _cuda(scores), _cuda(None if idx is None else idx.astype(idt)), B, THR, 0.5,
                           max_num)
    assert_same(got, ref, name)
    again = T.multiclass_nms(_cuda(boxes), _cuda(scores), _cuda(None if idx is None else idx.astype(idt)), B, THR, 0.5,
                             max_num)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_multiclass_nms_no_rows_and_negative_threshold(T):
    z = torch.zeros(0, 8, device="cuda"), torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda")
    dets, labels, rows, counts = T.multiclass_nms(*z, 2, max_num=3)
    assert counts.tolist() == [0, 0] and not dets.any() and (labels == -1).all() and (rows == -1).all()
    # -0.0 ties with +0.0 and comes back as the stored -0.0
    boxes = np.stack([f32([10, 10, 29, 29]) + 100 * i for i in range(3)])
    scores = f32([[0, -0.0, 0.0], [0, 0.0, -0.0], [0, -1, -1]])
    ref = D.multiclass_nms(boxes, scores, None, 1, -0.5, 0.5, 3)
    assert_same(T.multiclass_nms(_cuda(boxes), _cuda(scores), None, 1, -0.5, 0.5, 3), ref, "signed zeros")
    assert ref[0][0, :, 4].view(np.uint32).tolist() == [0x80000000, 0, 0]


# ---- bbox_head_detections -------------------------------------------------------------------------------------------
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2)
SHAPES = [(600, 900), (480, 1000)]


def head_case(R, C, dtype, agnostic, style, seed):
    g = np.random.default_rng(seed)
    B = len(SHAPES)
    xy = g.uniform(0, 700, (R, 2))
    wh = g.uniform(16, 200, (R, 2))
    img = g.integers(0, B, (R, 1)).astype(np.float64)
    img[g.random((R, 1)) < 0.15] = -1                                    # padding rows
    if R > 3:
        img[1], img[2] = B, 0.5                                          # outside / truncates to image 0
    rois = np.concatenate([img, xy, xy + wh], 1).astype(f32)
    if style == "dominant":
        x = g.normal(0, 1.0, (R, C))
        x[np.arange(R), g.integers(0, C, R)] += 12.0
    else:
        x = g.normal(0, 0.01, (R, C))
    K = 1 if agnostic else C
    d = g.normal(0, 0.8, (R, K, 4))
    d[::3, :, 2:] = 0                                                    # exp-free rows
    cls = torch.from_numpy(x).to(dtype).contiguous()
    reg = torch.from_numpy(d.reshape(R, 4 * K)).to(dtype).contiguous()
    return torch.from_numpy(rois), cls, reg


def decode_tolerance(rois, deltas):
    """§4b: 4·spacing(max(|gx|, gw, 1)) per x coordinate (y alike), from float64 stand-ins."""
    R = rois.shape[0]
    dd = deltas.reshape(R, -1, 4).astype(np.float64) * np.asarray(STDS)
    tol = np.empty(dd.shape, np.float64)
    for ax in (0, 1):
        pw = ((rois[:, 3 + ax] - rois[:, 1 + ax]) + 1)[:, None].astype(np.float64)
        gw = pw * np.exp(np.clip(dd[..., 2 + ax], -4.1351666, 4.1351666))
        gx = np.abs((rois[:, 1 + ax] + rois[:, 3 + ax])[:, None] * 0.5 + pw * dd[..., ax])
        t = 4 * np.spacing(np.maximum(np.maximum(gx, gw), 1.0).astype(f32)).astype(np.float64)
        tol[..., ax], tol[..., 2 + ax] = t, t
    return tol.reshape(R, -1)


def run_head(T, R, C, dt, agnostic, style, scale_kind, seed, thr=THR, max_per_img=100):
    rois, cls, reg = head_case(R, C, DTYPES[dt], agnostic, style, seed)
    scale = {"none": None, "number": 1.25, "tensor": np.asarray([0.8, 1.6], f32)}[scale_kind]
    ish = torch.tensor(SHAPES, dtype=torch.int32).cuda()
    args = (rois.cuda(), cls.cuda(), reg.cuda(), ish, _cuda(scale) if scale_kind == "tensor" else scale)
    kw = dict(score_thr=thr, nms_thr=0.5, max_per_img=max_per_img, target_means=MEANS, target_stds=STDS)
    out = T.bbox_head_detections(*args, return_dense=True, **kw)
    assert len(out) == 6
    scores, boxes = out[4].cpu().numpy(), out[5].cpu().numpy()
    x, d = cls.float().numpy(), reg.float().numpy()
    p64, z, ref_boxes, rscale, img = D.dense(rois.numpy(), x, d, SHAPES, scale, MEANS, STDS)
    # 1. dense scores
    assert scores.dtype == f32 and scores.shape == (R, C)
    err = np.abs(scores.astype(np.float64) - p64)
    bound = (16 + np.abs(z)) * U * p64 + 2.0 ** -149
    bound[img < 0] = 0
    assert (err <= bound).all(), "scores: worst error / bound %.3g" % (err / np.maximum(bound, 1e-300)).max()
    # 2. dense boxes
    deltas = d if agnostic else d[:, 4:]
    assert boxes.dtype == f32 and boxes.shape == ref_boxes.shape == (R, deltas.shape[1])
    tol = decode_tolerance(rois.numpy(), deltas)
    ref = ref_boxes.astype(np.float64)
    if rscale is not None:
        ref = ref / rscale[:, None].astype(np.float64)
        tol = tol / rscale[:, None] + np.spacing(np.abs(ref).astype(f32))
    tol[img < 0] = 0
    berr = np.abs(boxes.astype(np.float64) - ref)
    assert (berr <= tol).all(), "boxes: worst error / tolerance %.3g" % (berr / np.maximum(tol, 1e-300)).max()
    exact = ref_boxes if rscale is None else (ref_boxes / rscale[:, None]).astype(f32)
    assert np.array_equal(boxes[::3].view(np.uint32), exact[::3].view(np.uint32)), "exp-free rows are bit-exact"
    assert not scores[img < 0].any() and not boxes[img < 0].any()
    # 3. final outputs: the oracle on the GPU's own dense values
    st = {}
    ref_out = D.multiclass_nms(boxes, scores, img, len(SHAPES), thr, 0.5, max_per_img, st)
    assert_same(out[:4], ref_out, "head R%d C%d %s" % (R, C, dt))
    # 4. the selection path does not depend on return_dense
    plain = T.bbox_head_detections(*args, **kw)
    assert len(plain) == 4
    for a, b in zip(plain, out[:4]):
        assert torch.equal(a, b)
    return out, st, img


HEAD_VARIANTS = [(False, "dominant", "none"), (True, "uniform", "number"), (False, "uniform", "tensor"),
                 (True, "dominant", "tensor"), (False, "dominant", "number"), (True, "uniform", "none")]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("C", [2, 81])
@pytest.mark.parametrize("R", [1, 7, 512, 1031])
def test_bbox_head_detections(T, R, C, dt):
    i = [1, 7, 512, 1031].index(R) + (4 if C == 81 else 0) + sorted(DTYPES).index(dt)
    agnostic, style, scale_kind = HEAD_VARIANTS[i % 6]
    # near-uniform rows score 1 / C each: a threshold under that keeps them candidates
    thr = THR if style == "dominant" else 0.5 / C
    run_head(T, R, C, dt, agnostic, style, scale_kind, 100 + i, thr)
    agnostic, style, scale_kind = HEAD_VARIANTS[(i + 3) % 6]
    thr = THR if style == "dominant" else 0.5 / C
    run_head(T, R, C, dt, agnostic, style, scale_kind, 200 + i, thr)


def test_head_cases_are_not_hollow(T):
    out, st, img = run_head(T, 1031, 81, "f32", False, "dominant", "none", 7)
    assert sum(st["suppressed"]) > 0 and min(st["classes"]) >= 2 and (out[3] > 0).all()
    out, st, img = run_head(T, 512, 81, "bf16", True, "uniform", "number", 8, thr=0.5 / 81, max_per_img=50)
    assert sum(st["suppressed"]) > 0 and max(st["total"]) > 50 and out[3].tolist() == [50, 50]


def test_chain_from_rpn_proposals(T):
    levels = [((50, 84), 4), ((25, 42), 8), ((13, 21), 16), ((7, 11), 32)]
    gens = [T.AnchorGenerator(s, [8], [0.5, 1.0, 2.0]) for _, s in levels]
    anchors, _ = T.anchor_pyramid(gens, [fs for fs, _ in levels], [s for _, s in levels], "cuda")
    B, C = 2, 21
    g = torch.Generator().manual_seed(21)
    cls = [torch.randn(B, 3, h, w, generator=g).bfloat16().cuda() for (h, w), _ in levels]
    reg = [(torch.randn(B, 12, h, w, generator=g) * 0.5).bfloat16().cuda() for (h, w), _ in levels]
    ish = torch.tensor([(200, 336), (180, 300)], dtype=torch.int32).cuda()
    M = 1200                                          # more than the 300 + 300 + 300 + 231 boxes that leave the levels
    props, _, pc = T.rpn_proposals(cls, reg, anchors, ish, nms_pre=300, nms_post=300, max_num=M, nms_thr=0.9)
    rois = T.rois_from_proposals(props, pc)
    R = rois.shape[0]
    logits = torch.randn(R, C, generator=g) * 2
    logits[:, 0] -= 1
    deltas = torch.randn(R, 4 * C, generator=g) * 0.5
    dets, labels, rows, counts, scores, boxes = T.bbox_head_detections(
        rois, logits.cuda(), deltas.cuda(), ish, score_thr=0.2, max_per_img=60, return_dense=True)
    pc, rois_h = pc.cpu().numpy(), rois.cpu().numpy()
    assert (pc < M).all() and (pc > 0).all(), "the case has padded RoIs"
    img = D.roi_images(rois_h, B)
    assert ((img >= 0).reshape(B, M).sum(1) == pc).all()
    scores, boxes = scores.cpu().numpy(), boxes.cpu().numpy()
    assert not scores[img < 0].any() and not boxes[img < 0].any()
    ref = D.multiclass_nms(boxes, scores, img, B, 0.2, 0.5, 60)
    assert_same((dets, labels, rows, counts), ref, "chain")
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    assert (counts > 0).all()
    for b in range(B):
        r = rows[b, :counts[b]]
        assert (r // M == b).all() and (r % M < pc[b]).all()       # only the image's own, unpadded RoIs


def test_graph_capture_and_replay(T):
    """Both functions captured once and replayed on new scores, logits and img_shapes: a host synchronisation or an
    allocation inside the library would break the capture.  Eager and replayed results agree bit for bit."""
    def new(seed):
        b, s, i, _ = mc_case(seed, (150, 90), 7, "mixed", False)
        r, c, d = head_case(300, 21, torch.bfloat16, False, "dominant", seed)
        sh = torch.tensor([(600 - seed, 900), (480, 1000 - 3 * seed)], dtype=torch.int32)
        return [torch.from_numpy(b), torch.from_numpy(s), torch.from_numpy(i), r, c, d, sh]
    bufs = [t.cuda() for t in new(1)]

    def step():
        a = T.multiclass_nms(bufs[0], bufs[1], bufs[2], 2, THR, 0.5, 40)
        h = T.bbox_head_detections(bufs[3], bufs[4], bufs[5], bufs[6], 1.5, max_per_img=30, return_dense=True)
        return list(a) + list(h)

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
            assert torch.equal(a, b) if a.dtype != torch.float32 else np.array_equal(_bits(a), _bits(b))
        seen.append([captured[0].clone(), captured[4].clone()])
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])


# ---- under the guard -------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import detect_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, detect_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


@pytest.mark.parametrize("name", ["b3_n1_64_65_c5_all", "n65_c81_agnostic_top1", "b3_4096_4097_candidates"])
def test_guarded_multiclass_nms(T, guard, name):
    """Poisoned outputs: the unused rows must have been WRITTEN, as 0 / -1, and the oversized image's rows too."""
    test_multiclass_nms_bit_exact(T, name)
    _clean(guard, ["multiclass_nms"])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_guarded_bbox_head_detections(T, guard, dt):
    for R, C, variant in ((1031, 81, 0), (7, 2, 1), (1, 81, 3), (512, 2, 2)):
        agnostic, style, scale_kind = HEAD_VARIANTS[variant]
        run_head(T, R, C, dt, agnostic, style, scale_kind, 300 + R, THR if style == "dominant" else 0.5 / C)
        _clean(guard, ["bbox_head_detections"])


def test_guarded_no_rows(T, guard):
    ish = torch.tensor(SHAPES, dtype=torch.int32).cuda()
    out = T.bbox_head_detections(torch.zeros(0, 5, device="cuda"), torch.zeros(0, 5, device="cuda"),
                                 torch.zeros(0, 20, device="cuda"), ish, max_per_img=4, return_dense=True)
    _clean(guard, [])
    assert out[3].tolist() == [0, 0] and not out[0].any() and (out[1] == -1).all() and out[4].shape == (0, 5)


def test_every_detect_entry_point_ran_under_the_guard_and_both_truncation_sides_ran():
    """Counts what the tests above did IN THIS RUN (run the file as a whole)."""
    from torch_detection_amd import detect_ops
    public = sorted(n for n, v in vars(detect_ops).items()
                    if inspect.isfunction(v) and v.__module__ == detect_ops.__name__ and not n.startswith("_"))
    assert public == ["bbox_head_detections", "multiclass_nms"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in public:
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)
    assert SEEN["over"] >= 1 and SEEN["under"] >= 1, SEEN
