"""GPU tests of the mask branch (mask_target, mask_head_loss, rois_from_detections, mask_head_masks; csrc/mask.hip)
against the CPU oracle tests/mask_ref.py: the targets and rois bit for bit, the loss and its gradient
within K_LOSS x 2^-24 of the float64 oracle, the paste equal to the oracle except where the float64 value lies within
K_PASTE x 2^-24 of the threshold; graph replay; the chain from sample_rois; and every entry point of mask_ops.py under
guard-banded, poisoned outputs with exact-size workspaces (tests/guard_util.py)."""
import inspect

import numpy as np
import pytest
import torch

import guard_util as G
import mask_cases as MC
import mask_ref as R

pytestmark = pytest.mark.gpu

U = MC.U
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT = {torch.bfloat16: 7, torch.float16: 10}
ENTERED, WS_SEEN = set(), {}        # what ran under the guard in this run (checked by the last test of the file)


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared cases stay as they are


def _bits(t):
    t = t.detach().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _ulp16(ref, dtype):
    """Spacing of the 16-bit type at |ref| (its smallest subnormal below the normal range)."""
    if dtype == torch.float32:
        return np.zeros_like(ref)
    emin = -14 if dtype == torch.float16 else -126
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref), where=ref != 0, out=np.full(ref.shape, float(emin))))
    return 2.0 ** (np.maximum(e, emin) - MANT[dtype])


def _layout(t, nhwc):
    return t.contiguous(memory_format=torch.channels_last) if nhwc else t.contiguous()


@pytest.fixture(scope="module")
def polys(T):
    cpu = T.pack_polygons(MC.target_polys(), MC.G)
    return [t.numpy() for t in cpu], [t.cuda() for t in cpu]


# ---- mask_target -----------------------------------------------------------------------------------------------------
def _check_targets(T, polys, M):
    (xy, po, gpo), gpu = polys
    rois, inds = MC.target_rows(M)
    want_t, want_w = R.mask_target(rois, inds, xy, po, gpo, M)
    got_t, got_w = T.mask_target(_cuda(rois), _cuda(inds), *gpu, mask_size=M)
    assert got_t.shape == (40, M, M) and got_t.dtype == torch.uint8 and got_w.dtype == torch.float32
    gt, gw = got_t.cpu().numpy(), got_w.cpu().numpy()
    bad = np.nonzero((gt != want_t).reshape(40, -1).any(1))[0]
    assert bad.size == 0, "rows %s differ (%d cells)" % (bad.tolist(), int((gt != want_t).sum()))
    assert np.array_equal(gw.view(np.uint32), want_w.view(np.uint32))
    assert want_t.sum() > 0
    return want_t, want_w


@pytest.mark.parametrize("M", [28, 7, 1])
def test_mask_target_bit_equal(T, polys, M):
    _check_targets(T, polys, M)
    # a slice of rows and no rows at all
    (xy, po, gpo), gpu = polys
    rois, inds = MC.target_rows(M)
    t, w = T.mask_target(_cuda(rois[10:17]), _cuda(inds[10:17]), *gpu, mask_size=M)
    want_t, want_w = R.mask_target(rois[10:17], inds[10:17], xy, po, gpo, M)
    assert np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(w.cpu().numpy(), want_w)
    t, w = T.mask_target(_cuda(rois[:0]), _cuda(inds[:0]), *gpu, mask_size=M)
    assert t.shape == (0, M, M) and w.shape == (0,)


def test_mask_target_wild_offsets_are_clamped(T, polys):
    """Offsets outside their arrays (a corrupt pack) are clamped on the device: no fault, and equal to the oracle, which
    clamps the same way."""
    (xy, po, gpo), gpu = polys
    po2, gpo2 = po.copy(), gpo.copy()
    po2[2], po2[4] = -5, 1 << 30
    gpo2[1, 2], gpo2[0, 3] = 1 << 30, -3
    rois, inds = MC.target_rows(7)
    want_t, want_w = R.mask_target(rois, inds, xy, po2, gpo2, 7)
    t, w = T.mask_target(_cuda(rois), _cuda(inds), gpu[0], _cuda(po2), _cuda(gpo2), mask_size=7)
    assert np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(w.cpu().numpy(), want_w)


# ---- mask_head_loss --------------------------------------------------------------------------------------------------
def _cotangent(dtype):
    return 32768.0 if dtype == torch.float16 else 1.5           # an fp16 loss scale arrives as the cotangent


def run_loss(T, case, dtype, nhwc, avg_gpu, avg_ref, what):
    """forward + backward twice (bitwise equal), then everything against the oracle."""
    pred, targets, labels, w = case
    g = _cotangent(dtype)
    x = _layout(_cuda(pred).to(dtype), nhwc)
    tg = [_cuda(targets), _cuda(labels), _cuda(w)]
    gt = torch.tensor([g], dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):
        leaf = x.detach().requires_grad_(True)
        loss = T.mask_head_loss(leaf, *tg, avg_factor=avg_gpu)
        runs.append((loss, torch.autograd.grad(loss, [leaf], gt)[0]))
    torch.cuda.synchronize()
    (loss, grad), (loss2, grad2) = runs
    assert loss.shape == (1,) and loss.dtype == torch.float32
    assert grad.shape == x.shape and grad.dtype == dtype and grad.stride() == x.stride(), (grad.stride(), x.stride())
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(grad), _bits(grad2)), what + ": run to run"
    stored = x.float().cpu().numpy()
    ref = R.mask_head_loss(stored, targets, labels, w, avg_ref, g=g)
    got = _np64(grad)
    assert np.all(np.isfinite(got)), what
    assert np.array_equal(got == 0, ref["dpred"] == 0), "%s: zero pattern differs at %d elements" % (
        what, int(((got == 0) != (ref["dpred"] == 0)).sum()))
    unit = U * ref["unit"][:, None, None, None] * np.ones_like(got)
    err = np.abs(got - ref["dpred"])
    live = unit > 0
    worst = float((err[live] / unit[live]).max()) if live.any() else 0.0
    tol = MC.K_LOSS * unit + _ulp16(ref["dpred"], dtype)
    lerr = abs(float(loss.item()) - ref["loss"])
    lworst = lerr / (U * ref["mag"]) if ref["mag"] > 0 else 0.0
    print("%s: loss %r (ref %r) avg %g, loss error %.2f, worst gradient error %.2f (x 2^-24 of the bound's unit)" % (
        what, float(loss.item()), ref["loss"], float(ref["avg"]), lworst, worst))
    assert np.all(err <= tol), "%s: %d gradient elements beyond the bound, worst %.2f x 2^-24 |g w| / (D M^2)" % (
        what, int((err > tol).sum()), worst)
    ltol = MC.K_LOSS * U * ref["mag"] + float(np.spacing(np.float32(abs(ref["loss"]))))
    assert lerr <= ltol, "%s: loss %r, ref %r, error %g > %g" % (what, float(loss.item()), ref["loss"], lerr, ltol)
    return ref, loss, grad


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("C,M", [(5, 28), (5, 7), (1, 28), (1, 7)])
def test_mask_head_loss_vs_oracle(T, C, M, dt):
    case = MC.loss_case(24, C, M, 10 * C + M)
    assert (case[3] == 0).sum() >= 3 and np.isnan(case[0]).any()
    for nhwc in (False, True):
        run_loss(T, case, DTYPES[dt], nhwc, None, None, "C%d M%d %s %s" % (C, M, dt, "nhwc" if nhwc else "nchw"))


def test_mask_head_loss_avg_factor_forms(T):
    case = MC.loss_case(24, 5, 7, 21)
    a = torch.tensor([3, 4], dtype=torch.int32, device="cuda")
    b = torch.tensor([10, 0, 2], dtype=torch.int32, device="cuda")
    z = torch.zeros(2, dtype=torch.int32, device="cuda")
    for gpu, ref in ((19.5, 19.5), (a, np.array([3, 4])), ((a, b), (np.array([3, 4]), np.array([10, 0, 2]))),
                     ((z, z), (np.zeros(2, int), np.zeros(2, int)))):
        out, _, _ = run_loss(T, case, torch.float32, False, gpu, ref, "avg forms")
        assert out["avg"] == R.L.divisor(ref)


def test_mask_head_loss_all_weights_zero(T):
    from torch_detection_amd import mask_ops
    case = MC.loss_case(24, 5, 7, 22, all_zero=True)
    ref, loss, grad = run_loss(T, case, torch.float32, True, None, None, "all rows weight 0")
    assert float(loss.item()) == 0.0 and not grad.any() and ref["avg"] == 1
    x = _cuda(case[0])
    loss, avg = mask_ops.mask_head_loss_fwd(x, _cuda(case[1]), _cuda(case[2]), _cuda(case[3]), None)
    assert loss.tolist() == [0.0] and avg.tolist() == [1.0]


def test_mask_head_loss_more_rows_than_partials(T):
    """R = 300 rows: more than the 256 workgroups of the forward launch, so some take two rows."""
    run_loss(T, MC.loss_case(300, 3, 7, 23), torch.bfloat16, True, None, None, "R300")


def test_mask_head_loss_graph_replay(T):
    """Forward + backward captured once and replayed on new logits, targets and weights: bit-equal to eager."""
    def new(seed):
        return MC.loss_case(24, 5, 28, seed)
    c = new(1)
    x = _cuda(c[0]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    tg = [_cuda(c[1]), _cuda(c[2]), _cuda(c[3])]
    cot = torch.tensor([2.0], device="cuda")

    def step():
        loss = T.mask_head_loss(x, *tg)
        return [loss, torch.autograd.grad(loss, [x], cot)[0]]

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
        c = new(seed)
        with torch.no_grad():
            x.copy_(_cuda(c[0]))
            for dst, src in zip(tg, c[1:]):
                dst.copy_(_cuda(src))
        graph.replay()
        eager = step()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(_bits(a), _bits(b))
        seen.append(captured[0].clone())
    assert not torch.equal(seen[0], seen[1])


# ---- rois_from_detections --------------------------------------------------------------------------------------------
def test_rois_from_detections_bit_equal(T):
    g = np.random.default_rng(5)
    dets = (g.random((3, 7, 5)) * 500).astype(np.float32)
    counts = np.array([0, 7, -1], np.int32)
    scales = np.array([0.37, 1.6, 2.0], np.float32)
    for cn in (counts, np.array([3, 7, 1], np.int32)):
        for gpu, ref in ((None, None), (0.37, 0.37), (_cuda(scales), scales)):
            got = T.rois_from_detections(_cuda(dets), _cuda(cn), gpu)
            want = R.rois_from_detections(dets, cn, ref)
            assert got.shape == (21, 5) and got.dtype == torch.float32
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- mask_head_masks -------------------------------------------------------------------------------------------------
def run_paste(T, C, M, dtype, nhwc, img_shapes, what):
    x = _layout(_cuda(MC.paste_pred(C, M)).to(dtype), nhwc)
    stored = x.float().cpu().numpy()
    want, v = R.mask_head_masks(stored, MC.PASTE_DETS, MC.PASTE_LABELS, MC.PASTE_COUNTS, MC.CANVAS, img_shapes, 0.5)
    args = (x, _cuda(MC.PASTE_DETS), _cuda(MC.PASTE_LABELS), _cuda(MC.PASTE_COUNTS), MC.CANVAS)
    kw = dict(img_shapes=None if img_shapes is None else _cuda(img_shapes), thr=0.5)
    got = T.mask_head_masks(*args, **kw)
    packed = T.mask_head_masks(*args, packed=True, **kw)
    H, W = MC.CANVAS
    assert got.shape == (12, H, W) and got.dtype == torch.uint8
    assert packed.shape == (12, H, 8 * ((W + 63) // 64)) and packed.dtype == torch.uint8
    got, packed = got.cpu().numpy(), packed.cpu().numpy()
    assert set(np.unique(got).tolist()) <= {0, 1}
    near = MC.near_threshold(v, 0.5)
    n = MC.box_pixels(v)
    differ = (got != want) & ~near
    print("%s: %d box pixels, %d set, %d near the threshold, %d differ from the oracle there" % (
        what, n, int(want.sum()), int(near.sum()), int(((got != want) & near).sum())))
    assert int(near.sum()) * 10 ** 4 <= n
    assert not differ.any(), "%s: %d pixels differ, first %s" % (what, int(differ.sum()), np.argwhere(differ)[0])
    assert np.array_equal(packed, R.pack_bits(got)), what + ": packed"
    assert np.array_equal(np.unpackbits(packed, axis=-1, bitorder="little")[..., :W], got)
    return got


@pytest.mark.parametrize("C", [4, 1])
@pytest.mark.parametrize("M", [28, 14])
def test_mask_head_masks_vs_oracle(T, C, M):
    for dt, nhwc, shapes in (("f32", False, MC.PASTE_IMG_SHAPES), ("f32", True, None), ("bf16", True, MC.PASTE_IMG_SHAPES),
                             ("f16", False, MC.PASTE_IMG_SHAPES)):
        run_paste(T, C, M, DTYPES[dt], nhwc, shapes, "C%d M%d %s %s" % (C, M, dt, "nhwc" if nhwc else "nchw"))


def test_mask_head_masks_constant_logits(T):
    """Logits of +8 fill the clipped boxes, -8 nothing, and 0 at thr = 0.5 nothing: sigma(0) is 0.5 exactly and the box
    sizes here (multiples of 2M) make every sample position dyadic."""
    dets = _cuda(np.array([[[3, 2, 10, 9, 1], [-4, -3, 11, 12, 1], [60, 60, 75, 75, 1]]], np.float32))
    labels = torch.zeros(1, 3, dtype=torch.int64, device="cuda")
    counts = torch.tensor([3], dtype=torch.int32, device="cuda")
    want = np.zeros((3, 70, 150), np.uint8)
    want[0, 2:10, 3:11] = 1
    want[1, 0:13, 0:12] = 1
    want[2, 60:70, 60:76] = 1
    for logit, res in ((8.0, want), (-8.0, 0 * want), (0.0, 0 * want)):
        x = torch.full((3, 1, 4, 4), logit, device="cuda")
        got = T.mask_head_masks(x, dets, labels, counts, MC.CANVAS).cpu().numpy()
        assert np.array_equal(got, res), logit
    x = torch.zeros(3, 1, 4, 4, device="cuda")
    assert T.mask_head_masks(x, dets, labels, counts, MC.CANVAS, thr=0.4999).cpu().numpy().sum() == want.sum()
    # the overflow marker of multiclass_nms: nothing is drawn
    none = T.mask_head_masks(x + 8, dets, labels, torch.tensor([-1], dtype=torch.int32, device="cuda"), MC.CANVAS)
    assert not none.any()


# ---- the chain --------------------------------------------------------------------------------------------------------
def _chain_inputs(T):
    g = np.random.default_rng(9)
    gt = np.array([[[30, 40, 120, 140], [130, 20, 230, 100], [60, 150, 200, 240]],
                   [[20, 20, 110, 90], [140, 120, 240, 230], [0, 0, 0, 0]]], np.float32)
    gt_counts = np.array([3, 2], np.int32)
    gt_labels = np.array([[3, 1, 7], [2, 5, 0]], np.int64)
    polys = []
    for b in range(2):
        inst = []
        for j in range(gt_counts[b]):
            x1, y1, x2, y2 = gt[b, j]
            rx, ry = (x2 - x1) / 2, (y2 - y1) / 2
            s = MC.star(0, 0, 0.6, 1.0, 12, 50 + 3 * b + j)
            inst.append([MC.flat(s * np.array([rx, ry], np.float32) + np.array([x1 + rx, y1 + ry], np.float32))])
        polys.append(inst)
    props = np.zeros((2, 64, 5), np.float32)
    for b in range(2):
        for k in range(64):
            if k < 40:
                props[b, k, :4] = gt[b, k % gt_counts[b]] + g.integers(-8, 9, 4)
            else:
                xy = g.uniform(0, 180, 2)
                props[b, k, :4] = [xy[0], xy[1], xy[0] + g.uniform(20, 70), xy[1] + g.uniform(20, 70)]
            props[b, k, 4] = 1.0 - k / 64
    counts = np.array([64, 50], np.int32)
    feats = [(torch.randn(2, 8, 256 // s, 256 // s, generator=torch.Generator().manual_seed(s)) * 0.5).to(
        torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True) for s in (4, 8, 16, 32)]
    return ([_cuda(a) for a in (props, counts, gt, gt_labels, gt_counts)], [t.cuda() for t in T.pack_polygons(polys, 3)],
            [t.numpy() for t in T.pack_polygons(polys, 3)], feats)


def test_chain_sample_rois_to_mask_loss_graph(T):
    """sample_rois -> positive-block slice -> mask_target -> roi_align 14 x 14 -> a scale per channel standing in for
    the head -> mask_head_loss -> backward, B = 2, num = 32: captured once through torch.cuda.graph and compared with
    eager; the targets and the loss also against the oracle."""
    sample_in, pg, pc, feats = _chain_inputs(T)
    head = torch.linspace(0.5, 3.0, 8, device="cuda").view(1, 8, 1, 1).requires_grad_(True)
    num, npos, M = 32, 8, 14

    def step():
        out = T.sample_rois(*sample_in, num=num, pos_fraction=npos / num, seed=3)
        rois = out[0].view(2, num, 5)[:, :npos].reshape(-1, 5)
        labels = out[1].view(2, num)[:, :npos].reshape(-1)
        inds = out[5].view(2, num)[:, :npos].reshape(-1)
        targets, weights = T.mask_target(rois, inds, *pg, mask_size=M)
        x = T.roi_align(feats, rois, out_size=M, featmap_strides=(4, 8, 16, 32))
        pred = (x.float() * head).contiguous(memory_format=torch.channels_last)
        loss = T.mask_head_loss(pred, targets, labels, weights)
        grads = torch.autograd.grad(loss, [pred, head] + feats)
        return [rois, labels, inds, targets, weights, pred, loss] + list(grads)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        for t in captured:
            t.zero_()
    graph.replay()
    eager = step()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(captured, eager)):
        if k == 8:                                       # the head's gradient is a torch reduction
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-8)
        else:
            assert torch.equal(_bits(a), _bits(b)), k
    rois, labels, inds, targets, weights, pred, loss, dpred = (t.detach().cpu() for t in captured[:8])
    assert pred.shape == (16, 8, M, M) and pred.is_contiguous(memory_format=torch.channels_last)
    assert 4 <= int((weights > 0).sum()) <= 16 and int((inds >= 0).sum()) == int((weights > 0).sum())
    want_t, want_w = R.mask_target(rois.numpy(), inds.numpy(), *pc, M)
    assert np.array_equal(targets.numpy(), want_t) and np.array_equal(weights.numpy(), want_w)
    assert 0.2 < want_t[want_w > 0].mean() < 0.9         # the stars fill a good part of their boxes
    ref = R.mask_head_loss(pred.numpy(), want_t, labels.numpy(), want_w, None)
    assert abs(float(loss.item()) - ref["loss"]) <= MC.K_LOSS * U * ref["mag"] + float(np.spacing(np.float32(ref["loss"])))
    err = np.abs(dpred.numpy().astype(np.float64) - ref["dpred"])
    assert np.all(err <= MC.K_LOSS * U * ref["unit"][:, None, None, None])
    assert any(bool(t.any()) for t in captured[9:])      # the gradient went on through roi_align into the pyramid


# ---- under the guard ---------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import mask_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, mask_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


@pytest.mark.parametrize("M", [28, 7, 1])
def test_guarded_mask_target(T, guard, polys, M):
    _check_targets(T, polys, M)
    assert guard.calls["mask_target"] == 2
    _clean(guard, ["mask_target"])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_guarded_mask_head_loss(T, guard, dt):
    for C, M, nhwc in ((5, 7, False), (1, 28, True), (5, 28, True), (3, 1, False)):
        run_loss(T, MC.loss_case(24, C, M, 31), DTYPES[dt], nhwc, None, None, "guarded C%d M%d %s" % (C, M, dt))
        _clean(guard, ["mask_head_loss_fwd", "mask_head_loss_bwd"])
    run_loss(T, MC.loss_case(300, 3, 7, 32), DTYPES[dt], True, 7.0, 7.0, "guarded R300 %s" % dt)
    _clean(guard, [])


def test_guarded_mask_head_loss_no_rows(T, guard):
    from torch_detection_amd import mask_ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    loss, avg = mask_ops.mask_head_loss_fwd(z(0, 5, 7, 7), z(0, 7, 7, dt=torch.uint8), z(0, dt=torch.int64), z(0), None)
    _clean(guard, [])
    assert loss.tolist() == [0.0] and avg.tolist() == [1.0]


def test_guarded_rois_from_detections(T, guard):
    test_rois_from_detections_bit_equal(T)
    _clean(guard, ["rois_from_detections"])


@pytest.mark.parametrize("C,M", [(4, 28), (1, 14)])
def test_guarded_mask_head_masks(T, guard, C, M):
    for dt, nhwc in (("f32", False), ("bf16", True)):
        x = _layout(_cuda(MC.paste_pred(C, M)).to(DTYPES[dt]), nhwc)
        args = (x, _cuda(MC.PASTE_DETS), _cuda(MC.PASTE_LABELS), _cuda(MC.PASTE_COUNTS), MC.CANVAS)
        got = T.mask_head_masks(*args, img_shapes=_cuda(MC.PASTE_IMG_SHAPES))
        _clean(guard, ["mask_head_masks"])
        # packed bytes of a noisy mask can equal the guard's poison byte, which would read as "never written": the
        # packed output is guarded on solid masks (logits of +8: runs of ones, whose bytes never are 0x5A)
        solid = T.mask_head_masks(torch.full_like(x, 8.0), *args[1:], img_shapes=_cuda(MC.PASTE_IMG_SHAPES), packed=True)
        _clean(guard, [])
        full = T.mask_head_masks(torch.full_like(x, 8.0), *args[1:], img_shapes=_cuda(MC.PASTE_IMG_SHAPES))
        _clean(guard, [])
        assert np.array_equal(solid.cpu().numpy(), R.pack_bits(full.cpu().numpy()))
        assert got.any() and full.sum() > got.sum()


def test_value_errors_on_mixed_devices(T, polys):
    _, gpu = polys
    rois, inds = (_cuda(a) for a in MC.target_rows(7))
    with pytest.raises(ValueError, match="poly_xy must be a CUDA tensor"):
        T.mask_target(rois, inds, gpu[0].cpu(), gpu[1], gpu[2], mask_size=7)
    x = torch.zeros(4, 3, 7, 7, device="cuda")
    tg, lab, w = torch.zeros(4, 7, 7, dtype=torch.uint8, device="cuda"), torch.ones(4, dtype=torch.int64), torch.ones(4)
    with pytest.raises(ValueError, match="labels must be a CUDA tensor"):
        T.mask_head_loss(x, tg, lab, w.cuda())
    with pytest.raises(ValueError, match="mask_pred must be"):
        T.mask_head_loss(x[:, :, :, ::2], tg, lab.cuda(), w.cuda())


def test_every_mask_entry_point_ran_under_the_guard():
    """Counts what the guarded tests above did IN THIS RUN (run the file as a whole): every public wrapper of
    mask_ops.py returned under the guard, and the tdn_mask_loss_workspace_bytes query was answered at its exact size
    (rounded up only to the 256-byte alignment the header asks for)."""
    from torch_detection_amd import mask_ops
    public = sorted(n for n, v in vars(mask_ops).items()
                    if inspect.isfunction(v) and v.__module__ == mask_ops.__name__ and not n.startswith("_"))
    assert public == ["mask_head_loss_bwd", "mask_head_loss_fwd", "mask_head_masks", "mask_target",
                      "rois_from_detections"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    asked, given = WS_SEEN["mask_head_loss_fwd"]
    assert 0 <= given - asked < 256 and asked > 0, (asked, given)
