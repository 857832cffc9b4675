"""GPU tests of Mask Scoring R-CNN (mask_iou_stem, mask_iou_target, mask_iou_loss, mask_scores, MaskIoUHead;
csrc/mask_iou.hip) against the CPU oracle tests/ms_rcnn_ref.py: the target and the scores bit for bit; the
mask channel of the first layer, its two gradients, the loss and its gradient within the bounds of tests/ms_rcnn_cases.py
of the float64 oracle; the whole first layer and the head against float64 torch; identical bits run to run and from a
graph replay; the chain beside the mask loss; and every entry point of mask_iou_ops.py under guard-banded, poisoned
outputs with exact-size workspaces (tests/guard_util.py)."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import guard_util as G
import mask_cases as MC
import mask_ref as MR
import ms_rcnn_cases as K
import ms_rcnn_ref as R
import parity_util
from golden_util import rel_l2

pytestmark = pytest.mark.gpu

U = K.U
CL = torch.channels_last
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT = {torch.bfloat16: 7, torch.float16: 10}
ENTERED, WS_SEEN = set(), {}        # what ran under the guard in this run (checked by the last test of the file)


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


@pytest.fixture(scope="module")
def O(T):
    from torch_detection_amd import mask_iou_ops
    return mask_iou_ops


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the shared cases stay as they are


def _bits(t):
    t = t.detach().contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _ulp16(ref, dtype):
    """Spacing of the 16-bit type at |ref| (its smallest subnormal below the normal range); 0 for float32."""
    if dtype == torch.float32:
        return np.zeros_like(ref)
    emin = -14 if dtype == torch.float16 else -126
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref), where=ref != 0, out=np.full(ref.shape, float(emin))))
    return 2.0 ** (np.maximum(e, emin) - MANT[dtype])


def _layout(t, nhwc):
    return t.contiguous(memory_format=CL) if nhwc else t.contiguous()


def _replay(step):
    """Warm up on a side stream, capture ``step`` once, replay it: -> (captured outputs, the graph)."""
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
    torch.cuda.synchronize()
    return captured, graph


@pytest.fixture(scope="module")
def polys():
    cpu = K.packed_polys()
    return [t.numpy() for t in cpu], [t.cuda() for t in cpu]


# ---- mask_iou_target -----------------------------------------------------------------------------------------------------
def _check_target(T, polys, M, C, dt, nhwc, rows=slice(None), three_d=False):
    (xy, po, gpo), gpu = polys
    rois, inds, targets, pred, labels = (a[rows] for a in K.target_case(M, C))
    x = _cuda(pred).to(DTYPES[dt])
    x = x[:, 0].contiguous() if three_d else _layout(x, nhwc)
    stored = x.float().cpu().numpy().reshape(pred.shape)
    want, info = R.mask_iou_target(rois, inds, xy, po, gpo, stored, labels, targets, K.CANVASES, 0.5)
    got = T.mask_iou_target(_cuda(rois), _cuda(inds), *gpu, x, _cuda(labels), _cuda(targets), _cuda(K.CANVASES), thr=0.5)
    assert got.shape == (rois.shape[0],) and got.dtype == torch.float32
    g = got.cpu().numpy()
    bad = np.nonzero(g.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "rows %s differ: got %s, want %s (full %s, inside %s)" % (
        bad.tolist(), g[bad], want[bad], info["full"][bad], info["inside"][bad])
    return want, info


@pytest.mark.parametrize("M", [28, 7, 1])
def test_mask_iou_target_bit_equal(T, polys, M):
    want, info = _check_target(T, polys, M, 5, "f32", False)
    assert (want > 0).sum() >= 10 and info["valid"].sum() >= 30
    _check_target(T, polys, M, 5, "bf16", True)
    _check_target(T, polys, M, 5, "f16", False)
    _check_target(T, polys, M, 1, "f32", False)
    _check_target(T, polys, M, 1, "bf16", False, three_d=True)
    _check_target(T, polys, M, 5, "f32", True, rows=slice(10, 17))
    got = _check_target(T, polys, M, 5, "f32", False, rows=slice(0, 0))[0]
    assert got.shape == (0,)


@pytest.mark.parametrize("w", [1, 63, 64, 65, 129])
def test_mask_iou_target_word_boundaries(T, w):
    """Canvas widths around the 64-pixel word, boxes that start and end on word boundaries, lie off every edge, are
    reversed, saturate or hold NaN; crossings exactly on pixel centres and a vertex on a row of centres."""
    plist, rois, inds, shapes = K.word_case(w)
    cpu = T.pack_polygons(plist, 1)
    xy, po, gpo = (t.numpy() for t in cpu)
    M = 7
    targets, _ = MR.mask_target(rois, inds, xy, po, gpo, M)
    g = np.random.default_rng(w)
    pred = g.normal(0, 1.5, (rois.shape[0], M, M)).astype(np.float32)
    labels = np.zeros(rois.shape[0], np.int64)
    want, info = R.mask_iou_target(rois, inds, xy, po, gpo, pred[:, None], labels, targets, shapes, 0.0)
    got = T.mask_iou_target(_cuda(rois), _cuda(inds), *[t.cuda() for t in cpu], _cuda(pred), _cuda(labels),
                            _cuda(targets), _cuda(shapes), thr=0.0).cpu().numpy()
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "rows %s (boxes %s) differ: got %s, want %s, inside %s of %s" % (
        bad.tolist(), rois[bad, 1:].tolist(), got[bad], want[bad], info["inside"][bad], info["full"][bad])
    assert info["full"][0] == R.instance_bitmap([np.array(plist[0][0][0], np.float32)], 5, w).sum() > 0
    assert len(set(info["inside"].tolist())) >= (2 if w == 1 else 4)


def test_mask_iou_target_wild_offsets_and_canvases(T, polys):
    """Offsets outside their arrays are clamped on the device and canvas sizes outside 0..8192 too: no fault, and equal
    to the oracle, which clamps the same way."""
    (xy, po, gpo), gpu = polys
    po2, gpo2 = po.copy(), gpo.copy()
    po2[2], po2[4] = -5, 1 << 30
    gpo2[1, 2], gpo2[0, 3] = 1 << 30, -3
    shapes = np.array([[360, -4], [1 << 20, 260]], np.int32)
    rois, inds, targets, pred, labels = K.target_case(7)
    want, _ = R.mask_iou_target(rois, inds, xy, po2, gpo2, pred, labels, targets, shapes, 0.5)
    got = T.mask_iou_target(_cuda(rois), _cuda(inds), gpu[0], _cuda(po2), _cuda(gpo2), _cuda(pred), _cuda(labels),
                            _cuda(targets), _cuda(shapes)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- mask_iou_stem -------------------------------------------------------------------------------------------------------
def _stem_inputs(S, C, seed, dtype, pred_dt, nhwc, off, three_d=False):
    feats, pred, labels, weight, bias, gy = K.stem_case(S, C, seed)
    labels = labels - off
    f = _cuda(feats).to(dtype).contiguous(memory_format=CL)
    x = _cuda(pred).to(pred_dt)
    x = x[:, 0].contiguous() if three_d else _layout(x, nhwc)
    g = _cuda(gy).to(dtype).contiguous(memory_format=CL)
    stored = dict(feats=f.float().cpu().numpy(), pred=x.float().cpu().numpy().reshape(pred.shape),
                  gy=g.float().cpu().numpy())
    return f, x, _cuda(labels), _cuda(weight), _cuda(bias), g, stored, labels, weight, bias


def run_stem(T, O, S, C, dtype, pred_dt, nhwc, off, what, three_d=False, seed=None):
    """The mask channel's launches under their bounds, then the whole layer against the float64 composition."""
    f, x, lab, w, b, g, st, labels, weight, bias = _stem_inputs(S, C, seed or (10 * S + C), dtype, pred_dt, nhwc, off,
                                                                three_d)
    Rr, Cf, Cout = f.shape[0], f.shape[1], w.shape[0]
    # the addend, P and the windows' indices
    a, P, idx = O.mask_iou_stem_fwd(x, lab, w, off, dtype)
    assert a.shape == (Rr, S, S, Cout) and a.dtype == dtype and P.dtype == torch.float32 and idx.dtype == torch.uint8
    gz = g.permute(0, 2, 3, 1)                               # the cotangent as it is behind a layer without ReLU
    ref = R.stem(st["feats"], st["pred"], labels, weight, bias, off, False, st["gy"])
    okr = ref["ok"]
    want_idx = np.where(ref["idx"] < 0, 255, ref["idx"])
    assert np.array_equal(idx.cpu().numpy(), want_idx), what + ": window indices"
    assert np.all(np.abs(_np64(P) - ref["P"]) <= 5 * U * ref["P"]), what + ": P"
    got_a = _np64(a).transpose(0, 3, 1, 2)
    err = np.abs(got_a - ref["a"])
    tol = K.K_A * U * ref["a_abs"] + _ulp16(ref["a"], dtype)
    unit = U * ref["a_abs"]
    worst_a = float((np.maximum(err - _ulp16(ref["a"], dtype), 0)[unit > 0] / unit[unit > 0]).max())
    assert np.all(err <= tol), "%s: a: %d elements beyond the bound" % (what, int((err > tol).sum()))
    assert not got_a[~okr].any() and not _np64(P)[~okr].any()
    # its two gradients
    dpred, dw1, dP = O.mask_iou_stem_bwd(gz, P, idx, x, lab, w, off)
    assert dpred.shape == x.shape and dpred.dtype == x.dtype and dpred.stride() == x.stride()
    got_d = _np64(dpred).reshape(st["pred"].shape)
    assert np.all(np.isfinite(got_d)), what
    assert not got_d[ref["dpred"] == 0].any(), what + ": dmask_pred is not an exact zero off the windows' maxima"
    err = np.abs(got_d - ref["dpred"])
    ulp = _ulp16(ref["dpred"], pred_dt)
    tol = K.K_DPRED(Cout) * U * ref["dpred_abs"] + ulp
    unit = U * ref["dpred_abs"]
    worst_d = float((np.maximum(err - ulp, 0)[unit > 0] / unit[unit > 0]).max())
    assert np.all(err <= tol), "%s: dmask_pred: %d elements beyond the bound, worst %.2f" % (
        what, int((err > tol).sum()), worst_d)
    got_w = _np64(dw1)
    want_w = ref["dweight"][:, Cf]
    err = np.abs(got_w - want_w)
    tol = K.K_DW1 * U * ref["dw1_abs"]
    worst_w = float((err[tol > 0] / (U * ref["dw1_abs"][tol > 0])).max())
    assert np.all(err <= tol), "%s: dw1: worst %.2f" % (what, worst_w)
    print("%s: worst error in units of 2^-24 of the bound's magnitude: a %.2f (K %d), dmask_pred %.2f (K %d), dw1 %.2f "
          "(K %d)" % (what, worst_a, K.K_A, worst_d, K.K_DPRED(Cout), worst_w, K.K_DW1))
    # the whole layer, twice (identical bits), against float64 with the conv path's 16-bit feature weights
    runs = []
    for _ in range(2):
        leaves = [f.detach().requires_grad_(True), x.detach().requires_grad_(True), w.detach().requires_grad_(True),
                  b.detach().requires_grad_(True)]
        y = T.mask_iou_stem(leaves[0], leaves[1], lab, leaves[2], leaves[3], label_offset=off, relu=True)
        runs.append([y] + list(torch.autograd.grad(y, leaves, g)))
    torch.cuda.synchronize()
    for u, v in zip(*runs):
        assert torch.equal(_bits(u), _bits(v)), what + ": run to run"
    y, df, dx, dw, db = runs[0]
    assert y.shape == (Rr, Cout, S, S) and y.dtype == dtype and y.permute(0, 2, 3, 1).is_contiguous()
    assert dx.shape == x.shape and dx.dtype == x.dtype and dx.stride() == x.stride()
    assert dw.shape == w.shape and dw.dtype == torch.float32 and df.shape == f.shape and df.dtype == dtype
    w_eff = weight.copy()
    w_eff[:, :Cf] = _cuda(weight[:, :Cf]).to(dtype).float().cpu().numpy()
    full = R.stem(st["feats"], st["pred"], labels, w_eff, bias, off, False)
    # in situ, as tests/parity_util.py compares a conv launch: on the launch's own operands (the conv launch reads the
    # STORED 16-bit addend, which is under its own bound above), the float64 value rounded to the output's type, and the
    # backward given the ReLU mask the GPU stored
    r16 = lambda v, dt: torch.from_numpy(v).to(dt).double() if dt != torch.float32 else torch.from_numpy(v)
    full["y"] = np.maximum(full["y"] - full["a"] + got_a, 0)
    gzt = st["gy"] * (y.detach().float().cpu().numpy() > 0)
    back = R.stem_backward(st["feats"], st["pred"], w_eff, full["P"], full["idx"], full["ch"], full["ok"], gzt)
    res = dict(y=rel_l2(y.float().cpu(), r16(full["y"], dtype)),
               dfeats=rel_l2(df.float().cpu(), r16(back["dfeats"], dtype)),
               dmask_pred=rel_l2(torch.from_numpy(_np64(dx).reshape(st["pred"].shape)), r16(back["dpred"], x.dtype)),
               dweight=rel_l2(dw.cpu(), torch.from_numpy(back["dweight"])),
               dbias=rel_l2(db.cpu(), torch.from_numpy(back["dbias"])))
    print("%s: whole layer, relative L2 against float64: %s" % (what, {k: "%.2e" % v for k, v in res.items()}))
    assert res["y"] <= parity_util.FWD_IN_SITU_TOL, res
    assert max(res["dfeats"], res["dmask_pred"], res["dweight"], res["dbias"]) <= parity_util.BWD_IN_SITU_TOL, res
    got_dx = _np64(dx).reshape(st["pred"].shape)
    assert not got_dx[back["dpred"] == 0].any() and np.all(np.isfinite(got_dx))
    return worst_a, worst_d, worst_w


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("S", [14, 2, 1])
def test_mask_iou_stem_vs_oracle(T, O, S, dt):
    d = DTYPES[dt]
    run_stem(T, O, S, 5, d, torch.float32, False, 0, "S%d %s pred f32 nchw" % (S, dt))
    run_stem(T, O, S, 5, d, d, True, 0, "S%d %s pred 16-bit nhwc" % (S, dt))
    run_stem(T, O, S, 5, d, d, True, 1, "S%d %s offset 1" % (S, dt))
    run_stem(T, O, S, 1, d, torch.float32, False, 0, "S%d %s C = 1" % (S, dt))
    run_stem(T, O, S, 1, d, d, False, 0, "S%d %s 3-D pred" % (S, dt), three_d=True)


def test_mask_iou_stem_wider_output(T, O):
    """Cout = 128, Cf = 128: two channels per lane in dP, two chunks in dw1; R = 70 rows give more pixels than one
    workgroup of the backward launch takes."""
    Rr, S, C, Cf, Cout = 70, 4, 3, 128, 128
    feats, pred, labels, weight, bias, gy = K.stem_case(S, C, 77, R=Rr, Cf=Cf, Cout=Cout)
    x, lab, w = _cuda(pred), _cuda(labels), _cuda(weight)
    a, P, idx = O.mask_iou_stem_fwd(x, lab, w, 0, torch.bfloat16)
    gz = _cuda(gy).to(torch.bfloat16).permute(0, 2, 3, 1).contiguous()
    dpred, dw1, _ = O.mask_iou_stem_bwd(gz, P, idx, x, lab, w, 0)
    ref = R.stem(feats, pred, labels, weight, bias, 0, False, gz.float().cpu().numpy().transpose(0, 3, 1, 2))
    assert np.all(np.abs(_np64(a).transpose(0, 3, 1, 2) - ref["a"]) <= K.K_A * U * ref["a_abs"] + _ulp16(ref["a"], torch.bfloat16))
    assert np.all(np.abs(_np64(dpred) - ref["dpred"]) <= K.K_DPRED(Cout) * U * ref["dpred_abs"])
    assert np.all(np.abs(_np64(dw1) - ref["dweight"][:, Cf]) <= K.K_DW1 * U * ref["dw1_abs"])


def test_mask_iou_stem_graph_replay_and_repack(T):
    """Forward + backward captured once: the replay equals eager bit for bit, and after the weight is updated in place
    the replay computes with the updated weight (the packed copy is re-derived inside the graph)."""
    f, x, lab, w0, b, g, _, _, _, _ = _stem_inputs(4, 5, 3, torch.bfloat16, torch.bfloat16, True, 0)
    holder = torch.nn.Module()
    holder.weight = torch.nn.Parameter(w0)
    w = holder.weight
    leaves = [f.requires_grad_(True), x.requires_grad_(True), w, b.requires_grad_(True)]

    def step():
        y = T.mask_iou_stem(leaves[0], leaves[1], lab, leaves[2], leaves[3])
        return [y.detach()] + list(torch.autograd.grad(y, leaves, g))

    captured, graph = _replay(step)
    for u, v in zip(captured, step()):
        assert torch.equal(_bits(u), _bits(v))
    before = captured[0].clone()
    with torch.no_grad():
        w.mul_(0.5)
    graph.replay()
    eager = step()
    torch.cuda.synchronize()
    for u, v in zip(captured, eager):
        assert torch.equal(_bits(u), _bits(v))
    assert not torch.equal(before, captured[0])
    # an update that bypasses the version counter is not seen until invalidate_packed
    w.data.mul_(2.0)
    stale = step()[0]
    assert not torch.equal(_bits(stale), _bits(before))
    T.invalidate_packed(holder)
    assert torch.equal(_bits(step()[0]), _bits(before))


# ---- mask_iou_loss ---------------------------------------------------------------------------------------------------------
def run_loss(T, case, dtype, what, lw=0.5):
    pred, labels, targets = case
    g = 32768.0 if dtype == torch.float16 else 1.5          # an fp16 loss scale arrives as the cotangent
    x = _cuda(pred).to(dtype)
    tg = [_cuda(labels), _cuda(targets)]
    gt = torch.tensor([g], dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):
        leaf = x.detach().requires_grad_(True)
        loss = T.mask_iou_loss(leaf, *tg, loss_weight=lw)
        runs.append((loss, torch.autograd.grad(loss, [leaf], gt)[0]))
    torch.cuda.synchronize()
    (loss, grad), (loss2, grad2) = runs
    assert loss.shape == (1,) and loss.dtype == torch.float32
    assert grad.shape == x.shape and grad.dtype == dtype and grad.is_contiguous()
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(grad), _bits(grad2)), what + ": run to run"
    ref = R.mask_iou_loss(x.float().cpu().numpy(), labels, targets, lw, g=g)
    got = _np64(grad)
    assert np.all(np.isfinite(got)), what
    assert not got[ref["dpred"] == 0].any(), what + ": not an exact zero off the live rows' columns"
    unit = U * ref["unit"][:, None] * np.ones_like(got)
    err = np.abs(got - ref["dpred"])
    live = unit > 0
    ulp = _ulp16(ref["dpred"], dtype)
    worst = float((np.maximum(err - ulp, 0)[live] / unit[live]).max()) if live.any() else 0.0
    tol = K.K_IOU_GRAD * unit + ulp
    lerr = abs(float(loss.item()) - ref["loss"])
    lworst = lerr / (U * ref["loss"]) if ref["loss"] > 0 else 0.0
    print("%s: loss %r (ref %r), D %d, loss error %.2f, worst gradient error %.2f (x 2^-24 of the magnitude)" % (
        what, float(loss.item()), ref["loss"], ref["D"], lworst, worst))
    assert np.all(err <= tol), "%s: %d gradient elements beyond the bound, worst %.2f" % (what, int((err > tol).sum()),
                                                                                      worst)
    ltol = K.K_IOU_LOSS * U * ref["loss"] + float(np.spacing(np.float32(abs(ref["loss"]))))
    assert lerr <= ltol, "%s: loss %r, ref %r, error %g > %g" % (what, float(loss.item()), ref["loss"], lerr, ltol)
    return ref, loss, grad


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_mask_iou_loss_vs_oracle(T, dt):
    for Rr, C in ((24, 5), (1, 2), (70000, 3), (300, 81)):
        case = K.loss_case(Rr, C, 7 * Rr + C)
        run_loss(T, case, DTYPES[dt], "R%d C%d %s" % (Rr, C, dt))
    run_loss(T, K.loss_case(24, 5, 2), DTYPES[dt], "loss_weight 1.25 %s" % dt, lw=1.25)


def test_mask_iou_loss_no_live_rows(T, O):
    for case in (K.loss_case(24, 5, 1, none_live=True), K.loss_case(5, 1, 2)):
        ref, loss, grad = run_loss(T, case, torch.float32, "no live rows")
        assert float(loss.item()) == 0.0 and not grad.any() and ref["D"] == 1
        loss, avg = O.mask_iou_loss_fwd(_cuda(case[0]), _cuda(case[1]), _cuda(case[2]), 0.5)
        assert loss.tolist() == [0.0] and avg.tolist() == [1.0]


# ---- mask_scores -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_mask_scores_bit_equal(T, dt):
    for C in (5, 1, 81):
        pred, dets, labels, counts = K.scores_case(C)
        x = _cuda(pred).to(DTYPES[dt])
        for cn in (counts, np.array([3, 6, 1], np.int32)):
            want = R.mask_scores(x.float().cpu().numpy(), dets, labels, cn)
            got = T.mask_scores(x, _cuda(dets), _cuda(labels), _cuda(cn))
            assert got.shape == (3, 6) and got.dtype == torch.float32
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (C, cn)
        assert not got[2, 1:].any() and (C == 1 or got[1, 4] != 0)


def test_target_loss_scores_graph_replay(T, polys):
    """mask_iou_target -> mask_iou_loss (+ backward) and mask_scores captured once and replayed on new logits: the same
    bits as eager."""
    _, gpu = polys
    rois, inds, targets, pred, labels = K.target_case(28)
    x = _layout(_cuda(pred).to(torch.bfloat16), True)
    fixed = [_cuda(rois), _cuda(inds)] + gpu
    rest = [_cuda(labels), _cuda(targets), _cuda(K.CANVASES)]
    iou_pred = torch.randn(40, 5, device="cuda").requires_grad_(True)
    sp, sd, sl, sc = (_cuda(a) for a in K.scores_case(5))

    def step():
        t = T.mask_iou_target(*fixed, x, *rest)
        loss = T.mask_iou_loss(iou_pred, rest[0], t)
        return [t, loss, torch.autograd.grad(loss, [iou_pred])[0], T.mask_scores(sp, sd, sl, sc)]

    captured, graph = _replay(step)
    first = [c.clone() for c in captured]
    for u, v in zip(captured, step()):
        assert torch.equal(_bits(u), _bits(v))
    with torch.no_grad():
        x.copy_(torch.where(torch.isnan(x), x, -x))
    graph.replay()
    eager = step()
    torch.cuda.synchronize()
    for u, v in zip(captured, eager):
        assert torch.equal(_bits(u), _bits(v))
    assert not torch.equal(first[0], captured[0]) and float(captured[1].detach()) > 0


# ---- MaskIoUHead -----------------------------------------------------------------------------------------------------------
class _RefHead(torch.nn.Module):
    """The head in plain torch, float64: what mmdetection v1's MaskIoUHead computes."""

    def __init__(self, head):
        super().__init__()
        import copy
        self.convs, self.fcs, self.fc_mask_iou = (copy.deepcopy(m).cpu().double() for m in
                                                  (head.convs, head.fcs, head.fc_mask_iou))

    def forward(self, feat, pred, labels):
        p = torch.sigmoid(pred[torch.arange(pred.shape[0]), labels])[:, None]
        x = torch.cat([feat, TF.max_pool2d(p, 2, 2)], 1)
        for conv in self.convs:
            x = torch.relu(conv(x))
        x = x.reshape(x.shape[0], -1)
        for fc in self.fcs:
            x = torch.relu(fc(x))
        return self.fc_mask_iou(x)


def _small_iou_head(T, seed=5):
    torch.manual_seed(seed)
    head = T.MaskIoUHead(num_convs=2, roi_feat_size=4, in_channels=64, conv_out_channels=64, fc_out_channels=64,
                         num_classes=5).cuda()
    with torch.no_grad():                                   # biases away from 0, an output of visible size
        for p in head.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
        head.fc_mask_iou.weight.mul_(20)
    return head


def _head_inputs(dtype, Rr=9, S=4, C=5, seed=21):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(Rr, 64, S, S, generator=g).cuda().to(dtype).contiguous(memory_format=CL)
    pred = (2 * torch.randn(Rr, C, 2 * S, 2 * S, generator=g)).cuda().to(dtype).contiguous(memory_format=CL)
    labels = (torch.arange(Rr) % (C - 1) + 1).cuda()
    gout = torch.randn(Rr, C, generator=g).cuda()
    return feat, pred, labels, gout


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_mask_iou_head_vs_float64_module(T, dt):
    dtype = DTYPES[dt]
    head = _small_iou_head(T)
    feat, pred, labels, gout = _head_inputs(dtype)
    f, x = feat.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    out = head(f, x, labels)
    assert out.shape == (9, 5) and out.dtype == torch.float32
    out.backward(gout)
    got = [out.detach(), f.grad, x.grad] + [p.grad for p in head.parameters()]
    assert x.grad.shape == x.shape and x.grad.dtype == dtype and x.grad.stride() == x.stride()
    ref = _RefHead(head)
    rf, rx = feat.double().cpu().requires_grad_(True), pred.double().cpu().requires_grad_(True)
    ro = ref(rf, rx, labels.cpu())
    ro.backward(gout.double().cpu())
    want = [ro.detach(), rf.grad, rx.grad] + [p.grad for p in ref.parameters()]
    names = ["out", "dfeat", "dmask_pred"] + [n for n, _ in head.named_parameters()]
    assert [n for n, _ in ref.named_parameters()] == names[3:]
    errs = {n: rel_l2(a.float().cpu(), b) for n, a, b in zip(names, got, want)}
    print("MaskIoUHead %s against the float64 module, relative L2: %s" % (dt, {k: "%.2e" % v for k, v in errs.items()}))
    assert errs["out"] <= parity_util.FWD_END_TO_END_TOL, errs
    assert max(errs.values()) <= parity_util.BWD_TEACHER_TOL, errs
    # exact zeros off the rows' channels
    off = torch.ones_like(x.grad, dtype=torch.bool)
    off[torch.arange(9, device="cuda"), labels] = False
    assert not x.grad[off].any() and x.grad.any()
    # state dict round trip
    other = T.MaskIoUHead(num_convs=2, roi_feat_size=4, in_channels=64, conv_out_channels=64, fc_out_channels=64,
                          num_classes=5).cuda()
    other.load_state_dict(head.state_dict())
    with torch.no_grad():
        assert torch.equal(_bits(other(feat, pred, labels)), _bits(out))
    # test-time labels: 0-based with offset 1; and a second run has the same bits
    with torch.no_grad():
        assert torch.equal(_bits(head(feat, pred, labels - 1, label_offset=1)), _bits(out))


def test_mask_iou_head_sgd_step_inside_a_graph(T):
    """forward -> loss -> backward -> SGD.step captured as one graph: the replay is the second training step, bit for
    bit what two eager steps give (the packed weights, the first layer's included, are re-derived inside the graph)."""
    def trainer():
        head = _small_iou_head(T)
        feat, pred, labels, _ = _head_inputs(torch.bfloat16)
        targets = torch.linspace(0.0, 0.9, 9, device="cuda")
        params = list(head.parameters())
        for p in params:
            p.grad = torch.zeros_like(p)
        opt = T.SGD(params, lr=0.05, momentum=0.9, weight_decay=1e-4, modules=[head])

        def step():
            out = head(feat, pred, labels)
            loss = head.loss(out, labels, targets)["loss_mask_iou"]
            grads = torch.autograd.grad(loss, params)
            with torch.no_grad():
                for p, gp in zip(params, grads):
                    p.grad.copy_(gp)
            opt.step()
            return [out, loss] + list(grads)

        return params, step

    params, step = trainer()
    first = [t.clone() for t in step()]
    second = [t.clone() for t in step()]
    torch.cuda.synchronize()
    want = [p.detach().clone() for p in params]
    params, step = trainer()
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, c) in enumerate(zip(captured, second)):
        assert torch.equal(_bits(a), _bits(c)), k
    for a, c in zip(params, want):
        assert torch.equal(_bits(a), _bits(c))
    assert not torch.equal(first[0], second[0])              # the second step saw updated weights


# ---- the chain -----------------------------------------------------------------------------------------------------------
def test_chain_mask_loss_and_mask_iou_loss_share_mask_pred(T):
    """sample_rois -> roi_align -> FCNMaskHead -> mask_target -> mask_head_loss, and beside it MaskIoUHead -> get_target ->
    loss; one backward: the gradient of mask_pred is the sum of the two nodes' gradients taken alone, rounded once."""
    import test_gpu_deconv as TD
    sample_in, pg, feats = TD._problem(T)
    mask_head = TD._small_head(T, seed=7)
    torch.manual_seed(11)
    iou_head = T.MaskIoUHead(num_convs=2, roi_feat_size=14, in_channels=64, conv_out_channels=64, fc_out_channels=64,
                             num_classes=5).cuda()
    with torch.no_grad():
        iou_head.fc_mask_iou.weight.mul_(20)
    shapes = torch.tensor([[256, 256], [256, 256]], dtype=torch.int32, device="cuda")
    num, npos = 32, 8
    out = T.sample_rois(*sample_in, num=num, pos_fraction=npos / num, seed=3)
    rois = out[0].view(2, num, 5)[:, :npos].reshape(-1, 5)
    labels = out[1].view(2, num)[:, :npos].reshape(-1)
    inds = out[5].view(2, num)[:, :npos].reshape(-1)
    targets, weights = T.mask_target(rois, inds, *pg, mask_size=28)
    x = T.roi_align(feats, rois, out_size=14, featmap_strides=(4, 8, 16, 32))
    pred = mask_head(x)
    loss_mask = T.mask_head_loss(pred, targets, labels, weights)
    iou_pred = iou_head(x, pred, labels)
    iou_t = iou_head.get_target(rois, inds, *pg, pred.detach(), labels, targets, shapes, thr=0.0)
    loss_iou = iou_head.loss(iou_pred, labels, iou_t)["loss_mask_iou"]
    g1 = torch.autograd.grad(loss_mask, pred, retain_graph=True)[0]
    g2 = torch.autograd.grad(loss_iou, pred, retain_graph=True)[0]
    params = list(mask_head.parameters()) + list(iou_head.parameters())
    pred.retain_grad()                                      # from here on: the two calls above must not add to it
    (loss_mask + loss_iou).backward()
    torch.cuda.synchronize()
    assert int((iou_t > 0).sum()) >= 4 and float(iou_t.max()) <= 1 and float(loss_iou.detach()) > 0
    assert g2.any() and g1.any() and g2.dtype == pred.dtype and g2.stride() == pred.stride()
    both = (g1.float() + g2.float())
    want = both.to(pred.dtype).float()
    err = (pred.grad.float() - want).abs().cpu().numpy().astype(np.float64)
    ulp = _ulp16(both.cpu().numpy().astype(np.float64), pred.dtype)
    assert np.all(err <= ulp), "the gradient of mask_pred is more than one 16-bit rounding from the sum: %g" % err.max()
    for t in [pred.grad, loss_mask, loss_iou, iou_pred] + [p.grad for p in params] + [f.grad for f in feats]:
        assert t is not None and torch.isfinite(t.float()).all()
    assert all(p.grad.abs().sum() > 0 for p in iou_head.parameters())
    # test time: the head's output scales the detections' scores
    with torch.no_grad():
        dets = torch.tensor([[[30, 40, 120, 140, 0.9], [130, 20, 230, 100, 0.8]]], device="cuda")
        cnt = torch.tensor([2], dtype=torch.int32, device="cuda")
        lab0 = torch.tensor([[0, 2]], device="cuda")
        r2 = T.rois_from_detections(dets, cnt)
        x2 = T.roi_align([f.detach()[:1] for f in feats], r2, out_size=14, featmap_strides=(4, 8, 16, 32))
        p2 = mask_head(x2)
        s = iou_head.get_mask_scores(iou_head(x2, p2, lab0.view(-1), label_offset=1), dets, lab0, cnt)
    assert s.shape == (1, 2) and torch.isfinite(s).all() and s.any()


# ---- under the guard ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import mask_iou_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, mask_iou_ops, g)
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
def test_guarded_mask_iou_target(T, guard, polys, M):
    _check_target(T, polys, M, 5, "f32", False)
    _check_target(T, polys, M, 5, "bf16", True)
    _check_target(T, polys, M, 1, "f16", False, three_d=True)
    assert guard.calls["mask_iou_target"] == 3
    _clean(guard, ["mask_iou_target"])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_guarded_mask_iou_stem(T, O, guard, dt):
    d = DTYPES[dt]
    for S in (14, 2, 1):
        run_stem(T, O, S, 5, d, torch.float32, False, 0, "guarded S%d %s" % (S, dt))
        _clean(guard, ["mask_iou_stem_fwd", "mask_iou_stem_bwd"])
        run_stem(T, O, S, 5, d, d, True, 1, "guarded S%d %s nhwc" % (S, dt))
        _clean(guard, [])
    run_stem(T, O, 3, 1, d, d, False, 0, "guarded 3-D %s" % dt, three_d=True)
    _clean(guard, [])
    test_mask_iou_stem_wider_output(T, O)
    _clean(guard, [])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_guarded_mask_iou_loss(T, guard, dt):
    for Rr, C in ((24, 5), (1, 2), (70000, 3)):
        run_loss(T, K.loss_case(Rr, C, 9 * Rr + C), DTYPES[dt], "guarded R%d C%d %s" % (Rr, C, dt))
        _clean(guard, ["mask_iou_loss_fwd", "mask_iou_loss_bwd"])


def test_guarded_mask_iou_loss_no_rows(O, guard):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    loss, avg = O.mask_iou_loss_fwd(z(0, 5), z(0, dt=torch.int64), z(0), 0.5)
    grad = O.mask_iou_loss_bwd(z(0, 5), z(0, dt=torch.int64), z(0), 0.5, z(1) + 1, avg)
    _clean(guard, [])
    assert loss.tolist() == [0.0] and avg.tolist() == [1.0] and grad.shape == (0, 5)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_guarded_mask_scores(T, guard, dt):
    test_mask_scores_bit_equal(T, dt)
    _clean(guard, ["mask_scores"])


def test_value_errors_on_mixed_devices(T, polys):
    _, gpu = polys
    rois, inds, targets, pred, labels = (_cuda(a) for a in K.target_case(7))
    with pytest.raises(ValueError, match="labels must be a CUDA tensor"):
        T.mask_iou_target(rois, inds, *gpu, pred, labels.cpu(), targets, _cuda(K.CANVASES))
    with pytest.raises(ValueError, match="dets must be a CUDA tensor"):
        p, d, l, c = (_cuda(a) for a in K.scores_case(5))
        T.mask_scores(p, d.cpu(), l, c)
    with pytest.raises(ValueError, match="mask_iou_targets must be a CUDA tensor"):
        p, l, t = (_cuda(a) for a in K.loss_case(24, 5, 1))
        T.mask_iou_loss(p, l, t.cpu())


def test_every_mask_iou_entry_point_ran_under_the_guard():
    """Counts what the guarded tests above did IN THIS RUN (run the file as a whole): every public wrapper of
    mask_iou_ops.py returned under the guard, and the workspace queries were answered at their exact size (rounded up
    only to the 256-byte alignment the header asks for)."""
    from torch_detection_amd import mask_iou_ops
    public = sorted(n for n, v in vars(mask_iou_ops).items()
                    if inspect.isfunction(v) and v.__module__ == mask_iou_ops.__name__ and not n.startswith("_"))
    assert public == ["mask_iou_loss_bwd", "mask_iou_loss_fwd", "mask_iou_stem_bwd", "mask_iou_stem_fwd",
                      "mask_iou_target", "mask_scores"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in ("mask_iou_loss_fwd", "mask_iou_stem_bwd"):
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)
