"""GPU tests of the FCOS operations (fcos_points, fcos_target, fcos_loss, fcos_detections) against the CPU
oracle tests/fcos_ref.py.

Points and targets: every output bit for bit.  Loss: losses and gradients against the float64 oracle under the a-priori
bounds of §4n (fcos_ref computes them per element, margin included; + the output's final rounding: spacing(ref) for the
fp32 losses, one ulp16 of ref for a 16-bit gradient), gradients exactly 0 wherever the oracle's are, NaN / Inf on every
element that is never read, two runs bit-identical.  Detections: batch_idx, point_idx and the selection exactly (the
oracle's float64 keys are asserted to lie further apart than the fp32 keys can err), dense scores within (33 + |a| + |c|)
u p + 2^-149 (two sigmoids of §4l's (16 + |x|) u and one product), dense boxes within ((16 + |s x|) u d + spacing(x + d))
/ scale + spacing(ref); every final output bit-equal to the oracle's selection run on the GPU's own dense values, and to
multiclass_nms on them.  Then the chain, graph capture, and every wrapper under the guard of tests/guard_util.py.

Every case asserts on the ORACLE's result that it is not hollow; the last test of the file counts what ran IN THIS RUN
(run the file as a whole).
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import fcos_cases as K
import fcos_ref as F
import guard_util as G

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24
THR, NMS_THR = 0.05, 0.5
ENTERED, WS_SEEN = set(), {}                  # what ran under the guard in this run
SEEN = {"over": 0, "under": 0, "cut": 0}
MANT = {torch.float16: 10, torch.bfloat16: 7}


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


# ---- points and targets -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [K.LEVELS, K.BIG], ids=["small", "big"])
def test_fcos_points(T, levels):
    got = T.fcos_points(K.sizes(levels), K.strides(levels))
    _same([got], [F.points(K.sizes(levels), K.strides(levels))], ["points"], "fcos_points")


TARGET_CASES = {
    # name: (levels, ranges, B, G, counts, radius, labels, seed, extent)
    "b3_g7": (K.LEVELS, K.RANGES, 3, 7, (7, 0, 5), None, True, 4, (64, 96)),
    "b3_g7_centre": (K.LEVELS, K.RANGES, 3, 7, (7, 4, 9), 1.5, True, 5, (64, 96)),
    "b1_g1_nolabels": (K.LEVELS, K.RANGES, 1, 1, (1,), None, False, 6, (64, 96)),
    "b3_g0": (K.LEVELS, K.RANGES, 3, 0, (0, 0, 0), None, False, 7, (64, 96)),
    "big_b3_g7": (K.BIG, K.BIG_RANGES, 3, 7, (7, 7, 0), None, True, 8, (768, 768)),
    "big_b1_g7_centre": (K.BIG, K.BIG_RANGES, 1, 7, (6,), 2.5, True, 9, (768, 768)),
}
TARGET_NAMES = ["labels", "bbox_targets", "assigned_gt_inds", "num_pos"]


def run_target(T, name):
    levels, ranges, Bn, Gn, counts, radius, with_labels, seed, extent = TARGET_CASES[name]
    gt, gl, cn = K.gt_case(Bn, Gn, counts, seed, extent)
    gl = gl if with_labels else None
    info = {}
    ref = F.target(K.sizes(levels), K.strides(levels), ranges, gt, gl, cn, radius, info)
    if Gn >= 1:
        assert info["edge"] >= 1 and ref[3].sum() > 0, info
    if Gn >= 4:
        assert info["ties"] >= 1, info
    got = T.fcos_target(K.sizes(levels), K.strides(levels), ranges, _cuda(gt), _cuda(gl), _cuda(cn), radius)
    _same(got, ref, TARGET_NAMES, name)
    again = T.fcos_target(K.sizes(levels), K.strides(levels), ranges, _cuda(gt), _cuda(gl), _cuda(cn), radius)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    return ref


@pytest.mark.parametrize("name", sorted(TARGET_CASES))
def test_fcos_target(T, name):
    ref = run_target(T, name)
    counts = TARGET_CASES[name][4]
    for b, n in enumerate(counts):
        if n == 0:
            assert ref[3][b] == 0 and not ref[0][b].any()


# ---- loss -----------------------------------------------------------------------------------------------------------------
def _ulp16(ref, dtype):
    """Spacing of the 16-bit type at |ref| (its smallest subnormal below the normal range); 0 for float32."""
    if dtype == torch.float32:
        return np.zeros_like(ref)
    emin = -14 if dtype == torch.float16 else -126
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref), where=ref != 0, out=np.full(ref.shape, float(emin))))
    return 2.0 ** (np.maximum(e, emin) - MANT[dtype])


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _check_grad(got, ref, bound, dtype, what):
    got = _np64(got)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), what
    assert not got[ref == 0].any(), "%s: %d elements must be exactly 0" % (what, int((got[ref == 0] != 0).sum()))
    tol = bound + _ulp16(ref, dtype)
    err = np.abs(got - ref)
    live = bound > 0
    worst = float((err[live] / tol[live]).max()) if live.any() else 0.0          # of the tolerance, final rounding included
    assert np.all(err <= tol), "%s: %d beyond the bound, worst %.3f x the bound" % (what, int((err > tol).sum()), worst)
    return worst


LOSS_CASES = {
    # name: (levels, ranges, B, C, dtype, layout, loss_type, scales, eps, extent, seed)
    "c5_b3_f32_nchw_iou": (K.LEVELS, K.RANGES, 3, 5, "f32", "nchw", "iou", False, 1e-3, (64, 96), 1),
    "c80_b1_bf16_nhwc_giou_scales": (K.LEVELS, K.RANGES, 1, 80, "bf16", "nhwc", "giou", True, 1e-6, (64, 96), 2),
    "c1_b3_f16_mixed_iou_scales": (K.LEVELS, K.RANGES, 3, 1, "f16", "mixed", "iou", True, 1e-3, (64, 96), 3),
    "c5_b3_bf16_mixed_giou": (K.LEVELS, K.RANGES, 3, 5, "bf16", "mixed", "giou", False, 1e-6, (64, 96), 4),
    "c5_b3_f16_nhwc_iou_default_eps": (K.LEVELS, K.RANGES, 3, 5, "f16", "nhwc", "iou", False, 1e-6, (64, 96), 5),
    "big_c5_b1_bf16_nhwc_iou_scales": (K.BIG, K.BIG_RANGES, 1, 5, "bf16", "nhwc", "iou", True, 1e-3, (768, 768), 6),
    "big_c20_b3_f32_nchw_giou_scales": (K.BIG, K.BIG_RANGES, 3, 20, "f32", "nchw", "giou", True, 1e-6, (768, 768), 7),
}
G3 = (1.5, 0.75, 2.0)


def loss_inputs(name, counts=None):
    levels, ranges, Bn, C, dt, lay, kind, with_scales, eps, extent, seed = LOSS_CASES[name]
    counts = counts if counts is not None else [7, 3, 5][:Bn]
    gt, gl, cn = K.gt_case(Bn, 7, counts, seed, extent)
    gl = np.minimum(gl, C)
    labels, bt, _, _ = F.target(K.sizes(levels), K.strides(levels), ranges, gt, gl, cn)
    arrs = K.loss_case(levels, Bn, C, labels, bt, seed + 100)
    heads = K.to_tensors(arrs, K.DTYPES[dt], lay)
    scales = (f32(1) + f32(0.125) * np.arange(len(levels), dtype=f32) - f32(0.25)) if with_scales else None
    return heads, labels, bt, scales, kind, eps


def run_loss(T, name, counts=None, targets_gpu=None):
    """forward + backward twice (bitwise equal), then everything against the oracle.  Returns the worst ratios."""
    heads, labels, bt, scales, kind, eps = loss_inputs(name, counts)
    dtype = heads[0][0].dtype
    stored = [[t.float().numpy() for t in hs] for hs in heads]
    ref = F.loss(stored[0], stored[1], stored[2], labels, bt, scales, kind, 2.0, 0.25, eps, G3)
    if counts is None:
        assert ref["num_pos"] >= 10
        pos_r = np.concatenate([F.rows(a) for a in stored[1]], 1)[labels > 0]
        assert (np.exp(pos_r.astype(np.float64)) == bt[labels > 0]).sum() >= 1, "a min / max tie"
        if eps == 1e-3:
            assert (ref["iou"] < eps).sum() >= 2 and np.abs(ref["iou"] / eps - 1).min() > 1e-3
        else:
            assert (ref["iou"] < eps).sum() == 0
    lab_t, bt_t = targets_gpu or (_cuda(labels), _cuda(bt))
    gt = torch.tensor(G3, dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):
        leaves = [[t.cuda().requires_grad_() for t in hs] for hs in heads]
        for a, b in zip(sum(leaves, []), sum(heads, [])):
            assert a.stride() == b.stride()
        sc = None if scales is None else _cuda(scales).requires_grad_()
        losses = T.fcos_loss(leaves[0], leaves[1], leaves[2], lab_t, bt_t, sc, kind, 2.0, 0.25, eps)
        losses.backward(gt)
        runs.append((losses.detach(), [[t.grad for t in hs] for hs in leaves], None if sc is None else sc.grad))
    (l0, g0, s0), (l1, g1, s1) = runs
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    for a, b in zip(sum(g0, []), sum(g1, [])):
        assert a.dtype == dtype and torch.equal(_bytes(a), _bytes(b))
    worst = {}
    got = l0.cpu().numpy().astype(np.float64)
    assert l0.dtype == torch.float32 and l0.shape == (3,)
    for k in range(3):
        tol = ref["bound_losses"][k] + float(np.spacing(f32(abs(ref["losses"][k]))))
        err = abs(got[k] - ref["losses"][k])
        assert err <= tol, "%s: loss %d: got %r, ref %r, error %g > %g" % (name, k, got[k], ref["losses"][k], err, tol)
        worst["loss%d" % k] = err / ref["bound_losses"][k] if ref["bound_losses"][k] > 0 else 0.0
    for k, key in enumerate(("dcls", "dreg", "dctr")):
        for l in range(len(heads[0])):
            assert g0[k][l].stride() == heads[k][l].stride() and g0[k][l].shape == heads[k][l].shape
            w = _check_grad(g0[k][l], ref[key][l], ref["bound_" + key][l], dtype, "%s: %s[%d]" % (name, key, l))
            worst[key] = max(worst.get(key, 0.0), w)
    if scales is not None:
        assert s0.dtype == torch.float32 and s0.shape == (len(heads[0]),) and torch.equal(s0, s1)
        ds = s0.cpu().numpy().astype(np.float64)
        tol = ref["bound_dscale"] + np.spacing(np.abs(ref["dscale"]).astype(f32)).astype(np.float64)
        assert np.all(np.abs(ds - ref["dscale"]) <= tol), (name, ds, ref["dscale"], tol)
        assert not ds[ref["dscale"] == 0].any()
    print("%s: worst error / tolerance %s" % (name, {k: round(float(v), 3) for k, v in worst.items()}))
    return ref


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_fcos_loss(T, name):
    run_loss(T, name)


def test_fcos_loss_without_positives(T):
    """All three divisors: loss_cls / (0 + B), the other two exactly 0, every box and centre-ness gradient exactly 0."""
    ref = run_loss(T, "c5_b3_f32_nchw_iou", counts=[0, 0, 0])
    assert ref["num_pos"] == 0 and ref["losses"][0] > 0 and ref["losses"][1:].tolist() == [0, 0]
    ref = run_loss(T, "c1_b3_f16_mixed_iou_scales", counts=[0, 0, 0])
    assert ref["num_pos"] == 0 and not ref["dscale"].any()


# ---- detections -----------------------------------------------------------------------------------------------------------
DET_CASES = {
    # name: (levels, C, B, dtype, layout, nms_pre, max_per_img, scale, scales, extent, seed)
    "c5_b3_f32_nchw_pre50": (K.LEVELS, 5, 3, "f32", "nchw", 50, 100, "none", False, (64, 96), 21),
    "c80_b1_bf16_nhwc_pre95_top1": (K.LEVELS, 80, 1, "bf16", "nhwc", 95, 1, "number", True, (64, 96), 22),
    "c1_b3_f16_mixed_pre96": (K.LEVELS, 1, 3, "f16", "mixed", 96, 100, "tensor", True, (64, 96), 23),
    "c5_b3_bf16_nhwc_pre97": (K.LEVELS, 5, 3, "bf16", "nhwc", 97, 100, "none", True, (64, 96), 24),
    "c5_b1_bf16_nchw_pre0": (K.LEVELS, 5, 1, "bf16", "nchw", 0, 100, "number", False, (64, 96), 25),
    "c5_b3_f16_nhwc_pre4096": (K.LEVELS, 5, 3, "f16", "nhwc", 4096, 100, "none", False, (64, 96), 26),
    "c80_b3_bf16_mixed_pre50_top1": (K.LEVELS, 80, 3, "bf16", "mixed", 50, 1, "tensor", False, (64, 96), 27),
    "big_c5_b1_bf16_nhwc_pre1000": (K.BIG, 5, 1, "bf16", "nhwc", 1000, 100, "none", True, (768, 768), 28),
    "big_c5_b3_f32_nchw_pre4096": (K.BIG, 5, 3, "f32", "nchw", 4096, 100, "number", False, (768, 768), 29),
}
DET_NAMES = ["dets", "labels", "point_idx", "counts", "row_idx"]


def det_inputs(name):
    levels, C, Bn, dt, lay, nms_pre, top, scale, with_scales, extent, seed = DET_CASES[name]
    arrs = K.det_case(levels, Bn, C, seed)
    heads = K.to_tensors(arrs, K.DTYPES[dt], lay)
    scales = (f32(1) + f32(0.125) * np.arange(len(levels), dtype=f32) - f32(0.125)) if with_scales else None
    shapes = K.img_shapes(Bn, extent)
    sf = {"none": None, "number": 1.5, "tensor": np.linspace(0.75, 2.0, Bn).astype(f32)}[scale]
    return dict(heads=heads, scales=scales, shapes=shapes, sf=sf, strides=K.strides(levels), nms_pre=nms_pre, top=top,
                B=Bn, C=C, sizes=K.sizes(levels))


def run_det(T, name):
    c = det_inputs(name)
    Bn, C = c["B"], c["C"]
    stored = [[t.float().numpy() for t in hs] for hs in c["heads"]]
    info = {}
    d = F.dense(stored[0], stored[1], stored[2], c["strides"], c["shapes"], c["scales"], c["sf"], c["nms_pre"], info)
    # the fp32 order of the keys is decided: distinct float64 keys lie further apart than twice the score bound
    for keys, mag in info["keys"]:
        o = np.argsort(keys)
        k, m = keys[o], mag[o]
        gap = np.diff(k) / k[1:]
        assert np.all(gap[gap > 0] > 2 * (33 + np.maximum(m[1:], m[:-1])[gap > 0]) * U)
    cuts = info.get("cuts", [])
    if cuts:                                      # a case that selects: some cut has keys above it and splits its ties
        assert any(q["above"] > 0 and q["ties"] > q["taken"] for q in cuts), cuts
        SEEN["cut"] += 1
    sf = _cuda(c["sf"]) if isinstance(c["sf"], np.ndarray) else c["sf"]
    args = ([t.cuda() for t in c["heads"][0]], [t.cuda() for t in c["heads"][1]], [t.cuda() for t in c["heads"][2]],
            c["strides"], _cuda(c["shapes"]))
    kw = dict(scales=_cuda(c["scales"]), scale_factors=sf, nms_pre=c["nms_pre"], score_thr=THR, nms_thr=NMS_THR,
              max_per_img=c["top"])
    out = T.fcos_detections(*args, return_dense=True, **kw)
    dets, labels, pidx, counts, sc, bx, bidx, dpidx, rows = [t.cpu().numpy() for t in out]
    # 1. the selection of step 2 is exact
    _same([bidx, dpidx], [d["batch_idx"], d["point_idx"]], ["batch_idx", "dense_point_idx"], name)
    # 2. dense scores and boxes within their bounds
    assert sc.dtype == f32 and sc.shape == d["scores"].shape and not sc[:, 0].any()
    p64 = d["scores"][:, 1:]
    tol = (33 + np.abs(d["cls"]) + np.abs(d["ctr"])[:, None]) * U * p64 + 2.0 ** -149
    err = np.abs(sc[:, 1:].astype(np.float64) - p64)
    assert np.all(err <= tol), "%s: %d scores beyond the bound, worst %.2f" % (name, (err > tol).sum(), (err / tol).max())
    far = d["centre"] + d["dist"]
    tol = ((16 + np.abs(d["sx"])) * U * d["dist"] + np.spacing(far.astype(f32))) / d["scale"][:, None] + \
        np.spacing(np.abs(d["boxes"]).astype(f32))
    err = np.abs(bx.astype(np.float64) - d["boxes"])
    assert np.all(err <= tol), "%s: %d boxes beyond the bound, worst %.2f" % (name, (err > tol).sum(), (err / tol).max())
    # 3. every final output equals the oracle's selection on the GPU's own dense values
    st = {}
    ref = F.select(bx, sc, bidx, dpidx, Bn, THR, NMS_THR, c["top"], st)
    _same([dets, labels, pidx, counts, rows], ref, DET_NAMES, name)
    assert counts.min() >= 1
    SEEN["over"] += any(t > c["top"] for t in st["total"])
    SEEN["under"] += any(0 <= t < c["top"] for t in st["total"])
    # 4. the selection does not depend on return_dense, and multiclass_nms on the dense tensors reproduces it
    plain = T.fcos_detections(*args, **kw)
    assert len(plain) == 4
    for a, b in zip(plain, out[:4]):
        assert torch.equal(a, b)
    mc = T.multiclass_nms(out[5], out[4], out[6], Bn, THR, NMS_THR, c["top"])
    for a, b in zip(mc, (out[0], out[1], out[8], out[3])):
        assert torch.equal(a, b)
    return out, c, args, kw


@pytest.mark.parametrize("name", sorted(DET_CASES))
def test_fcos_detections(T, name):
    run_det(T, name)


def test_launch_count_matches_the_plan(T):
    """The launches the library records for one call == what the host-only plan query announces."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    for name in ("c5_b3_f32_nchw_pre50", "c5_b1_bf16_nchw_pre0"):
        c = det_inputs(name)
        p = T.fcos_detections_plan(c["sizes"], c["B"], c["C"], c["nms_pre"])
        args = ([t.cuda() for t in c["heads"][0]], [t.cuda() for t in c["heads"][1]], [t.cuda() for t in c["heads"][2]],
                c["strides"], _cuda(c["shapes"]))
        assert lib.tdn_plan_begin() == 0
        try:
            out = T.fcos_detections(*args, nms_pre=c["nms_pre"], max_per_img=c["top"], return_dense=True)
        finally:
            plan = lib.tdn_plan_end()
        stats = (ctypes.c_int32 * 3)()
        assert plan and lib.tdn_plan_stats(plan, stats) == 0
        lib.tdn_plan_free(plan)
        assert stats[0] == p["launches"] == (7 if c["nms_pre"] else 6), (name, list(stats), p)
        assert out[4].shape[0] == p["rows"]
    p = T.fcos_detections_plan(K.sizes(K.LEVELS), 3, 5, 50)
    assert p["kept"] == [50, 24, 6] and p["K"] == 80 and p["selecting"] == 1


# ---- the chain and graph capture --------------------------------------------------------------------------------------------
def _chain_inputs(seed, dtype=torch.bfloat16):
    levels, Bn, C = K.LEVELS, 2, 5
    gt, gl, cn = K.gt_case(Bn, 7, (7, 4), seed)
    arrs = K.det_case(levels, Bn, C, seed)
    heads = K.to_tensors(arrs, dtype, "mixed")
    shapes = torch.tensor([(64 - seed, 96), (60, 96 - 2 * seed)], dtype=torch.int32)
    return sum(heads, []) + [torch.from_numpy(gt), torch.from_numpy(gl), torch.from_numpy(cn), shapes]


def test_chain_eager_and_graph_replay(T):
    """fcos_target -> fcos_loss -> backward, and fcos_detections on the same tensors, captured once and replayed on new
    inputs: a host synchronisation or an allocation inside the library would break the capture.  Eager and replayed
    results agree bit for bit, and two replays differ."""
    sizes, strides = K.sizes(K.LEVELS), K.strides(K.LEVELS)
    bufs = [t.cuda() for t in _chain_inputs(1)]
    scales = torch.tensor([1.0, 0.875, 1.125], device="cuda")

    def step():
        leaves = [t.detach().requires_grad_() for t in bufs[:9]]
        sc = scales.detach().requires_grad_()
        tg = T.fcos_target(sizes, strides, K.RANGES, bufs[9], bufs[10], bufs[11], 1.5)
        losses = T.fcos_loss(leaves[0:3], leaves[3:6], leaves[6:9], tg[0], tg[1], sc, "giou")
        losses.sum().backward()
        det = T.fcos_detections(bufs[0:3], bufs[3:6], bufs[6:9], strides, bufs[12], scales, 1.5, nms_pre=50,
                                max_per_img=30, return_dense=True)
        return list(tg) + [losses.detach()] + [t.grad for t in leaves] + [sc.grad] + list(det)

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
            for dst, src in zip(bufs, _chain_inputs(seed)):
                assert dst.stride() == src.stride()
                dst.copy_(src)
        graph.replay()
        eager = step()
        torch.cuda.synchronize()
        assert int(eager[3].sum()) > 0 and int(eager[18].min()) >= 1        # num_pos; counts
        for a, b in zip(captured, eager):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))
        seen.append([captured[4].clone(), captured[5].clone(), captured[15].clone()])
    for x, y in zip(*seen):
        assert not torch.equal(x, y)


# ---- under the guard -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import fcos_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, fcos_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


def test_guarded_points(T, guard):
    test_fcos_points(T, K.BIG)
    _clean(guard, ["fcos_points"])


@pytest.mark.parametrize("name", ["b3_g7", "b3_g0", "big_b1_g7_centre"])
def test_guarded_targets(T, guard, name):
    run_target(T, name)
    _clean(guard, ["fcos_target"])


@pytest.mark.parametrize("name", ["c5_b3_f32_nchw_iou", "c80_b1_bf16_nhwc_giou_scales", "c1_b3_f16_mixed_iou_scales",
                                  "big_c5_b1_bf16_nhwc_iou_scales"])
def test_guarded_loss(T, guard, name):
    """Poisoned outputs and an exact-size workspace: every gradient element must have been WRITTEN."""
    run_loss(T, name)
    _clean(guard, ["fcos_loss_fwd", "fcos_loss_bwd"])


@pytest.mark.parametrize("name", ["c5_b3_f32_nchw_pre50", "c80_b1_bf16_nhwc_pre95_top1", "c5_b1_bf16_nchw_pre0",
                                  "big_c5_b1_bf16_nhwc_pre1000"])
def test_guarded_detections(T, guard, name):
    """Every dense element and every unused row must have been WRITTEN."""
    run_det(T, name)
    _clean(guard, ["fcos_detections"])


def test_guarded_plan(T, guard):
    assert T.fcos_detections_plan(K.sizes(K.BIG), 1, 5, 1000)["kept"] == [1000, 1]
    _clean(guard, ["fcos_detections_plan"])


def test_every_entry_point_ran_under_the_guard_and_both_sides_ran():
    """Counts what the tests above did IN THIS RUN (run the file as a whole)."""
    from torch_detection_amd import fcos_ops
    public = sorted(n for n, v in vars(fcos_ops).items()
                    if inspect.isfunction(v) and v.__module__ == fcos_ops.__name__ and not n.startswith("_"))
    assert public == ["fcos_detections", "fcos_detections_plan", "fcos_loss_bwd", "fcos_loss_fwd", "fcos_points",
                      "fcos_target"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in ("fcos_target", "fcos_loss_fwd", "fcos_detections"):
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)
    assert SEEN["over"] >= 1 and SEEN["under"] >= 1 and SEEN["cut"] >= 1, SEEN
