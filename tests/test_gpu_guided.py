"""GPU: the Guided Anchoring kernels (csrc/guided.hip) against tests/ga_ref.py.

Location targets and shape targets: every output bit for bit, two runs equal; with one approx per location the
assignment is bit-equal to assign_max_iou on the GPU.  Guided anchors: bit-equal to delta2bbox on the same values, within
§4b's decode bound of the oracle, the mask bit-exact with logits planted on the threshold and one fp32 step either side.
Loss: losses and every gradient within the oracle's a-priori per-element bounds (+ the output's final rounding:
spacing(ref) for the fp32 losses, one ulp16 of ref for a 16-bit gradient), gradients exactly 0 wherever the oracle's are,
NaN / Inf on every element that is never read, two runs bit-identical.  Guided RPN proposals: with shared anchors and a
full mask bit-equal to rpn_proposals; with per-image anchors and masks equal to the oracle's selection run on the GPU's
own decoded values, with a mask empty on one level and one empty everywhere.  Then the chain, graph capture, and every wrapper
under the guard of tests/guard_util.py.

Every case asserts on the ORACLE's result that it is not hollow; the last test of the file counts what ran IN THIS RUN
(run the file as a whole).
"""
import inspect

import numpy as np
import pytest
import torch

import ga_cases as K
import ga_ref as R
import guard_util as G

pytestmark = pytest.mark.gpu
f32 = np.float32
ENTERED, WS_SEEN = set(), {}                  # what ran under the guard in this run
SEEN = {"erased": 0, "cut": 0, "uncut": 0, "tie": 0, "clip": 0, "first": 0, "empty_level": 0, "empty_image": 0}
MANT = {torch.float16: 10, torch.bfloat16: 7}
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


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


def _twice(first, again):
    for a, b in zip(first, again):
        if torch.is_tensor(a):
            assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))
        else:
            assert a == b


# ---- location targets -----------------------------------------------------------------------------------------------------
LOC_CASES = {
    # name: (sizes, B, G, counts, seed, center_ratio, ignore_ratio)
    "b3_g9": (K.SMALL, 3, 9, (9, 0, 5), 1, 0.2, 0.5),
    "b1_g1": (K.SMALL, 1, 1, (1,), 2, 0.2, 0.5),
    "b2_g0": (K.SMALL, 2, 0, (0, 0), 3, 0.2, 0.5),
    "b2_g256": (K.SMALL, 2, K.MAX_GT, (K.MAX_GT, 100), 4, 0.2, 0.5),
    "b3_g9_ratios": (K.SMALL, 3, 9, (7, 9, 2), 5, 0.35, 0.8),
    "big_b3_g9": (K.BIG, 3, 9, (9, 0, 5), 6, 0.2, 0.5),
}


def run_loc(T, name):
    sizes, Bn, Gn, counts, seed, cr, ir = LOC_CASES[name]
    gt, cn = K.gt_case(Bn, Gn, counts, seed, sizes)
    info = {}
    ref = R.loc_target(sizes, K.STRIDES, K.ANCHOR_SCALE, gt, cn, cr, ir, info)
    if counts[0] >= 7:
        assert info["levels"] >= {0, len(sizes) - 1} and info["one_pixel"] >= 1 and info["clamped"] >= 1, info
        assert (cr, ir) != (0.2, 0.5) or info["erased_final"] >= 1, info     # the planted pair overlaps at these ratios
        SEEN["erased"] += info["erased_final"]
    args = (sizes, K.STRIDES, K.ANCHOR_SCALE, _cuda(gt), _cuda(cn), cr, ir)
    got = T.ga_loc_target(*args)
    _same(got[:2], ref[:2], ["loc_targets", "loc_weights"], name)
    assert got[2] == ref[2] and isinstance(got[2], float)
    _twice(got, T.ga_loc_target(*args))
    return ref


@pytest.mark.parametrize("name", sorted(LOC_CASES))
def test_ga_loc_target(T, name):
    ref = run_loc(T, name)
    for b, n in enumerate(LOC_CASES[name][3]):
        if n == 0:
            assert not ref[0][b].any() and np.all(ref[1][b] == f32(0.1))


# ---- shape targets --------------------------------------------------------------------------------------------------------
SHAPE_CASES = {
    # name: (sizes, A, B, G, counts, seed, per-image flags, border, gt_max_assign_all, sampling, num)
    "a9_b3": (K.SMALL, 9, 3, 7, (7, 0, 5), 1, True, 0, True, True, 16),
    "a9_b3_first": (K.SMALL, 9, 3, 7, (7, 0, 5), 2, False, 0, False, True, 8192),
    "a3_b2_noborder": (K.SMALL, 3, 2, 5, (5, 3), 3, True, -1, True, True, 24),
    "a1_b3_all": (K.SMALL, 1, 3, 7, (7, 0, 5), 4, False, 0, True, False, 256),
    "a9_b1_g1": (K.SMALL, 9, 1, 1, (1,), 5, False, 0, True, True, 256),
    "a3_b2_g0": (K.SMALL, 3, 2, 0, (0, 0), 6, True, 0, True, True, 64),
    "a9_b2_g256": (K.SMALL, 9, 2, K.MAX_GT, (K.MAX_GT, 40), 7, True, 0, True, True, 64),
    "big_a9_b3": (K.BIG, 9, 3, 7, (7, 0, 5), 8, True, 0, True, True, 48),
    "big_a3_b2_first_all": (K.BIG, 3, 2, 7, (7, 6), 9, False, -1, False, False, 256),
}
SHAPE_NAMES = ["bbox_anchors", "bbox_gts", "bbox_weights", "num_pos", "num_neg", "assigned_gt_inds", "max_overlaps"]


def run_shape(T, name):
    sizes, A, Bn, Gn, counts, seed, per_img, border, all_, sampling, num = SHAPE_CASES[name]
    c = K.shape_case(sizes, A, Bn, Gn, counts, seed, per_img)
    kw = dict(num=num, allowed_border=border, keys=c["keys"], gt_max_assign_all=all_, sampling=sampling)
    info = {}
    ref = R.shape_target(c["approxs"], c["squares"], c["flags"], c["gt"], c["counts"], c["img_shapes"], info=info, **kw)
    if Gn >= 5:
        assert info["single"] >= 1 and info["col_ties"] >= 1 and ref[3].sum() > 0, info
        assert A == 1 or info["approx_ties"] >= 1, info
        assert border < 0 or info["out"] > Bn, info
        assert border < 0 or info["single_inside"] >= 1, info   # every flag set, a single approx inside the image
    if sampling:
        SEEN["cut" if info["cut"] else "uncut"] += 1
    SEEN["first"] += int(not all_ and Gn > 0)
    kw["keys"] = _cuda(c["keys"])
    args = tuple(_cuda(c[k]) for k in ("approxs", "squares", "flags", "gt", "counts", "img_shapes"))
    got = T.ga_shape_target(*args, **kw)
    _same(got, ref, SHAPE_NAMES, name)
    _twice(got, T.ga_shape_target(*args, **kw))
    return c, got


@pytest.mark.parametrize("name", sorted(SHAPE_CASES))
def test_ga_shape_target(T, name):
    run_shape(T, name)


@pytest.mark.parametrize("all_", [True, False])
def test_one_approx_is_assign_max_iou(T, all_):
    """A = 1 and approxs == squares: the new assign passes give assign_max_iou's bits on the GPU."""
    c = K.shape_case(K.BIG, 1, 3, 7, (7, 0, 5), 11, True)
    ap, sq, gt, cn = (_cuda(c[k]) for k in ("approxs", "squares", "gt", "counts"))
    assert torch.equal(ap[:, 0], sq)
    for flags, fl1 in ((None, None), (_cuda(c["flags"]), _cuda(c["flags"]))):
        got = T.ga_shape_target(ap, sq, flags, gt, cn, None, allowed_border=-1, gt_max_assign_all=all_, sampling=False)
        a, m = T.assign_max_iou(sq, gt, cn, 0.7, 0.3, 0.3, all_, fl1)
        assert torch.equal(got[5], a) and torch.equal(got[6].view(torch.int32), m.view(torch.int32))
        assert int((a > 0).sum()) > 0


# ---- guided anchors -------------------------------------------------------------------------------------------------------
def _layout(arrs, dtype, layout):
    """float32 arrays -> CUDA tensors of ``dtype``; 'mixed': odd levels channels_last."""
    out = []
    for l, a in enumerate(arrs):
        t = torch.from_numpy(a).cuda().to(DT[dtype])
        if layout == "nhwc" or (layout == "mixed" and l % 2):
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t)
    return out


ANCHOR_CASES = {
    # name: (sizes, B, dtype, layout, threshold, seed)
    "b3_f32_nchw": (K.SMALL, 3, "f32", "nchw", 0.01, 1),
    "b2_bf16_mixed": (K.SMALL, 2, "bf16", "mixed", 0.3, 2),
    "b1_f16_nhwc_nomask": (K.SMALL, 1, "f16", "nhwc", None, 3),
    "big_b2_f32_mixed": (K.BIG, 2, "f32", "mixed", 0.7, 4),
}


def run_anchors(T, name):
    sizes, Bn, dtype, layout, thr, seed = ANCHOR_CASES[name]
    loc, shape = K.head_case(sizes, Bn, dtype, seed, scale=6.0)
    shape[0][0, 0, 0, :4] = K.stored([120, -120, 98.6, -98.7], dtype)          # beyond the clip on both sides
    sq = K.squares_of(sizes)
    if thr is not None:
        t = R.loc_threshold(thr)
        if dtype == "f32":                                  # on the threshold and one fp32 step either side
            loc[0][0, 0, 1, :3] = [t, np.nextafter(t, f32(np.inf)), np.nextafter(t, f32(-np.inf))]
        z = np.concatenate([R.rows(p) for p in loc], 1)[..., 0]
        near = np.abs(z.astype(np.float64) - float(t)) <= float(np.spacing(np.abs(t)))
        assert near.sum() == (3 if dtype == "f32" else 0)   # no other logit lies that close
    ref = R.guided_anchors(shape, sq, loc if thr is not None else None, thr)
    assert ref[1].any() and (thr is None or not ref[1].all())
    sh, lc = _layout(shape, dtype, layout), _layout(loc, dtype, layout)
    args = (sh, _cuda(sq), lc if thr is not None else None, thr)
    got = T.guided_anchors(*args)
    _same([got[1]], [ref[1]], ["loc_mask"], name)
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - ref[0])
    assert np.all(err <= ref[2]), "%s: worst %.2f of the decode bound" % (name, (err / ref[2]).max())
    flat = torch.cat([s.float().permute(0, 2, 3, 1).reshape(Bn, -1, 2) for s in sh], 1)
    for b in range(Bn):
        d = torch.cat([torch.zeros_like(flat[b]), flat[b]], 1).contiguous()
        box = T.delta2bbox(_cuda(sq), d, (0, 0, 0, 0), (0.07, 0.07, 0.14, 0.14), None, 1e-6)
        assert torch.equal(got[0][b].view(torch.int32), box.view(torch.int32))
    _twice(got, T.guided_anchors(*args))
    return got


@pytest.mark.parametrize("name", sorted(ANCHOR_CASES))
def test_guided_anchors(T, name):
    run_anchors(T, name)


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
    # name: (sizes, B, dtype, layout, seed, rows per image, all-zero weight map, shape avg factor)
    "b3_f32_nchw": (K.SMALL, 3, "f32", "nchw", 2, 12, False, 7.0),
    "b3_bf16_mixed_clip_up": (K.SMALL, 3, "bf16", "mixed", 3, 10, False, "tensors"),
    "b2_f16_nhwc": (K.SMALL, 2, "f16", "nhwc", 4, 9, False, "tensor"),
    "b2_f32_mixed_zero_weights": (K.SMALL, 2, "f32", "mixed", 6, 14, True, 3.0),
    "big_b2_bf16_nhwc": (K.BIG, 2, "bf16", "nhwc", 8, 40, False, 31.0),
}


def run_loss(T, name):
    sizes, Bn, dtype, layout, seed, nrows, zero_w, avg = LOSS_CASES[name]
    c = K.poison_unread(K.loss_case(sizes, Bn, dtype, seed, nrows, zero_w))
    g = (0.75, 1.5)
    N = K.nloc(sizes)
    loc_avg = Bn * N / 200.0
    avg_np, avg_t = avg, avg
    if avg == "tensors":
        avg_np = (np.array([3, 4], np.int32), np.array([5], np.int32))
        avg_t = tuple(_cuda(a) for a in avg_np)
    elif avg == "tensor":
        avg_np = (np.array([nrows, 2], np.int32),)
        avg_t = _cuda(avg_np[0])
    ref = R.loss(c["loc"], c["shape"], c["loc_targets"], c["loc_weights"], c["bbox_anchors"], c["bbox_gts"],
                 c["bbox_weights"], loc_avg, avg_np, g=g)
    assert ref["num_rows"] == nrows * (Bn - 1 if Bn > 1 else 1) and ref["switch_gap"] > 1e-3, ref["switch_gap"]
    assert ref["ties"] >= 1 and ref["clipped"] >= 2 and ref["losses"][1] > 0
    assert (ref["losses"][0] == 0) == zero_w
    assert np.all(ref["below_beta"] >= 1) and np.all(ref["above_beta"] >= 1), (ref["below_beta"], ref["above_beta"])
    assert ref["centre_clamped"] >= 2, ref["centre_clamped"]   # the far row's dx and dy terms are clamped at 0
    SEEN["tie"] += ref["ties"]
    SEEN["clip"] += ref["clipped"]
    dt = DT[dtype]
    targets = [_cuda(c[k]) for k in ("loc_targets", "loc_weights", "bbox_anchors", "bbox_gts", "bbox_weights")]
    gv = torch.tensor(g, device="cuda")

    def once():
        loc = [t.requires_grad_() for t in _layout(c["loc"], dtype, layout)]
        shape = [t.requires_grad_() for t in _layout(c["shape"], dtype, layout)]
        losses = T.ga_loss(loc, shape, *targets, loc_avg, avg_t)
        (losses * gv).sum().backward()
        return losses.detach(), loc, shape

    losses, loc, shape = once()
    got = losses.cpu().numpy().astype(np.float64)
    worst = {}
    for k in range(2):
        tol = ref["bound_losses"][k] + float(np.spacing(f32(abs(ref["losses"][k]))))
        err = abs(got[k] - ref["losses"][k])
        assert err <= tol, "%s: loss %d: got %r, ref %r, error %g > %g" % (name, k, got[k], ref["losses"][k], err, tol)
        worst["loss%d" % k] = err / tol
    for key, heads in (("dloc", loc), ("dshape", shape)):
        for l, h in enumerate(heads):
            assert h.grad.stride() == h.stride() and h.grad.shape == h.shape and h.grad.dtype == dt
            w = _check_grad(h.grad, ref[key][l], ref["bound_" + key][l], dt, "%s: %s[%d]" % (name, key, l))
            worst[key] = max(worst.get(key, 0.0), w)
    losses2, loc2, shape2 = once()
    _twice([losses] + [h.grad for h in loc + shape], [losses2] + [h.grad for h in loc2 + shape2])
    print("%s: worst error / tolerance %s" % (name, {k: round(float(v), 3) for k, v in worst.items()}))
    return ref


@pytest.mark.parametrize("name", sorted(LOSS_CASES))
def test_ga_loss(T, name):
    run_loss(T, name)


# ---- guided RPN proposals -------------------------------------------------------------------------------------------------
PROP_NAMES = ["proposals", "anchor_idx", "counts"]
PROPOSAL_CASES = {
    # name: (sizes, B, dtype, channels_last, mask kind, config)
    "b3_f32_masked": (K.SMALL, 3, "f32", False, "random", dict(nms_pre=40, nms_post=30, max_num=64, nms_thr=0.7)),
    "b2_bf16_nhwc_masked_minsize": (K.SMALL, 2, "bf16", True, "random",
                                    dict(nms_pre=0, nms_post=200, max_num=300, nms_thr=0.6, min_bbox_size=12,
                                         target_means=(0.0, 0.1, 0.0, -0.1), target_stds=(0.1, 0.1, 0.2, 0.2))),
    "b1_f32_ones": (K.SMALL, 1, "f32", True, "ones", dict(nms_pre=100, nms_post=50, max_num=120, nms_thr=0.7)),
    "big_b3_bf16_masked": (K.BIG, 3, "bf16", False, "random", dict(nms_pre=1000, nms_post=300, max_num=500, nms_thr=0.7)),
}


def _heads_t(arrs, dtype, channels_last):
    out = [torch.from_numpy(a).cuda().to(DT[dtype]) for a in arrs]
    return [t.contiguous(memory_format=torch.channels_last) for t in out] if channels_last else out


def run_proposals(T, name):
    sizes, Bn, dtype, cl, kind, cfg = PROPOSAL_CASES[name]
    c = K.proposal_case(sizes, Bn, dtype, 1, kind)
    means, stds = cfg.get("target_means", (0, 0, 0, 0)), cfg.get("target_stds", (1, 1, 1, 1))

    def gpu_decode(r, d, shape):
        return T.delta2bbox(_cuda(r), _cuda(d), means, stds, shape).cpu().numpy()

    info = {}
    ref = R.rpn_proposals(c["cls"], c["reg"], c["anchors"], c["mask"], c["img_shapes"], decode=gpu_decode, info=info,
                          **cfg)
    assert ref[2][0] > 0
    if kind == "random":
        assert info["empty_levels"] >= 1 and (Bn == 1 or ref[2][Bn - 1] == 0), info
        SEEN["empty_level"] += 1
        SEEN["empty_image"] += int(Bn > 1)
    args = (_heads_t(c["cls"], dtype, cl), _heads_t(c["reg"], dtype, cl), _cuda(c["anchors"]), _cuda(c["mask"]),
            _cuda(c["img_shapes"]))
    got = T.ga_rpn_proposals(*args, **cfg)
    p, a, n = (t.cpu().numpy() for t in got)
    assert np.array_equal(n, ref[2]), (n, ref[2])
    assert np.array_equal(a, ref[1])
    assert np.array_equal(p[..., :4].view(np.uint32), ref[0][..., :4].view(np.uint32))
    assert np.all(np.abs(p[..., 4] - ref[0][..., 4]) <= 1e-6)
    for b in range(Bn):
        assert np.all(p[b, n[b]:] == 0) and np.all(a[b, n[b]:] == -1)
    _twice(got, T.ga_rpn_proposals(*args, **cfg))
    return got


@pytest.mark.parametrize("name", sorted(PROPOSAL_CASES))
def test_ga_rpn_proposals(T, name):
    run_proposals(T, name)


@pytest.mark.parametrize("sizes,dtype,cl", [(K.SMALL, "f32", False), (K.BIG, "bf16", True)], ids=["small", "big"])
def test_shared_anchors_and_a_full_mask_are_rpn_proposals(T, sizes, dtype, cl):
    """Shared anchors broadcast to (B, Nloc, 4), a mask of ones, A = 1: all three outputs are rpn_proposals' bits."""
    Bn = 3
    c = K.proposal_case(sizes, Bn, dtype, 2, "ones")
    shared = _cuda(c["anchors"][0])
    off = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])])
    per_level = [shared[off[l]:off[l + 1]].contiguous() for l in range(len(sizes))]
    cls, reg, ish = _heads_t(c["cls"], dtype, cl), _heads_t(c["reg"], dtype, cl), _cuda(c["img_shapes"])
    for cfg in (dict(nms_pre=300, nms_post=200, max_num=400, nms_thr=0.7, min_bbox_size=8),
                dict(nms_pre=4096 if sizes is K.BIG else 0, nms_post=1000, max_num=2000, nms_thr=0.5)):
        ref = T.rpn_proposals(cls, reg, per_level, ish, **cfg)
        got = T.ga_rpn_proposals(cls, reg, shared[None].expand(Bn, -1, -1).contiguous(), _cuda(c["mask"]), ish, **cfg)
        assert int(ref[2].min()) > 0
        _twice(got, ref)


# ---- the chain, captured ----------------------------------------------------------------------------------------------------
def _chain_inputs(seed):
    c = K.shape_case(K.SMALL, 9, 2, 7, (7, 4), seed, True)
    loc, shape = K.head_case(K.SMALL, 2, "bf16", seed)
    p = K.proposal_case(K.SMALL, 2, "bf16", seed, "ones")
    heads = [torch.from_numpy(a).to(torch.bfloat16) for a in loc + shape + p["cls"] + p["reg"]]
    return heads + [torch.from_numpy(c[k]) for k in ("gt", "counts", "flags", "img_shapes", "keys")], c


def test_chain_eager_and_graph_replay(T):
    """guided_anchors -> anchor_target and -> ga_rpn_proposals, ga_loc_target + ga_shape_target -> ga_loss -> backward, captured once and replayed
    on new inputs: a host synchronisation or an allocation inside the library would break the capture.  Eager and
    replayed results agree bit for bit, and two replays differ."""
    L = len(K.SMALL)
    first, c = _chain_inputs(1)
    bufs = [t.cuda() for t in first]
    approxs, squares = _cuda(c["approxs"]), _cuda(c["squares"])

    def step():
        leaves = [t.detach().requires_grad_() for t in bufs[:2 * L]]
        gt, cn, flags, shapes, keys = bufs[4 * L:]
        anchors, mask = T.guided_anchors(bufs[L:2 * L], squares, bufs[:L], 0.01)
        at = T.anchor_target(anchors, mask, gt, cn, shapes, keys=keys)
        pr = T.ga_rpn_proposals(bufs[2 * L:3 * L], bufs[3 * L:4 * L], anchors, mask, shapes, nms_pre=60, max_num=100)
        lt, lw, lavg = T.ga_loc_target(K.SMALL, K.STRIDES, K.ANCHOR_SCALE, gt, cn)
        st = T.ga_shape_target(approxs, squares, flags, gt, cn, shapes, keys=keys)
        losses = T.ga_loss(leaves[:L], leaves[L:], lt, lw, st[0], st[1], st[2], lavg, (st[3], st[4]))
        losses.sum().backward()
        return [anchors, mask, at[0], at[2], lt, lw] + list(st) + [losses.detach()] + [t.grad for t in leaves] + list(pr)

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
            for dst, src in zip(bufs, _chain_inputs(seed)[0]):
                assert dst.stride() == src.stride()
                dst.copy_(src)
        graph.replay()
        eager = step()
        torch.cuda.synchronize()
        assert int(eager[9].sum()) > 0 and int(eager[2].sum()) > 0              # shape positives; anchor_target positives
        assert int(eager[-1].min()) > 0 and int(eager[1].sum()) < eager[1].numel()   # proposals; a mask that cuts
        for a, b in zip(captured, eager):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))
        seen.append([captured[0].clone(), captured[13].clone(), captured[14 + L].clone(), captured[-3].clone()])
    for x, y in zip(*seen):
        assert not torch.equal(x, y)


# ---- under the guard -----------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import guided_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, guided_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


@pytest.mark.parametrize("name", ["b3_g9", "b2_g0", "big_b3_g9"])
def test_guarded_loc_target(T, guard, name):
    run_loc(T, name)
    _clean(guard, ["ga_loc_target"])


@pytest.mark.parametrize("name", ["a9_b3", "a9_b3_first", "a1_b3_all", "a3_b2_g0", "big_a9_b3"])
def test_guarded_shape_target(T, guard, name):
    run_shape(T, name)
    _clean(guard, ["ga_shape_target"])


@pytest.mark.parametrize("name", ["b3_f32_nchw", "b2_bf16_mixed", "b1_f16_nhwc_nomask", "big_b2_f32_mixed"])
def test_guarded_anchors(T, guard, name):
    run_anchors(T, name)
    _clean(guard, ["guided_anchors"])


@pytest.mark.parametrize("name", ["b3_f32_nchw", "b3_bf16_mixed_clip_up", "b2_f16_nhwc", "big_b2_bf16_nhwc"])
def test_guarded_loss(T, guard, name):
    """Poisoned outputs and an exact-size workspace: every gradient element must have been WRITTEN."""
    run_loss(T, name)
    _clean(guard, ["ga_loss_fwd", "ga_loss_bwd"])


@pytest.mark.parametrize("name", ["b3_f32_masked", "b2_bf16_nhwc_masked_minsize", "big_b3_bf16_masked"])
def test_guarded_proposals(T, guard, name):
    """Every unused output row must have been WRITTEN, on an exact-size workspace."""
    run_proposals(T, name)
    _clean(guard, ["ga_rpn_proposals"])


def test_every_entry_point_ran_under_the_guard_and_every_path_ran():
    """Counts what the tests above did IN THIS RUN (run the file as a whole)."""
    from torch_detection_amd import guided_ops
    public = sorted(n for n, v in vars(guided_ops).items()
                    if inspect.isfunction(v) and v.__module__ == guided_ops.__name__ and not n.startswith("_"))
    assert public == ["ga_loc_target", "ga_loss_bwd", "ga_loss_fwd", "ga_rpn_proposals", "ga_shape_target",
                      "guided_anchors"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in ("ga_shape_target", "ga_loss_fwd", "ga_rpn_proposals"):
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)
    assert all(v >= 1 for v in SEEN.values()), SEEN
