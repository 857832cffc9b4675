"""CPU: the Guided Anchoring oracle (tests/ga_ref.py) is pinned on its own — the level rule against mmdetection's float64
log2 formula, the region rule on hand-computed boxes, the approx-max assignment against target_ref's max-IoU assignment,
the loss against finite differences — the shared cases (tests/ga_cases.py) hold what they promise, and every wrapper of
torch_detection_amd.guided refuses bad arguments before it needs a GPU."""
import numpy as np
import pytest
import torch

import ga_cases as K
import ga_ref as G
import target_ref as TR

f32 = np.float32


# ---- the level rule -------------------------------------------------------------------------------------------------------
def test_level_rule_agrees_with_the_log2_formula_off_the_thresholds():
    L = len(K.SMALL)
    thr = G.level_thresholds(K.ANCHOR_SCALE, K.STRIDES[0], L)
    assert [float(t) for t in thr] == [72.0, 288.0, 1152.0, 4608.0]
    seen = set()
    for seed in range(6):
        gt, cn = K.gt_case(3, 40, (40, 40, 40), seed, K.BIG)
        boxes = gt.reshape(-1, 4)
        area = G.gt_areas(boxes).astype(np.float64)
        on_thr = np.isin(area, np.asarray(thr, np.float64))
        lv = G.gt_levels(boxes, K.ANCHOR_SCALE, K.STRIDES[0], L)
        ref = G.gt_levels_log2(boxes, K.ANCHOR_SCALE, K.STRIDES[0], L)
        # a box within a few float64 ulp of a threshold may fall either way in the log2 formula: none of the cases is
        near = np.min(np.abs(area[:, None] / np.asarray(thr, np.float64)[None] - 1), axis=1) < 1e-9
        assert np.array_equal(lv[~on_thr & ~near], ref[~on_thr & ~near])
        assert on_thr.sum() >= 1 and not (near & ~on_thr).any()
        seen |= set(lv.tolist())
    assert seen == set(range(L))
    # planted exactly on t_1: the upper level
    assert G.gt_levels(K.PLANTED[2], K.ANCHOR_SCALE, K.STRIDES[0], L)[0] == 1
    assert G.gt_areas(K.PLANTED[2])[0] == 72
    for k, t in enumerate(thr):                               # on every threshold, and one fp32 step below it
        side = np.sqrt(float(t))
        if side == int(side):
            box = np.array([0, 0, side - 1, side - 1], f32)
            assert G.gt_levels(box, K.ANCHOR_SCALE, K.STRIDES[0], L)[0] == k + 1


# ---- the region rule ------------------------------------------------------------------------------------------------------
def test_region_rule_on_hand_computed_boxes():
    half = G.ratio_pair(0.5)
    assert half == (f32(0.25), f32(0.75))
    # g = (0, 0, 2, 1.5): x1 = 0.5 -> 0, x2 = 1.5 -> 2 (half to even), y1 = 0.375 -> 0, y2 = 1.125 -> 1
    assert G.calc_region(np.array([0, 0, 2, 1.5], f32), half, 16, 24) == (0, 0, 2, 1)
    # g = (1, 1, 3, 7): x1 = 1.5 -> 2, x2 = 2.5 -> 2, y1 = 2.5 -> 2, y2 = 5.5 -> 6
    assert G.calc_region(np.array([1, 1, 3, 7], f32), half, 16, 24) == (2, 2, 2, 6)
    # clamped at every border
    assert G.calc_region(np.array([-90, -90, 99, 99], f32), half, 4, 6) == (0, 0, 5, 3)
    assert G.calc_region(np.array([50, 50, 60, 60], f32), half, 4, 6) == (5, 3, 5, 3)
    ctr = G.ratio_pair(0.2)
    assert ctr == (f32(0.4), f32(0.6))
    # g = (10, 10, 10.5, 10.5): 10.2 -> 10 and 10.3 -> 10: one pixel
    assert G.calc_region(np.array([10, 10, 10.5, 10.5], f32), ctr, 16, 24) == (10, 10, 10, 10)


@pytest.mark.parametrize("sizes", [K.SMALL, K.BIG], ids=["small", "big"])
def test_loc_target_cases_hold_what_they_promise(sizes):
    gt, cn = K.gt_case(3, 9, (9, 0, 5), 1, sizes)
    info = {}
    t, w, avg = G.loc_target(sizes, K.STRIDES, K.ANCHOR_SCALE, gt, cn, info=info)
    N = K.nloc(sizes)
    assert t.shape == (3, N) and w.shape == (3, N) and avg == 3 * N / 200.0
    assert set(np.unique(t).tolist()) == {0, 1}
    assert set(np.unique(w).tolist()) == {0.0, float(f32(0.1)), 1.0}
    assert info["levels"] >= {0, len(sizes) - 1} and info["one_pixel"] >= 1 and info["clamped"] >= 1
    assert info["erased_final"] >= 1                          # a later ignore region erased an earlier weight 1
    assert not t[1].any() and np.all(w[1] == f32(0.1))        # no ground truths
    # the order matters: the two overlapping boxes swapped give another result
    sw = gt.copy()
    sw[0, [5, 6]] = gt[0, [6, 5]]
    t2, w2, _ = G.loc_target(sizes, K.STRIDES, K.ANCHOR_SCALE, sw, cn)
    assert np.array_equal(t, t2) and not np.array_equal(w, w2)


# ---- the approx-max assignment --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("all_", [True, False])
def test_approx_assignment_is_max_iou_assignment_for_one_approx(all_):
    c = K.shape_case(K.SMALL, 1, 3, 7, (7, 0, 5), 3, True)
    assert np.array_equal(c["approxs"][:, 0], c["squares"])
    info = {}
    ref = TR.anchor_target(c["squares"], c["flags"], c["gt"], c["counts"], c["img_shapes"], keys=c["keys"],
                           gt_max_assign_all=all_)
    got = G.shape_target(c["approxs"], c["squares"], c["flags"], c["gt"], c["counts"], c["img_shapes"], keys=c["keys"],
                         gt_max_assign_all=all_, info=info)
    assert np.array_equal(got[5], ref[6])
    assert np.array_equal(got[3], ref[4]) and np.array_equal(got[4], ref[5])
    assert np.array_equal(got[2], ref[3])
    a2, m2 = TR.assign_max_iou(c["squares"], c["gt"], c["counts"], 0.7, 0.3, 0.3, all_)
    free = G.shape_target(c["approxs"], c["squares"], None, c["gt"], c["counts"], None, allowed_border=-1,
                          gt_max_assign_all=all_, sampling=False)
    assert np.array_equal(free[5], a2) and np.array_equal(free[6].view(np.uint32), m2.view(np.uint32))
    assert np.array_equal(free[3], (a2 > 0).sum(1)) and np.array_equal(free[4], (a2 == 0).sum(1))
    assert info["col_ties"] >= 1 and got[3].sum() > 0


@pytest.mark.parametrize("A", [3, 9])
def test_shape_cases_hold_what_they_promise(A):
    c = K.shape_case(K.SMALL, A, 3, 7, (7, 0, 5), 4, False)
    info = {}
    out = G.shape_target(c["approxs"], c["squares"], c["flags"], c["gt"], c["counts"], c["img_shapes"], num=16,
                         keys=c["keys"], info=info)
    assert info["single"] >= 1 and info["out"] >= 1 and info["approx_ties"] >= 1 and info["col_ties"] >= 1
    assert info["single_inside"] >= 1                         # every flag set, one approx inside the image
    assert info["cut"] >= 1 and out[3].sum() > 0
    pos = out[2][..., 0] > 0
    assert np.array_equal(out[0][pos], np.broadcast_to(c["squares"], out[0].shape)[pos])
    assert not out[0][~pos].any() and not out[1][~pos].any()
    # the maximum runs over all approxs: dropping one changes overlaps somewhere
    ov = G.approx_overlaps(c["approxs"], c["gt"][0, :7])
    assert (ov > G.approx_overlaps(c["approxs"][:, :1], c["gt"][0, :7])).any()


# ---- guided anchors -------------------------------------------------------------------------------------------------------
def test_guided_anchor_oracle():
    loc, shape = K.head_case(K.SMALL, 2, "f32", 5)
    sq = K.squares_of(K.SMALL)
    anchors, mask, tol = G.guided_anchors([np.zeros_like(s) for s in shape], sq)
    assert np.array_equal(anchors[0], sq) and mask.all()      # zero deltas give the integer squares back
    thr = G.loc_threshold(0.01)
    assert abs(1 / (1 + np.exp(-float(thr))) - 0.01) < 1e-8
    anchors, mask, tol = G.guided_anchors(shape, sq, loc, 0.01)
    z = np.concatenate([G.rows(p) for p in loc], 1)[..., 0]
    assert np.array_equal(mask, (1 / (1 + np.exp(-z.astype(np.float64))) >= 0.01).astype(np.uint8))
    assert 0 < mask.mean() < 1 and np.all(tol > 0)


# ---- guided RPN proposals -------------------------------------------------------------------------------------------------
def test_proposal_oracle_is_the_rpn_oracle_for_shared_anchors_and_a_full_mask():
    import proposal_ref as PR
    c = K.proposal_case(K.SMALL, 2, "f32", 1, "ones")
    c["anchors"][1] = c["anchors"][0]
    off = np.concatenate([[0], np.cumsum([h * w for h, w in K.SMALL])])
    per_level = [c["anchors"][0, off[l]:off[l + 1]] for l in range(len(K.SMALL))]
    cfg = dict(nms_pre=100, nms_post=60, max_num=150, nms_thr=0.7, min_bbox_size=4)
    ref = PR.rpn_proposals(c["cls"], c["reg"], per_level, c["img_shapes"], **cfg)
    got = G.rpn_proposals(c["cls"], c["reg"], c["anchors"], c["mask"], c["img_shapes"], **cfg)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    assert ref[2].min() > 60


def test_proposal_oracle_with_masks():
    c = K.proposal_case(K.SMALL, 3, "bf16", 2, "random")
    info = {}
    cfg = dict(nms_pre=40, nms_post=30, max_num=64, nms_thr=0.7)
    props, aidx, counts = G.rpn_proposals(c["cls"], c["reg"], c["anchors"], c["mask"], c["img_shapes"], info=info, **cfg)
    assert info["empty_levels"] >= 1 + len(K.SMALL) and info["cut_levels"] >= 1 and info["short_levels"] >= 1
    assert counts[2] == 0 and not props[2].any() and np.all(aidx[2] == -1) and counts[0] > 0
    for b in range(2):
        assert c["mask"][b, aidx[b, :counts[b]]].all()        # only locations that are in
        assert np.all(np.diff(props[b, :counts[b], 4]) <= 0)
    n0, n1 = 16 * 24, 16 * 24 + 8 * 12
    assert not ((aidx[0] >= n0) & (aidx[0] < n1)).any()       # image 0's level 1 is masked out
    # the mask matters: with a full mask other locations win
    full = G.rpn_proposals(c["cls"], c["reg"], c["anchors"], np.ones_like(c["mask"]), c["img_shapes"], **cfg)
    assert not np.array_equal(full[1][0], aidx[0]) and full[2][2] > 0


# ---- the loss -------------------------------------------------------------------------------------------------------------
def _loss_args(c, avg=7.0):
    return (c["loc"], c["shape"], c["loc_targets"], c["loc_weights"], c["bbox_anchors"], c["bbox_gts"],
            c["bbox_weights"], 5.12, avg)


def test_loss_oracle_matches_finite_differences():
    c = K.loss_case(K.SMALL, 3, "f32", 6, 12)
    g = (0.7, 1.3)
    ref = G.loss(*_loss_args(c), g=g)
    assert ref["num_rows"] == 24 and ref["ties"] >= 1 and ref["clipped"] >= 2 and ref["switch_gap"] > 1e-3
    assert ref["losses"][0] > 0 and ref["losses"][1] > 0
    assert np.all(ref["below_beta"] >= 1) and np.all(ref["above_beta"] >= 1) and ref["centre_clamped"] >= 2
    rng = np.random.default_rng(0)
    h = 1e-6
    row = c["bbox_weights"][..., 0] > 0
    n0 = 0
    checked = 0
    for l, (H, W) in enumerate(K.SMALL):
        n1 = n0 + H * W
        for key, grad in (("loc", "dloc"), ("shape", "dshape")):
            arr = c[key][l]
            for _ in range(6):
                i = tuple(int(rng.integers(0, s)) for s in arr.shape)
                p = n0 + i[2] * W + i[3]
                if key == "shape" and (not row[i[0], p] or p in (c["planted"]["tie"], c["planted"]["clip"])):
                    assert ref[grad][l][i] == 0 or p == c["planted"]["tie"]
                    continue
                vals = []
                for sgn in (1, -1):
                    cc = dict(c)
                    cc[key] = [a.astype(np.float64) for a in c[key]]
                    cc[key][l][i] += sgn * h
                    r = G.loss(*_loss_args(cc), g=g)
                    vals.append(float(np.dot(r["losses"], np.asarray(g, f32).astype(np.float64))))
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - ref[grad][l][i]) <= 1e-6 * max(1.0, abs(fd)), (key, l, i, fd, ref[grad][l][i])
                checked += 1
        n0 = n1
    assert checked >= 20
    # the tie takes half of each side's derivative, the clipped row none
    t = c["planted"]["tie"]
    flat = np.concatenate([G.rows(d) for d in ref["dshape"]], 1)
    assert flat[0, t, 0] != 0 and not flat[0, c["planted"]["clip"]].any()


def test_loss_oracle_bounds_and_unread_elements():
    c = K.loss_case(K.SMALL, 3, "bf16", 8, 10)
    ref = G.loss(*_loss_args(c))
    poisoned = G.loss(*_loss_args(K.poison_unread(c)))
    for k in ("losses", "bound_losses"):
        assert np.array_equal(ref[k], poisoned[k])
    for k in ("dloc", "dshape", "bound_dloc", "bound_dshape"):
        for a, b in zip(ref[k], poisoned[k]):
            assert np.array_equal(a, b)
    assert np.all(ref["bound_losses"] > 0) and np.all(ref["bound_losses"] < 1e-4 * ref["losses"])
    for d, b in zip(ref["dshape"], ref["bound_dshape"]):
        assert np.all(b[d != 0] > 0) and not b[d == 0].any()
    d, b = (np.concatenate([G.rows(v) for v in ref[k]], 1) for k in ("dshape", "bound_dshape"))
    rel = b / np.maximum(np.abs(d), 1e-300)
    tie = c["planted"]["tie"]                                 # there the two sides of min nearly cancel: a gradient of
    assert 1e-3 < rel[0, tie].max() < 0.5                     # the order of eps with the rounding errors of each side
    rel[0, tie] = 0
    assert rel.max() < 1e-4
    zero = G.loss(*_loss_args(K.loss_case(K.SMALL, 2, "f32", 9, 5, zero_weights=True)))
    assert zero["losses"][0] == 0 and not any(d.any() for d in zero["dloc"])
    ints = G.loss(*_loss_args(c, avg=(np.array([3, 4], np.int32), np.array([5], np.int32))))
    assert ints["norm"][1] == 12


# ---- argument checks ------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_without_a_gpu():
    import torch_detection_amd as T
    gt, cn = K.gt_case(2, 3, (3, 1), 0, K.SMALL)
    gt, cn = torch.from_numpy(gt), torch.from_numpy(cn)
    bad = pytest.raises(ValueError)
    with bad:
        T.ga_loc_target(K.SMALL, K.STRIDES[:4], 8, gt, cn)
    with bad:
        T.ga_loc_target([], [], 8, gt, cn)
    with bad:
        T.ga_loc_target(K.SMALL, K.STRIDES, 0, gt, cn)
    with bad:
        T.ga_loc_target(K.SMALL, K.STRIDES, 8, gt, cn, center_ratio=1.5)
    with bad:
        T.ga_loc_target(K.SMALL, K.STRIDES, 8, gt.double(), cn)
    with bad:
        T.ga_loc_target(K.SMALL, K.STRIDES, 8, torch.zeros(2, 300, 4), cn)
    with pytest.raises(ValueError, match="CUDA"):
        T.ga_loc_target(K.SMALL, K.STRIDES, 8, gt, cn)
    c = K.shape_case(K.SMALL, 3, 2, 3, (3, 1), 0, True)
    ap, sq, fl = (torch.from_numpy(c[k]) for k in ("approxs", "squares", "flags"))
    shp = torch.from_numpy(c["img_shapes"])
    with bad:
        T.ga_shape_target(ap.reshape(-1, 4), sq, fl, gt, cn, shp)
    with bad:
        T.ga_shape_target(torch.zeros(512, 17, 4), sq, None, gt, cn, shp)
    with bad:
        T.ga_shape_target(ap, sq[:100], fl, gt, cn, shp)
    with bad:
        T.ga_shape_target(ap, sq, fl[:, :100], gt, cn, shp)
    with bad:
        T.ga_shape_target(ap, sq, fl, gt, cn, None)               # allowed_border 0 needs the shapes
    with bad:
        T.ga_shape_target(ap, sq, fl, gt, cn, shp, num=1 << 20)
    with bad:
        T.ga_shape_target(ap, sq, fl, gt, cn, shp, pos_iou_thr=(0.5, 0.7))
    with pytest.raises(ValueError, match="CUDA"):
        T.ga_shape_target(ap, sq, fl, gt, cn, shp)
    loc, shape = K.head_case(K.SMALL, 2, "f32", 1)
    loc, shape = [torch.from_numpy(a) for a in loc], [torch.from_numpy(a) for a in shape]
    with bad:
        T.guided_anchors(shape, sq, loc)                          # loc_preds without a threshold
    with bad:
        T.guided_anchors(shape, sq, loc, 1.0)
    with bad:
        T.guided_anchors(shape[:4], sq)                           # the squares of another pyramid
    with bad:
        T.guided_anchors(shape, sq, anchoring_stds=(1, 1, 1))
    with bad:
        T.guided_anchors([s[:, :1] for s in shape], sq)
    with bad:
        T.guided_anchors([s.transpose(2, 3) for s in shape], sq)  # neither NCHW nor channels_last
    with pytest.raises(ValueError, match="CUDA"):
        T.guided_anchors(shape, sq)
    k = K.loss_case(K.SMALL, 2, "f32", 2, 4)
    tg = [torch.from_numpy(k[n]) for n in ("loc_targets", "loc_weights", "bbox_anchors", "bbox_gts", "bbox_weights")]
    with bad:
        T.ga_loss(loc[:4], shape, *tg, 5.0, 3.0)
    with bad:
        T.ga_loss(loc, shape, tg[0][:, :100], *tg[1:], 5.0, 3.0)
    with bad:
        T.ga_loss(loc, shape, *tg, 0.0, 3.0)
    with bad:
        T.ga_loss(loc, shape, *tg, 5.0, None)
    with bad:
        T.ga_loss(loc, shape, *tg, 5.0, 3.0, beta=0)
    with bad:
        T.ga_loss(loc, shape, *tg, 5.0, 3.0, eps=1.0)
    with bad:
        T.ga_loss(loc, [s.half() for s in shape], *tg, 5.0, 3.0)
    with pytest.raises(ValueError, match="CUDA"):
        T.ga_loss(loc, shape, *tg, 5.0, 3.0)
    p = K.proposal_case(K.SMALL, 2, "f32", 3, "random")
    cls, reg = [torch.from_numpy(a) for a in p["cls"]], [torch.from_numpy(a) for a in p["reg"]]
    an, mk, ish = torch.from_numpy(p["anchors"]), torch.from_numpy(p["mask"]), torch.from_numpy(p["img_shapes"])
    with bad:
        T.ga_rpn_proposals(cls, reg[:4], an, mk, ish)
    with bad:
        T.ga_rpn_proposals([c.repeat(1, 3, 1, 1) for c in cls], reg, an, mk, ish)   # one anchor per location
    with bad:
        T.ga_rpn_proposals(cls, reg, an[0], mk, ish)                                # anchors are per image
    with bad:
        T.ga_rpn_proposals(cls, reg, an, mk[:, :100], ish)
    with bad:
        T.ga_rpn_proposals(cls, reg, an, mk.float(), ish)
    with bad:
        T.ga_rpn_proposals(cls, reg, an, mk, ish, nms_pre=5000)
    with bad:
        T.ga_rpn_proposals(cls, reg, an, mk, ish, max_num=0)
    with bad:
        T.ga_rpn_proposals([c.half() for c in cls], [r.half() for r in reg], an, mk, ish)
    with bad:
        T.ga_rpn_proposals(cls, reg, an, mk, [(64, 96)] * 2)                        # a device tensor: no host copy
    with pytest.raises(ValueError, match="CUDA"):
        T.ga_rpn_proposals(cls, reg, an, mk, ish)
