"""GPU tests of the training-target kernels (assign_max_iou, sample_assigned, anchor_target, sample_rois) against the
CPU oracle tests/target_ref.py, at full size, in a graph, and under guard-banded, poisoned outputs
with exact-size workspaces (tests/guard_util.py)."""
import inspect

import numpy as np
import pytest
import torch

import guard_util as G
import proposal_ref as PR
import target_cases as C
import target_ref as R
import test_gpu_proposals as TP

pytestmark = pytest.mark.gpu

MEANS, STDS = (0.0, 0.1, 0.0, -0.1), (0.1, 0.1, 0.2, 0.2)
ENTERED, WS_SEEN = set(), {}        # what ran under the guard in this run (checked by the last test of the file)


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _cuda(case):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _compare_targets(got_t, ref_t, boxes, gt, assigned_rows, means, stds, what):
    """dx, dy bit for bit; dw, dh within the bound of test_gpu_proposals.test_bbox2delta_vs_oracle: 4 ulp of the
    un-normalised value / std + 1 ulp.  ``assigned_rows``: (rows of got_t, box of the row, gt of the row)."""
    assert np.array_equal(_bits(got_t[..., :2]), _bits(ref_t[..., :2])), what + ": dx / dy differ"
    rows, bx, g = assigned_rows
    tol = np.zeros(ref_t.shape[:-1] + (2,), np.float32)
    if len(rows):
        raw = PR.bbox2delta(bx, g)
        tol[rows] = 4 * np.spacing(np.abs(raw[:, 2:])) / np.float32(stds[2]) + np.spacing(np.abs(ref_t[rows][:, 2:]))
    err = np.abs(got_t[..., 2:] - ref_t[..., 2:])
    print("%s: dw/dh max error %g over %d positives" % (what, float(err.max()) if err.size else 0.0, bx.shape[0]))
    assert np.all(err <= tol), what + ": dw / dh beyond the bound"


def _check_anchor_target(T, case, info_check, **kw):
    info = {}
    ref = R.anchor_target(info=info, **case, **kw)
    if info_check:
        C.assert_coverage(info, int(kw.get("num", 256) * kw.get("pos_fraction", 0.5)))
    else:
        assert info["only_step6"] >= 1 and info["step6_ties"] >= 1, info
    d = _cuda(case)
    dk = dict(kw)
    if dk.get("keys") is not None:
        dk["keys"] = torch.from_numpy(dk["keys"]).cuda()
    got = T.anchor_target(**d, **dk)
    again = T.anchor_target(**d, **dk)
    torch.cuda.synchronize()
    for a, b in zip(got, again):                                   # run to run: bitwise
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    got = [g.cpu().numpy() for g in got]
    names = ("labels", "label_weights", "bbox_targets", "bbox_weights", "num_pos", "num_neg", "assigned")
    for k in (6, 4, 5, 0, 1, 3):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, names[k]
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), "%s: %d differ" % (names[k], (got[k] != ref[k]).sum())
    bi, ii = np.nonzero(ref[0])
    anchors = case["anchors"]
    bx = anchors[ii] if anchors.ndim == 2 else anchors[bi, ii]
    g = case["gt_bboxes"][bi, ref[6][bi, ii] - 1]
    _compare_targets(got[2], ref[2], None, None, ((bi, ii), bx, g), kw.get("target_means", (0, 0, 0, 0)),
                     kw.get("target_stds", (1, 1, 1, 1)), "anchor_target")
    assert np.all(got[2][ref[0] == 0] == 0)
    return got


@pytest.mark.parametrize("name,per_image,all_,own_keys", [
    ("b3", False, True, False),
    ("b3", True, False, True),
    ("b2", False, True, True),
    ("b2", True, True, False),
])
def test_anchor_target_c4_vs_oracle(T, name, per_image, all_, own_keys):
    case = C.anchor_case(per_image_boxes=per_image, **C.CASES[name])
    assert case["anchors"].shape[-2] == C.NUM_ANCHORS
    Bn = len(case["gt_counts"])
    keys = C.caller_keys(Bn, C.NUM_ANCHORS, 5) if own_keys else None
    # num = 2000 at (100, 256) ground truths: one image has more positives than 1000, the other fewer
    _check_anchor_target(T, case, info_check=all_ and not per_image, gt_max_assign_all=all_, keys=keys, seed=77,
                         num=256 if name == "b3" else 2000, target_means=MEANS, target_stds=STDS)


@pytest.mark.parametrize("all_", [True, False])
def test_assign_and_sample_c4_vs_oracle(T, all_):
    """The two building blocks on their own: max_overlaps as bit patterns, masks with generated and caller keys."""
    case = C.anchor_case(**C.CASES["b3"])
    valid = case["valid_flags"] & R.inside_border(case["anchors"], (800, 1100), 0).astype(np.uint8)[None]
    ra, rm = R.assign_max_iou(case["anchors"], case["gt_bboxes"], case["gt_counts"], 0.7, 0.3, 0.3, all_, valid)
    d = _cuda(case)
    ga, gm = T.assign_max_iou(d["anchors"], d["gt_bboxes"], d["gt_counts"], 0.7, 0.3, 0.3, all_,
                              torch.from_numpy(valid).cuda())
    assert np.array_equal(ga.cpu().numpy(), ra)
    assert np.array_equal(_bits(gm.cpu().numpy()), _bits(rm))
    assert (ra > 0).sum() > 0 and (ra == -1).sum() > 0
    for keys in (None, C.caller_keys(3, C.NUM_ANCHORS, 9)):
        for num, frac, ub in ((256, 0.5, -1), (64, 0.25, 3), (8192, 0.5, 0.5), (0, 0.5, -1)):
            ref = R.sample_assigned(ra, num, frac, ub, keys, 123)
            got = T.sample_assigned(ga, num, frac, ub, None if keys is None else torch.from_numpy(keys).cuda(), 123)
            for r, g_, nm in zip(ref, got, ("pos_mask", "neg_mask", "num_pos", "num_neg")):
                assert g_.cpu().numpy().dtype == r.dtype and np.array_equal(g_.cpu().numpy(), r), (nm, num, frac, ub)


def _rpn_output(T, B):
    anchors = TP._pyramid(T, TP.LEVELS)
    cls, reg = TP._head_outputs(B, TP.LEVELS, 31, torch.float32, False, "normal")
    ish = torch.tensor([(800, 1344), (600, 1000)][:B], dtype=torch.int32).cuda()
    props, _, counts = T.rpn_proposals(cls, reg, anchors, ish, nms_pre=2000, nms_post=2000, max_num=2000)
    return props, counts


def _roi_gts(props, counts, G, gt_counts, seed):
    """Ground truths around real proposals (moved by a few pixels: IoU on both sides of 0.5), a duplicate pair."""
    g = np.random.default_rng(seed)
    Bn = props.shape[0]
    gt = np.zeros((Bn, G, 4), np.float32)
    for b in range(Bn):
        pick = g.integers(0, max(int(counts[b]), 1), gt_counts[b])
        gt[b, :gt_counts[b]] = np.floor(props[b, pick, :4]) + g.integers(-6, 7, (gt_counts[b], 4)).astype(np.float32)
        gt[b, :gt_counts[b], 2:] = np.maximum(gt[b, :gt_counts[b], 2:], gt[b, :gt_counts[b], :2] + 4)
        if gt_counts[b] >= 2:
            gt[b, 1] = gt[b, 0]
    labels = g.integers(1, 81, (Bn, G)).astype(np.int64)
    return gt, labels


def _check_sample_rois(T, props, counts, gt, labels, gt_counts, **kw):
    info = {}
    ref = R.sample_rois(props.cpu().numpy(), counts.cpu().numpy(), gt, labels, gt_counts, info=info, **kw)
    dk = dict(kw)
    if dk.get("keys") is not None:
        dk["keys"] = torch.from_numpy(dk["keys"]).cuda()
    args = (props, counts, torch.from_numpy(gt).cuda(), torch.from_numpy(labels).cuda(),
            torch.from_numpy(np.asarray(gt_counts, np.int32)).cuda())
    got = [g.cpu().numpy() for g in T.sample_rois(*args, **dk)]
    names = ("rois", "labels", "label_weights", "bbox_targets", "bbox_weights", "pos_gt_inds", "num_pos", "num_neg")
    for k in (6, 7, 0, 1, 2, 4, 5):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, names[k]
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), "%s: %d differ" % (names[k], (got[k] != ref[k]).sum())
    rows = np.nonzero(ref[4][:, 0])[0]
    num = kw.get("num", 512)
    g = gt[rows // num, ref[5][rows]]
    _compare_targets(got[3], ref[3], None, None, (rows, ref[0][rows, 1:], g), kw.get("target_means", (0, 0, 0, 0)),
                     kw.get("target_stds", (0.1, 0.1, 0.2, 0.2)), "sample_rois")
    return got, ref, info


@pytest.mark.parametrize("add_gt,own_keys,all_,ub", [(True, False, True, 2), (True, True, False, -1),
                                                     (False, False, True, 2)])
def test_sample_rois_vs_oracle_and_roi_align(T, add_gt, own_keys, all_, ub):
    props, counts = _rpn_output(T, 2)
    c = counts.cpu().numpy()
    assert c.min() > 600
    G, gt_counts = 40, (40, 3)
    gt, labels = _roi_gts(props.cpu().numpy(), c, G, gt_counts, 3)
    num = 512
    keys = C.caller_keys(2, 2000 + (G if add_gt else 0), 4) if own_keys else None
    got, ref, info = _check_sample_rois(T, props, counts, gt, labels, gt_counts, num=num, add_gt_as_proposals=add_gt,
                                        keys=keys, seed=5, gt_max_assign_all=all_, neg_pos_ub=ub, pos_fraction=0.1)
    n_exp = int(num * 0.1)                  # 51: 40 ground truths give more positives than that, 3 give fewer
    if add_gt and all_:
        assert any(n > n_exp for n in info["n_pos"]) and any(n < n_exp for n in info["n_pos"]), info
    rois, npos, nneg = got[0], got[6], got[7]
    for b in range(2):                                             # row layout
        r = rois[b * num:(b + 1) * num]
        k = npos[b] + nneg[b]
        assert np.all(r[:k, 0] == b) and np.all(r[k:, 0] == -1) and np.all(r[k:, 1:] == 0)
        assert np.all(got[2][b * num:b * num + k] == 1) and np.all(got[2][b * num + k:(b + 1) * num] == 0)
        assert np.all(got[5][b * num:b * num + npos[b]] >= 0) and np.all(got[5][b * num + npos[b]:(b + 1) * num] == -1)
    assert ub < 0 or (rois[:, 0] == -1).sum() > 0                  # neg_pos_ub = 2 leaves padding rows
    # roi_align takes the rows as they are; padding rows give zeros
    feats = [torch.randn(2, 64, h, w, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
             for h, w in ((200, 336), (100, 168), (50, 84), (25, 42))]
    out = T.roi_align(feats, torch.from_numpy(rois).cuda(), 7, [4, 8, 16, 32])
    out = out.float().cpu().numpy()
    assert out.shape[0] == 2 * num and np.all(out[rois[:, 0] == -1] == 0) and np.any(out[rois[:, 0] >= 0] != 0)


def test_graph_replay_matches_eager(T):
    """One anchor_target and one sample_rois call in a graph, replayed twice on new ground truths in the same buffers:
    a host synchronisation or an allocation inside the library would break the capture."""
    case = C.anchor_case(**C.CASES["b3"])
    d = _cuda(case)
    props, counts = _rpn_output(T, 2)
    c = counts.cpu().numpy()
    gts = [_roi_gts(props.cpu().numpy(), c, 40, (40, 3), s) for s in (1, 2, 3)]
    rgt, rlab = torch.from_numpy(gts[0][0]).cuda(), torch.from_numpy(gts[0][1]).cuda()
    rcnt = torch.tensor([40, 3], dtype=torch.int32).cuda()
    kw = dict(seed=9, target_means=MEANS, target_stds=STDS)
    T.anchor_target(**d, **kw)
    T.sample_rois(props, counts, rgt, rlab, rcnt, seed=9)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ga = T.anchor_target(**d, **kw)
        gr = T.sample_rois(props, counts, rgt, rlab, rcnt, seed=9)
    seen = []
    for rep, seed in enumerate((41, 42)):
        new = C.anchor_case(**dict(C.CASES["b3"], seed=seed))
        d["gt_bboxes"].copy_(torch.from_numpy(new["gt_bboxes"]))
        rgt.copy_(torch.from_numpy(gts[rep + 1][0]))
        g.replay()
        ea = T.anchor_target(**d, **kw)
        er = T.sample_rois(props, counts, rgt, rlab, rcnt, seed=9)
        ea2 = T.anchor_target(**d, **kw)
        torch.cuda.synchronize()
        for a, b, c2 in zip(ga, ea, ea2):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b)
            assert torch.equal(b.view(torch.int32) if b.dtype == torch.float32 else b,
                               c2.view(torch.int32) if c2.dtype == torch.float32 else c2)
        for a, b in zip(gr, er):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b)
        seen.append(ga[6].clone())
    assert not torch.equal(seen[0], seen[1])


def test_host_refusals(T):
    case = C.anchor_case(**C.CASES["b3"])
    d = _cuda(case)
    a, gt, cnt = d["anchors"], d["gt_bboxes"], d["gt_counts"]
    assigned = torch.zeros(3, 100, dtype=torch.int32, device="cuda")
    props = torch.zeros(3, 50, 5, device="cuda")
    pc = torch.zeros(3, dtype=torch.int32, device="cuda")
    lab = torch.zeros(3, gt.shape[1], dtype=torch.int64, device="cuda")
    bad = [
        (lambda: T.assign_max_iou(a.cpu(), gt, cnt, 0.7, 0.3), "boxes must be a CUDA tensor"),           # CPU tensors
        (lambda: T.assign_max_iou(a, gt.cpu(), cnt, 0.7, 0.3), "gt_bboxes must be a CUDA tensor"),
        (lambda: T.assign_max_iou(a.double(), gt, cnt, 0.7, 0.3), "boxes must be a contiguous float32"),  # dtypes
        (lambda: T.assign_max_iou(a, gt, cnt.long(), 0.7, 0.3), "gt_counts must be a contiguous int32"),
        (lambda: T.assign_max_iou(a, gt, cnt, 0.7, (0.1, 0.3)), "neg_iou_thr must be a number"),          # tuple threshold
        (lambda: T.assign_max_iou(a, gt, cnt, (0.7,), 0.3), "pos_iou_thr must be a number"),
        (lambda: T.assign_max_iou(a, torch.zeros(3, 257, 4, device="cuda"), cnt, 0.7, 0.3),
         r"257 ground truths per image \(max 256\)"),                                                    # G over the cap
        (lambda: T.assign_max_iou(a, torch.zeros(65, 4, 4, device="cuda"),
                                  torch.zeros(65, dtype=torch.int32, device="cuda"), 0.7, 0.3),
         "number of images must be in 1..64"),                                                           # B over 64
        (lambda: T.assign_max_iou(a, gt, cnt, 0.7, 0.3, valid=torch.ones(3, 5, dtype=torch.uint8, device="cuda")),
         r"valid must be a contiguous uint8 / bool \(3, \d+\)"),
        (lambda: T.sample_assigned(assigned, 8193, 0.5), "num must be in 0..8192"),                       # num over 8192
        (lambda: T.sample_assigned(assigned.long(), 256, 0.5), "assigned_gt_inds must be a contiguous int32"),
        (lambda: T.sample_assigned(assigned.cpu(), 256, 0.5), "assigned_gt_inds must be a CUDA tensor"),
        (lambda: T.sample_assigned(assigned, 256, 0.5, keys=torch.zeros(3, 100, device="cuda")),
         "keys must be a contiguous int32"),
        (lambda: T.anchor_target(**dict(d, img_shapes=d["img_shapes"].float())), "img_shapes must be a contiguous int32"),
        (lambda: T.anchor_target(num=8193, **d), "num must be in 0..8192"),
        (lambda: T.anchor_target(neg_iou_thr=(0.0, 0.3), **d), "neg_iou_thr must be a number"),
        (lambda: T.anchor_target(target_stds=(1, 1, 1), **d), "target_stds must have 4 finite entries"),
        (lambda: T.sample_rois(props, pc, gt, lab, cnt, num=8193), "num must be in 0..8192"),
        (lambda: T.sample_rois(props[..., :4].contiguous(), pc, gt, lab, cnt),
         r"proposals must be a contiguous float32 \(3, P, 5\)"),
        (lambda: T.sample_rois(props, pc, gt, lab.int(), cnt), "gt_labels must be a contiguous int64"),
        (lambda: T.sample_rois(props.cpu(), pc, gt, lab, cnt), "proposals must be a CUDA tensor"),
    ]
    for i, (f, msg) in enumerate(bad):
        with pytest.raises(ValueError, match=msg):
            f()
            pytest.fail("case %d was accepted" % i)
    torch.cuda.synchronize()


# ---- under the guard ------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import target_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, target_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


def test_guarded_anchor_target(T, guard):
    case = C.anchor_case(**C.CASES["b3"])
    _check_anchor_target(T, case, info_check=True, seed=77, target_means=MEANS, target_stds=STDS)
    _clean(guard, ["anchor_target"])
    case = C.anchor_case(per_image_boxes=True, **C.CASES["b2"])
    _check_anchor_target(T, case, info_check=False, gt_max_assign_all=False, keys=C.caller_keys(2, C.NUM_ANCHORS, 5))
    _clean(guard, [])


def test_guarded_assign_and_sample(T, guard):
    test_assign_and_sample_c4_vs_oracle(T, True)
    _clean(guard, ["assign_max_iou", "sample_assigned"])
    test_assign_and_sample_c4_vs_oracle(T, False)
    _clean(guard, [])


def test_guarded_sample_rois(T, guard):
    props, counts = _rpn_output(T, 2)
    guard.check()                                   # rpn_proposals is not under this guard; forget nothing of ours
    gt, labels = _roi_gts(props.cpu().numpy(), counts.cpu().numpy(), 40, (40, 3), 3)
    for all_ in (True, False):
        _check_sample_rois(T, props, counts, gt, labels, (40, 3), num=512, seed=5, gt_max_assign_all=all_)
        _clean(guard, ["sample_rois"])


def test_guarded_placeholder_regions(T, guard):
    """The shapes at which a workspace region would be empty and holds one placeholder element instead (DESIGN.md
    §5d): no ground truths, no anchors, no proposals.  The answers follow from the spec without the oracle."""
    anchors = torch.tensor([[0, 0, 9, 9], [5, 5, 20, 20], [30, 30, 40, 45], [2, 3, 11, 12], [50, 50, 60, 60]],
                           dtype=torch.float32, device="cuda")
    ish = torch.tensor([(100, 100), (80, 90)], dtype=torch.int32, device="cuda")
    none = torch.zeros(2, dtype=torch.int32, device="cuda")
    # G = 0: every anchor is a negative, num = 4 of the 5 are sampled
    got = T.anchor_target(anchors, None, torch.zeros(2, 0, 4, device="cuda"), none, ish, num=4)
    _clean(guard, [])
    labels, lw, bt, bwt, npos, nneg, assigned = [g.cpu() for g in got]
    assert assigned.shape == (2, 5) and bool((assigned == 0).all()) and bool((labels == 0).all())
    assert npos.tolist() == [0, 0] and nneg.tolist() == [4, 4] and lw.sum(1).tolist() == [4.0, 4.0]
    assert bool((bt == 0).all()) and bool((bwt == 0).all())
    # N = 0: empty outputs, counts of 0
    gt = torch.tensor([[[0, 0, 9, 9], [30, 30, 40, 45], [60, 10, 80, 25]], [[5, 5, 20, 20], [0, 0, 0, 0], [0, 0, 0, 0]]],
                      dtype=torch.float32, device="cuda")
    cnt = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
    got = T.anchor_target(torch.zeros(0, 4, device="cuda"), None, gt, cnt, ish, num=4)
    _clean(guard, [])
    assert got[0].shape == (2, 0) and got[2].shape == (2, 0, 4) and got[4].tolist() == [0, 0] and got[5].tolist() == [0, 0]
    # P = 0 with the ground truths added: each is its own positive, in index order, with a zero target
    lab = torch.tensor([[7, 8, 9], [3, 0, 0]], dtype=torch.int64, device="cuda")
    got = T.sample_rois(torch.zeros(2, 0, 5, device="cuda"), none, gt, lab, cnt, num=8, pos_fraction=0.5)
    _clean(guard, [])
    rois, labels, lw, bt, bwt, inds, npos, nneg = [g.cpu() for g in got]
    assert npos.tolist() == [3, 1] and nneg.tolist() == [0, 0]
    assert torch.equal(rois[:3, 1:], gt[0].cpu()) and rois[:3, 0].tolist() == [0, 0, 0] and bool((rois[3:8, 0] == -1).all())
    assert torch.equal(rois[8, 1:], gt[1, 0].cpu()) and rois[8, 0] == 1 and bool((rois[9:, 0] == -1).all())
    assert labels.tolist() == [7, 8, 9, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0]
    assert inds.tolist() == [0, 1, 2, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, -1]
    assert lw.tolist() == [float(i >= 0) for i in inds.tolist()] and bool((bt == 0).all())
    assert bwt[:, 0].tolist() == lw.tolist()
    # and without them there is no candidate at all
    got = T.sample_rois(torch.zeros(2, 0, 5, device="cuda"), none, gt, lab, cnt, num=8, add_gt_as_proposals=False)
    _clean(guard, [])
    assert got[6].tolist() == [0, 0] and got[7].tolist() == [0, 0] and bool((got[0][:, 0] == -1).all())


def test_every_target_entry_point_ran_under_the_guard():
    """Counts what the three tests above did IN THIS RUN (run the file as a whole): every public wrapper of
    target_ops.py returned under the guard, and every workspace query of the target block of include/tdn.h was
    answered at its exact size (rounded up only to the 256-byte alignment the header asks for)."""
    from torch_detection_amd import target_ops
    public = sorted(n for n, v in vars(target_ops).items()
                    if inspect.isfunction(v) and v.__module__ == target_ops.__name__ and not n.startswith("_"))
    assert public == ["anchor_target", "assign_max_iou", "sample_assigned", "sample_rois"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in ("anchor_target", "assign_max_iou", "sample_rois"):
        assert op in WS_SEEN, op
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256, (op, asked, given)
