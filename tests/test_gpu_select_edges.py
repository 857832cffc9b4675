"""GPU tests of the selection and NMS cores at their structural edges (csrc/select_core.h, csrc/nms_core.h) through every
public entry point that uses them, against the closed forms of tests/select_cases.py ("edge inputs").

Every assertion is on integers or bit patterns; only the sigmoid column of rpn_proposals keeps the 1e-6 of
test_gpu_proposals._check, which also cross-checks the CPU oracle.  tests/test_select_cases_oracle.py shows, without a
GPU, that each input reaches the edge it is named for and that the comparison helpers reject the wrong answers.
"""
import numpy as np
import pytest
import torch

import dense_detect_ref as DD
import detect_ref as D
import fcos_ref as F
import proposal_ref as PR
import select_cases as S
import target_ref as TR
import test_gpu_proposals as TP
from oracle import box_ref as B

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
NMS_PRE_MAX, NUM_MAX, SEG_MAX = 4096, 8192, 4096

ALL = S.key_cases()
K1_4 = S.key_cases("K1", "K2", "K3", "K4")
INT_CASES = [c for c in S.key_cases("K1", "K2", "K3", "K4", "K6") if c["int_ok"] and c["k"] <= NUM_MAX]
RPN_CASES = [c for c in ALL if c["values"] is not None and c["k"] <= NMS_PRE_MAX]
DENSE_CASES = [c for c in K1_4 if c["values"] is not None and c["k"] <= NMS_PRE_MAX and c["n"] > c["k"]]
MC_CASES = [c for c in S.key_cases("K1", "K2", "K3", "K5") if c["values"] is not None and c["k"] < SEG_MAX]
GRAPHS = S.graphs() + S.equal_score_graphs()


def _ids(cases):
    return [c["name"] for c in cases]


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


# ---- sample_assigned ------------------------------------------------------------------------------------------------------
def _sample_rows(case, mode):
    """One image's ``assigned`` row, its caller keys, (num, pos_fraction) and the expected masks and counts."""
    keys, k, n = case["keys"], case["k"], case["n"]
    ck = S.caller_keys(keys)
    i = np.arange(n)
    if mode == "pos":
        assigned, kp, kn, num, frac = np.ones(n, np.int32), k, 0, k, 1.0
    elif mode == "neg":
        assigned, kp, kn, num, frac = np.zeros(n, np.int32), 0, k, k, 0.25
    else:                                  # the family is the positives; every 97th box is a negative, a few are ignored
        assigned = np.where(i % 97 == 50, 0, np.where(i % 389 == 7, -1, 3)).astype(np.int32)
        npos, nneg = int((assigned > 0).sum()), int((assigned == 0).sum())
        kp, kn = min(k, npos - 1), nneg // 2
        num, frac = kp + kn, (kp + 0.5) / (kp + kn)
        assert kp >= 1 and kn >= 1 and int(num * frac) == kp
    pos_keys = np.where(assigned > 0, keys, u32(0)).astype(u32)      # what ClassFetch hands the select: non-members are 0
    neg_keys = np.where(assigned == 0, keys, u32(0)).astype(u32)
    pm = S.mask_of(S.expected(pos_keys, kp)[1], n) if kp else np.zeros(n, np.uint8)
    nm = S.mask_of(S.expected(neg_keys, kn)[1], n) if kn else np.zeros(n, np.uint8)
    assert not (pm & (assigned <= 0)).any() and not (nm & (assigned != 0)).any()
    return assigned, ck, num, frac, (pm, nm, kp, kn)


def _run_sample(T, rows, num, frac):
    assigned = np.stack([r[0] for r in rows])
    ck = np.stack([r[1] for r in rows])
    assert num <= NUM_MAX
    got = [_np(t) for t in T.sample_assigned(_cuda(assigned), num, frac, -1, _cuda(ck))]
    ref = TR.sample_assigned(assigned, num, frac, -1, ck)
    for b, r in enumerate(rows):
        pm, nm, kp, kn = r[4]
        assert (int(got[2][b]), int(got[3][b])) == (kp, kn)
        assert np.array_equal(got[0][b], pm), "pos_mask differs at %s" % np.nonzero(got[0][b] != pm)[0][:6].tolist()
        assert np.array_equal(got[1][b], nm), "neg_mask differs at %s" % np.nonzero(got[1][b] != nm)[0][:6].tolist()
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r)


@pytest.mark.parametrize("case", INT_CASES, ids=_ids(INT_CASES))
def test_sample_assigned_one_image(T, case):
    for mode in ("pos", "neg", "split"):
        if mode == "split" and case["n"] < 200:
            continue
        row = _sample_rows(case, mode)
        if row[2] <= NUM_MAX:
            _run_sample(T, [row], row[2], row[3])


def test_sample_assigned_two_images_different_families(T):
    """num = k at fraction 1: an all-positive image takes its k positives, an all-negative one its k negatives."""
    m = S.mixed_levels()
    for l in range(2):
        for modes in (("pos", "pos"), ("neg", "pos"), ("pos", "neg")):
            rows = [_sample_rows(m["images"][b][l], modes[b]) for b in range(2)]
            _run_sample(T, rows, m["k"], 1.0)


# ---- rpn_proposals --------------------------------------------------------------------------------------------------------
def _rpn_level(values, dtype=torch.float32, channels_last=False):
    """(B, n) logits -> (B, 1, 1, n) cls, zero (B, 4, 1, n) deltas."""
    v = torch.from_numpy(np.ascontiguousarray(values, f32))
    cls = v.reshape(v.shape[0], 1, 1, v.shape[1]).to(dtype).cuda()
    reg = torch.zeros(v.shape[0], 4, 1, v.shape[1], dtype=dtype).cuda()
    if channels_last:
        cls, reg = cls.contiguous(memory_format=torch.channels_last), reg.contiguous(memory_format=torch.channels_last)
    return cls, reg


def _rpn(T, levels, anchors, shape, dtype=torch.float32, channels_last=False, **cfg):
    """``levels``: per level a (B, n_l) array of logits.  Runs test_gpu_proposals._check (oracle, run-to-run, padding)."""
    heads = [_rpn_level(v, dtype, channels_last) for v in levels]
    Bn = levels[0].shape[0]
    with np.errstate(over="ignore"):
        props, aidx, counts = TP._check(T, [h[0] for h in heads], [h[1] for h in heads], [_cuda(a) for a in anchors],
                                        [shape] * Bn, min_bbox_size=0, **cfg)
    return _np(props), _np(aidx), _np(counts)


@pytest.mark.parametrize("case", RPN_CASES, ids=_ids(RPN_CASES))
def test_rpn_proposals_one_level(T, case):
    n, k, v = case["n"], case["k"], case["values"]
    anchors, shape = S.line_anchors(n)
    by_key = S.expected(case["keys"], k)[0]
    forms = [(torch.float32, False)] + ([(torch.bfloat16, True)] if S.bf16_exact(v) else [])
    for dtype, cl in forms:
        props, aidx, counts = _rpn(T, [v[None]], [anchors], shape, dtype, cl, nms_pre=k, nms_post=k, max_num=k, nms_thr=0.7)
        assert counts[0] == k
        S.check_selection(case["keys"], k, by_key=aidx[0, :k])
        assert np.array_equal(props[0, :, :4].view(u32), anchors[by_key].view(u32))
    # the merge: max_num below the survivors -> the second block_topk cuts the same order
    if case["edge"]["family"] in ("K1", "K2") and k >= 4:
        top = k // 2 + 1
        props, aidx, counts = _rpn(T, [v[None]], [anchors], shape, nms_pre=k, nms_post=k, max_num=top, nms_thr=0.7)
        assert counts[0] == top and np.array_equal(aidx[0], by_key[:top])
        assert np.array_equal(props[0, :, :4].view(u32), anchors[by_key[:top]].view(u32))


def test_rpn_proposals_bf16_ran_on_something():
    names = [c["name"] for c in RPN_CASES if S.bf16_exact(c["values"])]
    assert any(n.startswith("K1") for n in names) and any(n.startswith("K2_hi") for n in names)
    assert any(n.startswith("K3_hi") for n in names)


def _merged(cases, k, sizes, top):
    """Expected anchor_idx of one image: per level the k first by key, then the best ``top`` by (key desc, pyramid index)."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    cand = np.concatenate([off[l] + S.expected(c["keys"], k)[1] for l, c in enumerate(cases)])
    keys = np.concatenate([c["keys"] for c in cases])
    full = np.zeros(keys.shape[0], u32)
    full[cand] = keys[cand]
    assert np.all(keys[cand] > 0)
    return S.expected(full, min(top, cand.shape[0]))[0]


def test_rpn_proposals_two_levels_two_images(T):
    m = S.mixed_levels()
    k, sizes = m["k"], m["sizes"]
    anchors = [S.line_anchors(n)[0] for n in sizes]
    anchors[1] = anchors[1] + np.asarray([32, 0, 32, 0], f32)              # level 1 sits between level 0's boxes
    both = np.concatenate(anchors)
    shape = (16, 64 * max(sizes) + 64)
    levels = [np.stack([m["images"][b][l]["values"] for b in range(2)]) for l in range(2)]
    for top in (2 * k, k + 7, 5):
        props, aidx, counts = _rpn(T, levels, anchors, shape, nms_pre=k, nms_post=k, max_num=top, nms_thr=0.7)
        for b in range(2):
            want = _merged(m["images"][b], k, sizes, top)
            assert counts[b] == want.shape[0] and np.array_equal(aidx[b, :counts[b]], want)
            assert np.array_equal(props[b, :counts[b], :4].view(u32), both[want].view(u32))


@pytest.mark.parametrize("n", [65, 1025, 4096])
def test_rpn_proposals_chain_selection_nms_merge(T, n):
    """The G1 chain as anchors under descending logits: selection (nms_pre = n - 1 drops the last), NMS at 0.5 (the even
    anchors survive), merge (max_num below the survivors)."""
    for lead in (False, True):
        g = S.g1_chain(n, lead=lead)
        logits = (g["scores"] / f32(n)).astype(f32)
        kept = g["kept"][g["kept"] < n - 1]
        top = kept.shape[0] - 3
        shape = (16, int(g["boxes"].max()) + 1)
        props, aidx, counts = _rpn(T, [logits[None]], [g["boxes"]], shape, nms_pre=n - 1, nms_post=n, max_num=top, nms_thr=0.5)
        assert counts[0] == top and np.array_equal(aidx[0], kept[:top])
        assert np.array_equal(props[0, :, :4].view(u32), g["boxes"][kept[:top]].view(u32))


# ---- anchor_head_detections / fcos_detections ------------------------------------------------------------------------------
def _dense_expected(images, k, sizes):
    """dense_anchor_idx of a batch: image-major, level-major, each (image, level) ascending."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    return np.concatenate([off[l] + S.expected(c["keys"], k)[1] for cases in images for l, c in enumerate(cases)])


def _anchor_head(T, images, k, sizes):
    L, Bn = len(sizes), len(images)
    cls, reg, anchors = [], [], []
    for l, n in enumerate(sizes):
        c, r = _rpn_level(np.stack([images[b][l]["values"] for b in range(Bn)]))
        cls.append(c)
        reg.append(r)
        anchors.append(_cuda(S.line_anchors(n)[0]))
    shapes = torch.tensor([(16, 64 * max(sizes))] * Bn, dtype=torch.int32).cuda()
    out = T.anchor_head_detections(cls, reg, anchors, shapes, nms_pre=k, score_thr=0.99, max_per_img=100, return_dense=True)
    bidx, aidx = _np(out[6]), _np(out[7])
    assert np.array_equal(bidx, np.repeat(np.arange(Bn), L * k))
    want = _dense_expected(images, k, sizes)
    assert aidx.shape == want.shape and np.array_equal(aidx, want), np.nonzero(aidx != want)[0][:6].tolist()
    # the CPU oracle's per-level selection
    for b in range(Bn):
        for l in range(L):
            ref = DD.kept_anchors(images[b][l]["values"], k)
            assert np.array_equal(aidx[(b * L + l) * k:(b * L + l + 1) * k] - sum(sizes[:l]), ref)


def _rank_logits(keys):
    """Logits in [-4, 4] with the order and the ties of ``keys``, far enough apart for any faithful fp32 sigmoid."""
    uniq, inv = np.unique(keys, return_inverse=True)
    step = 8.0 / max(uniq.shape[0] - 1, 1)
    return (-4.0 + step * inv).astype(f32)


def _fcos(T, images, k, sizes):
    L, Bn = len(sizes), len(images)
    cls, reg, ctr = [], [], []
    for l, n in enumerate(sizes):
        logits = np.stack([_rank_logits(images[b][l]["keys"]) for b in range(Bn)])
        for b in range(Bn):
            # on the CPU first: with a constant centre-ness the key order is the logit order, by a wide margin
            lv = np.unique(logits[b])
            key64 = F.sg(lv) * F.sg(0.0)
            assert lv.shape[0] == np.unique(images[b][l]["keys"]).shape[0]
            assert np.all(np.diff(key64) > 2.0 ** -18 * key64[1:])
            assert np.array_equal(S.order_key(logits[b]).argsort(kind="stable"), images[b][l]["keys"].argsort(kind="stable"))
            assert np.array_equal(F.kept_points(F.sg(logits[b]) * F.sg(0.0), k), S.expected(images[b][l]["keys"], k)[1])
        c, r = _rpn_level(logits)
        cls.append(c)
        reg.append(r)
        ctr.append(torch.zeros(Bn, 1, 1, n).cuda())
    shapes = torch.tensor([(16, 8 * max(sizes))] * Bn, dtype=torch.int32).cuda()
    out = T.fcos_detections(cls, reg, ctr, [8] * L, shapes, nms_pre=k, score_thr=0.99, max_per_img=100, return_dense=True)
    bidx, pidx = _np(out[6]), _np(out[7])
    assert np.array_equal(bidx, np.repeat(np.arange(Bn), L * k))
    want = _dense_expected(images, k, sizes)
    assert pidx.shape == want.shape and np.array_equal(pidx, want), np.nonzero(pidx != want)[0][:6].tolist()


@pytest.mark.parametrize("case", DENSE_CASES, ids=_ids(DENSE_CASES))
def test_dense_heads_one_level(T, case):
    _anchor_head(T, [[case]], case["k"], (case["n"],))
    _fcos(T, [[case]], case["k"], (case["n"],))


def test_dense_heads_two_levels_two_images(T):
    m = S.mixed_levels()
    _anchor_head(T, m["images"], m["k"], m["sizes"])
    _fcos(T, m["images"], m["k"], m["sizes"])


# ---- multiclass_nms -------------------------------------------------------------------------------------------------------
MC_THR = -3.0e38                          # finite, above -FLT_MAX: every other value of the families is a candidate


@pytest.mark.parametrize("case", MC_CASES, ids=_ids(MC_CASES))
def test_multiclass_nms_score_column(T, case):
    """The family as the scores of one class over disjoint boxes, cut into images of at most 4096 rows (a segment's limit):
    per image the best max_num of its candidates by (score desc, row asc)."""
    n, top, v, keys = case["n"], case["k"], case["values"], case["keys"]
    boxes = S.line_anchors(n)[0]
    scores = np.stack([np.zeros(n, f32), v], 1)
    bidx = (np.arange(n) // SEG_MAX).astype(np.int32)
    Bn = int(bidx[-1]) + 1
    dets, labels, rows, counts = [_np(t) for t in T.multiclass_nms(_cuda(boxes), _cuda(scores), _cuda(bidx), Bn, MC_THR,
                                                                    0.5, top)]
    for b in range(Bn):
        mine = np.nonzero((bidx == b) & (v > f32(MC_THR)))[0]
        cnt = min(top, mine.shape[0])
        want = mine[S.expected(keys[mine], cnt)[0]]
        assert counts[b] == cnt
        assert np.array_equal(rows[b, :cnt], want), (b, np.nonzero(rows[b, :cnt] != want)[0][:6].tolist())
        assert np.array_equal(dets[b, :cnt, 4].view(u32), v[want].view(u32))
        assert np.array_equal(dets[b, :cnt, :4].view(u32), boxes[want].view(u32))
        assert np.all(rows[b, cnt:] == -1) and np.all(labels[b, :cnt] == 0) and not dets[b, cnt:].any()
    ref = D.multiclass_nms(boxes, scores, bidx, Bn, MC_THR, 0.5, top)
    assert np.array_equal(rows, ref[2]) and np.array_equal(counts, ref[3])
    assert np.array_equal(dets.view(u32), ref[0].view(u32))


MC_GRAPHS = [S.g1_chain(65), S.g1_chain(1025, lead=True), S.g1_chain(4096)] + [S.g4_dead(t) for t in S.G4_TRIPLES] + \
    [S.g6_threshold(False), S.g6_threshold(True)]


@pytest.mark.parametrize("g", MC_GRAPHS, ids=_ids(MC_GRAPHS))
def test_multiclass_nms_graph_beside_a_disjoint_class(T, g):
    n = g["n"]
    other = S.g5_disjoint(n)
    boxes = np.concatenate([g["boxes"], other["boxes"]], 1)
    scores = np.stack([np.zeros(n, f32), g["scores"], g["scores"]], 1)
    top = min(2 * n, NUM_MAX)
    dets, labels, rows, counts = [_np(t) for t in T.multiclass_nms(_cuda(boxes), _cuda(scores), None, 1, 0.05, g["thr"], top)]
    # survivors: class 0 the graph's kept rows, class 1 every row; order (score desc, class asc, row asc)
    rw = np.concatenate([g["kept"], np.arange(n)])
    cl = np.concatenate([np.zeros(g["kept"].shape[0], np.int64), np.ones(n, np.int64)])
    sel = np.lexsort((rw, cl, -g["scores"][rw].astype(np.float64)))[:top]
    cnt = sel.shape[0]
    assert counts[0] == cnt and np.array_equal(rows[0, :cnt], rw[sel]) and np.array_equal(labels[0, :cnt], cl[sel])
    assert np.all(rows[0, cnt:] == -1)
    want = np.where(cl[sel, None] == 0, g["boxes"][rw[sel]], other["boxes"][rw[sel]])
    assert np.array_equal(dets[0, :cnt, :4].view(u32), want.view(u32))
    assert np.array_equal(dets[0, :cnt, 4].view(u32), g["scores"][rw[sel]].view(u32))


# ---- ops.nms / batched_nms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onewave", ["0", "1"])
@pytest.mark.parametrize("g", GRAPHS, ids=_ids(GRAPHS))
def test_nms_graphs(T, g, onewave, monkeypatch):
    monkeypatch.setenv("TDN_NMS_ONEWAVE", onewave)
    equal = bool(np.all(g["scores"] == g["scores"][0])) and g["n"] > 1
    for h in ([g] if equal else [g, S.shuffled(g)]):
        keep, kept, num = T.ops.nms(_cuda(h["boxes"]), _cuda(h["scores"]), h["thr"])
        assert num.shape == (1,)
        S.check_keep(h, _np(keep), _np(kept), int(num.item()))
        if h["n"] <= 1100:                                                 # the C oracle, cheap at this size
            kr, ki, c = B.nms(h["boxes"], h["scores"], h["thr"])
            assert c == int(num.item()) and np.array_equal(_np(keep), kr) and np.array_equal(_np(kept), ki)


def _segments(thr_strict):
    g6 = S.g6_threshold(thr_strict)
    segs = [S.g1_chain(65), None, S.g3_long(64, False), S.g4_dead((62, 63, 64)), S.g4_dead((5, 1029, 2053)),
            S.g2_cover(4096), g6, S.shuffled(S.g1_chain(1025, lead=True))]
    return segs, g6["thr"]


@pytest.mark.parametrize("strict", [False, True])
def test_batched_nms_segments_of_different_graphs(T, strict):
    """Different graphs laid end to end, an empty segment among them: every segment's result is its own closed form, so
    neither the mask pitch nor the start offset leaks from one segment into the next."""
    segs, thr = _segments(strict)
    sizes = [0 if g is None else g["n"] for g in segs]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    boxes = np.concatenate([g["boxes"] for g in segs if g is not None])
    scores = np.concatenate([g["scores"] for g in segs if g is not None])
    ref = PR.batched_nms(boxes, scores, off, thr)
    for seg in (torch.from_numpy(off), torch.from_numpy(off).cuda()):
        keep, kept, counts = [_np(t) for t in T.batched_nms(_cuda(boxes), _cuda(scores), seg, thr)]
        for s, g in enumerate(segs):
            a, b = off[s], off[s + 1]
            if g is None:
                assert counts[s] == 0
                continue
            local = np.where(kept[a:b] >= 0, kept[a:b] - a, -1)
            assert np.all(kept[a:b][kept[a:b] >= 0] >= a)
            S.check_keep(g, keep[a:b], local, counts[s])
        assert np.array_equal(keep, ref[0]) and np.array_equal(kept, ref[1]) and np.array_equal(counts, ref[2])
