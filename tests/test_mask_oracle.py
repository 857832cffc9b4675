"""CPU tests that pin tests/mask_ref.py, the oracle of the mask-branch kernels: hand cases, exact
rational arithmetic, float64 and matplotlib for the targets; torch float64 autograd for the loss; hand cases for the
paste; pack_polygons; and the host refusals that need no GPU."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import mask_cases as MC
import mask_ref as R

F32 = np.float32


def _mask(box, polys, M):
    return R.instance_mask(box, [np.asarray(p, F32).reshape(-1, 2) for p in polys], M).astype(int)


# ---- targets: hand cases ---------------------------------------------------------------------------------------------
def test_rectangle_covers_the_cells_whose_centres_it_holds():
    # box (0, 0) 8 x 8, M = 4: centres at 1, 3, 5, 7; the rectangle [2, 6] x [0, 4] holds x in {3, 5}, y in {1, 3}
    m = _mask((0, 0, 8, 8), [[2, 0, 6, 0, 6, 4, 2, 4]], 4)
    want = np.zeros((4, 4), int)
    want[0:2, 1:3] = 1
    assert np.array_equal(m, want)


def test_triangle():
    # (0,0) (8,0) (0,8): centre (x, y) is inside iff x + y < 8 -> (1,1) (3,1) (5,1) (1,3) (3,3) (1,5); x + y = 8 is the
    # hypotenuse itself: px < xi is strict, so (1,7), (3,5), (5,3), (7,1) are outside
    m = _mask((0, 0, 8, 8), [[0, 0, 8, 0, 0, 8]], 4)
    assert np.array_equal(m, np.array([[1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]))


def test_concave_polygon():
    # a U: the notch [3, 5] x [0, 6] is cut out of [0, 8] x [0, 8]; M = 8 centres at 0.5 .. 7.5
    u = [0, 0, 3, 0, 3, 6, 5, 6, 5, 0, 8, 0, 8, 8, 0, 8]
    m = _mask((0, 0, 8, 8), [u], 8)
    want = np.ones((8, 8), int)
    want[0:6, 3:5] = 0
    assert np.array_equal(m, want)


def test_two_parts_are_a_union_also_where_they_overlap():
    a, b, c = [0, 0, 4, 0, 4, 4, 0, 4], [6, 6, 8, 6, 8, 8, 6, 8], [2, 2, 6, 2, 6, 6, 2, 6]
    disjoint = _mask((0, 0, 8, 8), [a, b], 8)
    want = np.zeros((8, 8), int)
    want[0:4, 0:4] = 1
    want[6:8, 6:8] = 1
    assert np.array_equal(disjoint, want)
    overlap = _mask((0, 0, 8, 8), [a, c], 8)
    want = np.zeros((8, 8), int)
    want[0:4, 0:4] = 1
    want[2:6, 2:6] = 1                                   # [2, 4]^2 lies in both parts and stays 1: union, not XOR
    assert np.array_equal(overlap, want)
    # one self-overlapping polygon is even-odd: the doubly wound region is OUT
    twice = _mask((0, 0, 8, 8), [a + a], 8)
    assert twice.sum() == 0


def test_vertex_on_a_cell_centre_row():
    # M = 4 over (0, 0) 8 x 8: centre rows at y = 1, 3, 5, 7.  The diamond's left and right vertices lie ON the row
    # y = 3.  `ya > py` is false for a vertex on the row, so that vertex counts as BELOW-or-on: of the two edges that
    # meet at (1, 3) only the one coming from y > 3 straddles the row, and the row is crossed once at each end.
    diamond = [4, 0, 7, 3, 4, 6, 1, 3]
    m = _mask((0, 0, 8, 8), [diamond], 4)
    # row y = 3: crossings at x = 1 and x = 7: centres 3 and 5 are inside; centre 1 is ON the left vertex: px < xi is
    # false for xi = 1 (left crossing) and true for xi = 7, one flip: inside.  Centre 7 is ON the right vertex: no flip.
    assert m[1].tolist() == [1, 1, 1, 0]
    # rows y = 1 and y = 5 cross at x = 3 and x = 5: the centre ON the left edge is in, the one ON the right edge is out
    assert m[0].tolist() == [0, 1, 0, 0] and m[2].tolist() == [0, 1, 0, 0] and m[3].tolist() == [0, 0, 0, 0]


def test_degenerate_polygons_contribute_nothing_and_nan_only_fails_comparisons():
    assert _mask((0, 0, 8, 8), [[0, 0, 8, 8]], 4).sum() == 0
    assert _mask((0, 0, 8, 8), [[0, 0, 8, 8], [0, 0, 8, 0, 0, 8]], 4).sum() == 6
    nan = float("nan")
    m = _mask((0, 0, 8, 8), [[nan, nan, 8, 0, 0, 8], [0, 0, 8, 0, 8, 8, 0, 8]], 4)
    assert np.array_equal(m, np.ones((4, 4), int))       # a NaN vertex only takes its own two edges out of the count
    assert _mask((0, 0, 8, 8), [[nan, nan, nan, 0, 0, nan]], 4).sum() == 0


def test_box_truncation_and_minimum_extent():
    assert R.int_box(np.array([10.9, -3.7, 20.2, 5.99], F32)) == (10, -3, 11, 9)
    assert R.int_box(np.array([30, 20, 25, 15], F32)) == (30, 20, 1, 1)
    assert R.int_box(np.array([np.nan, 3e9, -3e9, np.nan], F32)) == (0, 2 ** 31 - 1, 1, 1)
    assert R.row_batch(np.nan, 2) is None and R.row_batch(-1, 2) is None and R.row_batch(2, 2) is None
    assert R.row_batch(-0.5, 2) == 0 and R.row_batch(1.9, 2) == 1


# ---- targets: exact arithmetic, float64, matplotlib ------------------------------------------------------------------
def _inside_fraction(px, py, poly):
    inside = False
    n = len(poly)
    for k in range(n):
        (xa, ya), (xb, yb) = poly[k], poly[(k + 1) % n]
        if (ya > py) != (yb > py) and px < xa + (py - ya) * (xb - xa) / (yb - ya):
            inside = not inside
    return inside


@pytest.mark.parametrize("M", [28, 7, 1])
def test_exact_arithmetic_inputs_equal_a_rational_evaluation(M):
    rois, inds = MC.target_rows(M)
    poly = [(Fraction(int(x)), Fraction(int(y))) for x, y in MC.EXACT_POLY]
    seen = 0
    for r in MC.EXACT_ROWS:
        x1, y1, w, h = R.int_box(rois[r, 1:])
        assert w % (2 * M) == 0 and h % (2 * M) == 0
        got = R.instance_mask((x1, y1, w, h), [MC.EXACT_POLY], M)
        want = np.array([[_inside_fraction(x1 + Fraction((2 * j + 1) * w, 2 * M), y1 + Fraction((2 * i + 1) * h, 2 * M),
                                           poly) for j in range(M)] for i in range(M)])
        assert np.array_equal(got, want), r
        seen += int(want.sum())
    assert seen > 0


def _random_stars(n, seed):
    g = np.random.default_rng(seed)
    for k in range(n):
        nv = int(g.integers(3, 40))
        poly = MC.star(100 + g.uniform(-5, 5), 80 + g.uniform(-5, 5), 10, 60, nv, 1000 * seed + k)
        x1, y1 = poly.min(0) - g.uniform(0, 8, 2)
        x2, y2 = poly.max(0) + g.uniform(0, 8, 2)
        yield poly, R.int_box(np.array([x1, y1, x2, y2], F32))


def test_random_star_polygons_against_float64():
    M, differ, total = 28, 0, 0
    for poly, box in _random_stars(400, 7):
        a = R.instance_mask(box, [poly], M)
        b = R.instance_mask(box, [poly], M, dtype=np.float64)
        differ += int((a != b).sum())
        total += M * M
        assert 0 < a.sum() < M * M
    print("float32 vs float64: %d of %d cells differ" % (differ, total))
    assert differ * 10 ** 4 <= total


def test_random_star_polygons_against_matplotlib():
    path = pytest.importorskip("matplotlib.path")
    M, differ, total = 28, 0, 0
    for poly, box in _random_stars(400, 7):
        a = R.instance_mask(box, [poly], M)
        px, py = R.cell_centres(box, M)
        pts = np.stack(np.meshgrid(px.astype(np.float64), py.astype(np.float64)), -1).reshape(-1, 2)
        b = path.Path(poly.astype(np.float64)).contains_points(pts).reshape(M, M)
        differ += int((a != b).sum())
        total += M * M
    print("float32 vs matplotlib: %d of %d cells differ" % (differ, total))
    assert differ * 10 ** 3 <= total


@pytest.mark.parametrize("M", [28, 7, 1])
def test_batch_targets_and_pack_polygons(M):
    import torch_detection_amd as T
    xy, po, gpo = (t.numpy() for t in T.pack_polygons(MC.target_polys(), MC.G))
    assert xy.dtype == F32 and po.dtype == np.int32 and gpo.dtype == np.int32
    assert gpo.tolist() == [[0, 1, 3, 6], [6, 6, 7, 7]] and po[1] == 700 and po[-1] == xy.shape[0]
    rois, inds = MC.target_rows(M)
    t, w = R.mask_target(rois, inds, xy, po, gpo, M)
    assert t.shape == (40, M, M) and t.dtype == np.uint8 and w.dtype == F32
    for r in (3, 5, 7, 9, 13):                           # invalid rows
        assert w[r] == 0 and t[r].sum() == 0, r
    for r in (19, 23):                                   # valid, but nothing to draw
        assert w[r] == 1 and t[r].sum() == 0, r
    assert w[15] == 1 and w[17] == 1 and w[25] == 1      # NaN / huge coordinates are a box like any other
    if M == 28:
        full = [r for r in range(40) if r % 5 == 0 and r not in (5, 15, 25)]
        assert all(0 < t[r].sum() < M * M for r in full)
        assert all(t[r].sum() == 0 for r in range(40) if r % 5 == 3 and r not in MC.EXACT_ROWS)


def test_pack_polygons_refusals():
    import torch_detection_amd as T
    with pytest.raises(ValueError, match="more than G"):
        T.pack_polygons([[[[0, 0, 1, 0, 0, 1]]] * 3], 2)
    with pytest.raises(ValueError, match="at least 6"):
        T.pack_polygons([[[[0, 0, 1, 1]]]], 2)
    xy, po, gpo = T.pack_polygons([[], []], 0)
    assert xy.shape == (0, 2) and po.tolist() == [0] and gpo.tolist() == [[0], [0]]


# ---- loss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", [(5, 7), (1, 7), (5, 28)])
@pytest.mark.parametrize("avg", [None, 3.5])
def test_loss_and_gradient_against_torch_float64(C, M, avg):
    import torch.nn.functional as F
    pred, targets, labels, w = MC.loss_case(24, C, M, 3)
    ref = R.mask_head_loss(pred, targets, labels, w, avg, g=1.5)
    ch, ok = R.row_channels(labels, C)
    live = (w != 0) & ok
    assert live.sum() > 3 and (~live).sum() > 3
    x = torch.from_numpy(pred).double()
    x = torch.where(torch.from_numpy(live)[:, None, None, None], x, torch.zeros_like(x)).requires_grad_(True)
    rows = torch.arange(24)[torch.from_numpy(live)]
    sl = x[rows, torch.from_numpy(ch)[rows]]
    per = F.binary_cross_entropy_with_logits(sl, torch.from_numpy(targets[live]).double(), reduction="none")
    D = float(avg) if avg is not None else max(int((w > 0).sum()), 1)
    loss = (per.sum((1, 2)) * torch.from_numpy(w[live]).double()).sum() / (D * M * M)
    (1.5 * loss).backward()
    assert float(ref["avg"]) == D
    assert abs(ref["loss"] - loss.item()) <= 1e-12 * abs(loss.item())
    assert np.allclose(ref["dpred"], x.grad.numpy(), rtol=1e-11, atol=1e-300)
    assert np.array_equal(ref["dpred"] != 0, x.grad.numpy() != 0)


def test_loss_with_all_weights_zero():
    pred, targets, labels, w = MC.loss_case(24, 5, 7, 4, all_zero=True)
    ref = R.mask_head_loss(pred, targets, labels, w)
    assert ref["loss"] == 0 and float(ref["avg"]) == 1 and not ref["dpred"].any()


# ---- paste -----------------------------------------------------------------------------------------------------------
def _paste(logit, det, M=4, thr=0.5, canvas=(12, 16), img=None):
    pred = np.full((1, 1, M, M), logit, F32) if np.isscalar(logit) else logit
    dets = np.array([[list(det) + [1.0]]], F32)
    m, v = R.mask_head_masks(pred, dets, np.zeros((1, 1), np.int64), np.array([1], np.int32), canvas,
                             None if img is None else np.array([img], np.int32), thr)
    return m[0], v[0]


def test_paste_constant_logits():
    m, _ = _paste(8.0, (3, 2, 10, 9))
    want = np.zeros((12, 16), np.uint8)
    want[2:10, 3:11] = 1                                 # the whole box [x1, x1 + w) x [y1, y1 + h)
    assert np.array_equal(m, want)
    assert _paste(-8.0, (3, 2, 10, 9))[0].sum() == 0
    # sigma(0) = 0.5 exactly; w = h = 8 = 2M makes every sample position a dyadic number, so v = 0.5 exactly: `>` fails
    m, v = _paste(0.0, (3, 2, 10, 9))
    assert m.sum() == 0 and np.all(v[2:10, 3:11] == 0.5)
    assert _paste(0.0, (3, 2, 10, 9), thr=0.4999)[0].sum() == 64


def test_paste_small_and_inverted_boxes():
    m, _ = _paste(8.0, (5, 4, 5, 4))
    assert m.sum() == 1 and m[4, 5] == 1                 # w = h = 1
    m, _ = _paste(8.0, (9, 7, 2, 1))
    assert m.sum() == 1 and m[7, 9] == 1                 # x2 < x1: still one pixel at (x1, y1)


def test_paste_boxes_over_the_edges_and_the_image_size():
    for det, rows, cols in (((-4, -3, 5, 6), (0, 7), (0, 6)), ((10, 8, 30, 30), (8, 12), (10, 16)),
                            ((-9, -9, 40, 40), (0, 12), (0, 16))):
        m, _ = _paste(8.0, det)
        want = np.zeros((12, 16), np.uint8)
        want[rows[0]:rows[1], cols[0]:cols[1]] = 1
        assert np.array_equal(m, want), det
    m, _ = _paste(8.0, (-9, -9, 40, 40), img=(5, 7))
    assert m.sum() == 35 and m[:5, :7].all()


def test_paste_interpolates_between_cell_centres():
    # M = 2 over an 8-wide box: samples at ((x + 0.5) * 2) / 8 - 0.5 = -0.375, -0.125, 0.125 .. 1.375 -> clamped at 0,
    # and at M - 1 = 1 from x0 >= 1 on (both corners M - 1, fraction 0)
    pred = np.zeros((1, 1, 2, 2), F32)
    pred[0, 0, :, 1] = 20.0                              # left column sigma = 0.5, right column ~ 1
    _, v = _paste(pred, (0, 0, 7, 7), M=2, canvas=(8, 8))
    want = 0.5 + 0.5 * np.array([0, 0, 0.125, 0.375, 0.625, 0.875, 1, 1])
    assert np.allclose(v[0], want, atol=1e-8) and np.allclose(v[7], want, atol=1e-8)


@pytest.mark.parametrize("C", [4, 1])
@pytest.mark.parametrize("M", [28, 14])
def test_shared_paste_inputs_stay_clear_of_the_threshold(C, M):
    """What tests/test_gpu_mask.py relies on: in every variant it runs (the logits as stored in each dtype, with and
    without the images' own sizes) at most 1 box pixel in 10^4 lies within K_PASTE x 2^-24 of the threshold."""
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        stored = torch.from_numpy(MC.paste_pred(C, M).copy()).to(dt).float().numpy()
        for shapes in (MC.PASTE_IMG_SHAPES, None):
            m, v = R.mask_head_masks(stored, MC.PASTE_DETS, MC.PASTE_LABELS, MC.PASTE_COUNTS, MC.CANVAS, shapes, 0.5)
            n = MC.box_pixels(v)
            near = int(MC.near_threshold(v, 0.5).sum())
            print("C=%d M=%d %s: %d box pixels, %d within %d x 2^-24 of the threshold, %d set" % (
                C, M, dt, n, near, MC.K_PASTE, m.sum()))
            assert n > 20000 and near * 10 ** 4 <= n
            assert 0.1 * n < m.sum() < 0.9 * n
    m, v = R.mask_head_masks(MC.paste_pred(C, M), MC.PASTE_DETS, MC.PASTE_LABELS, MC.PASTE_COUNTS, MC.CANVAS,
                             MC.PASTE_IMG_SHAPES, 0.5)
    assert not m[10].any() and not m[11].any()           # past counts[1]
    assert not m[6][50:].any() and not m[6][:, 100:].any() and m[6].any()      # the image's own size
    if C == 4:
        assert not m[8].any()                            # label 3 has no channel in a C = 4 head
    assert np.array_equal(np.unpackbits(R.pack_bits(m), axis=-1, bitorder="little")[..., :150], m)
    assert R.pack_bits(m).shape == (12, 70, 24)


def test_rois_from_detections_restatement():
    out = R.rois_from_detections(MC.PASTE_DETS, np.array([6, -1], np.int32), np.array([2.0, 0.5], F32))
    assert out.shape == (12, 5) and np.array_equal(out[0], np.array([0, 40.6, 21.8, 120.4, 81.0], F32))
    assert np.array_equal(out[6:], np.tile(np.array([-1, 0, 0, 0, 0], F32), (6, 1)))


# ---- host refusals that need no GPU ----------------------------------------------------------------------------------
def test_value_errors_without_a_gpu():
    import torch_detection_amd as T
    z = torch.zeros
    rois, inds = z(4, 5), z(4, dtype=torch.int32)
    xy, po, gpo = T.pack_polygons(MC.target_polys(), MC.G)
    pred, tg, lab, w = z(4, 3, 7, 7), z(4, 7, 7, dtype=torch.uint8), z(4, dtype=torch.int64), z(4)
    dets, dl, cnt = z(2, 2, 5), z(2, 2, dtype=torch.int64), z(2, dtype=torch.int32)
    cases = [
        (lambda: T.mask_target(rois, inds, xy, po, gpo, mask_size=57), "mask_size must be in 1..56"),
        (lambda: T.mask_target(rois, inds, xy, po, gpo, mask_size=0), "mask_size must be in 1..56"),
        (lambda: T.mask_target(rois.double(), inds, xy, po, gpo), "rois must be a contiguous float32"),
        (lambda: T.mask_target(rois, inds.long(), xy, po, gpo), "pos_assigned_gt_inds must be a contiguous int32"),
        (lambda: T.mask_target(rois, inds[:3], xy, po, gpo), "pos_assigned_gt_inds must be"),
        (lambda: T.mask_target(rois, inds, xy.t(), po, gpo), "poly_xy must be"),
        (lambda: T.mask_target(rois, inds, xy, po, gpo), "rois must be a CUDA tensor"),
        (lambda: T.mask_head_loss(pred.double(), tg, lab, w), "mask_pred must be a float32 / bfloat16 / float16"),
        (lambda: T.mask_head_loss(z(4, 3, 7, 8), tg, lab, w), "mask_pred must be"),
        (lambda: T.mask_head_loss(z(4, 3, 57, 57), z(4, 57, 57, dtype=torch.uint8), lab, w), "M in 1..56"),
        (lambda: T.mask_head_loss(pred.permute(0, 1, 3, 2), tg, lab, w), "NCHW-contiguous or channels_last"),
        (lambda: T.mask_head_loss(pred, tg[:3], lab, w), "mask_targets must be"),
        (lambda: T.mask_head_loss(pred, tg.float(), lab, w), "mask_targets must be a contiguous uint8"),
        (lambda: T.mask_head_loss(pred, tg, lab.int(), w), "labels must be a contiguous int64"),
        (lambda: T.mask_head_loss(pred, tg, lab, w[:2]), "mask_weights must be"),
        (lambda: T.mask_head_loss(pred, tg, lab, w, avg_factor=-1.0), "avg_factor must be finite and > 0"),
        (lambda: T.mask_head_loss(pred, tg, lab, w), "mask_pred must be a CUDA tensor"),
        (lambda: T.rois_from_detections(dets[..., :4], cnt), "dets must be"),
        (lambda: T.rois_from_detections(dets, cnt[:1]), "counts must be"),
        (lambda: T.rois_from_detections(dets, cnt, scale_factors=0.0), "scale_factors must be finite and > 0"),
        (lambda: T.rois_from_detections(dets, cnt), "dets must be a CUDA tensor"),
        (lambda: T.mask_head_masks(pred[:3], dets, dl, cnt, (8, 8)), "mask_pred must be"),
        (lambda: T.mask_head_masks(pred, dets, dl.int(), cnt, (8, 8)), "labels must be a contiguous int64"),
        (lambda: T.mask_head_masks(pred, dets, dl, cnt, (0, 8)), r"out_shape\[0\] must be in"),
        (lambda: T.mask_head_masks(pred, dets, dl, cnt, 8), "out_shape must be"),
        (lambda: T.mask_head_masks(pred, dets, dl, cnt, (8, 8), img_shapes=z(2, 2)), "img_shapes must be"),
        (lambda: T.mask_head_masks(pred, dets, dl, cnt, (8, 8), thr=float("nan")), "thr must be finite"),
        (lambda: T.mask_head_masks(pred, dets, dl, cnt, (8, 8)), "mask_pred must be a CUDA tensor"),
    ]
    for fn, msg in cases:
        with pytest.raises(ValueError, match=msg):
            fn()
