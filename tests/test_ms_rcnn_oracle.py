"""CPU: the oracle of Mask Scoring R-CNN (tests/ms_rcnn_ref.py) against independent statements of the
same mathematics — torch float64 autograd for the first layer, the brute-force point test and exact rational arithmetic
for the target's bitmaps, mmdetection's numpy-slice formula, torch's ``mse_loss`` — and, without a GPU, the module
(registry, state-dict keys, shapes, init, refusals) and every ValueError of the wrappers."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import mask_cases as MC
import mask_ref as MR
import ms_rcnn_cases as K
import ms_rcnn_ref as R

F32 = np.float32


# ---- the first layer ---------------------------------------------------------------------------------------------------
def _torch_stem(feats, pred, labels, weight, bias, label_offset, relu, gy):
    """cat(feats, max_pool2d(sigmoid(pred[r, ch_r]))) -> conv2d -> relu in float64 autograd."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    f, w, b = t(feats).requires_grad_(True), t(weight).requires_grad_(True), t(bias).requires_grad_(True)
    x = torch.from_numpy(np.nan_to_num(np.asarray(pred, np.float64))).requires_grad_(True)
    ch, ok = R.stem_channels(labels, pred.shape[1], label_offset)
    rows = torch.arange(pred.shape[0])
    sel = torch.sigmoid(x[rows, torch.from_numpy(ch)]) * torch.from_numpy(ok.astype(np.float64))[:, None, None]
    P = TF.max_pool2d(sel[:, None], 2, 2)
    z = TF.conv2d(torch.cat([f, P], 1), w, b, 1, 1)
    y = torch.relu(z) if relu else z
    y.backward(t(gy))
    return y.detach().numpy(), f.grad.numpy(), x.grad.numpy(), w.grad.numpy(), b.grad.numpy(), P.detach().numpy()[:, 0]


@pytest.mark.parametrize("S,C,off,relu", [(14, 5, 0, True), (2, 5, 0, False), (1, 5, 0, True), (4, 1, 0, True),
                                          (3, 5, 1, True)])
def test_stem_oracle_equals_torch_autograd(S, C, off, relu):
    feats, pred, labels, weight, bias, gy = K.stem_case(S, C, 100 + S)
    labels = labels - off
    ref = R.stem(feats, pred, labels, weight, bias, off, relu, gy)
    y, df, dx, dw, db, P = _torch_stem(feats, pred, labels, weight, bias, off, relu, gy)
    for name, a, b in (("y", ref["y"], y), ("P", ref["P"], P), ("dfeats", ref["dfeats"], df),
                       ("dpred", ref["dpred"], dx), ("dweight", ref["dweight"], dw), ("dbias", ref["dbias"], db)):
        assert a.shape == b.shape, name
        assert np.allclose(a, b, rtol=1e-11, atol=1e-13), (name, float(np.abs(a - b).max()))
    assert np.abs(ref["dpred"]).sum() > 0 and np.abs(ref["dweight"][:, -1]).sum() > 0
    # exact zeros off the rows' channels and off the windows' maxima: one element per window at most
    assert (np.count_nonzero(ref["dpred"].reshape(pred.shape[0], -1), 1) <= S * S).all()
    if C > 1:
        assert not ref["dpred"][[2, 5]].any() and not ref["P"][[2, 5]].any() and (ref["idx"][[2, 5]] == -1).all()


def test_stem_oracle_ties_go_to_the_first_element():
    feats, pred, labels, weight, bias, gy = K.stem_case(4, 5, 7)
    ref = R.stem(feats, pred, labels, weight, bias, 0, False, gy)
    assert ref["idx"][0, 0, 0] == 0 and ref["idx"][0, 3, 3] == 0 and ref["idx"][1, 0, 0] == 1
    assert ref["P"][0, 0, 0] == 1.0 and 0 < ref["P"][0, 3, 3] < 1e-17
    # float32 sigma of +40 is exactly 1, of -40 a normal number: whole windows tie either way
    assert F32(1) / (F32(1) + np.exp(F32(-40))) == F32(1)
    d = ref["dpred"]
    for r, (y0, x0), hot in ((0, (0, 0), (0, 0)), (0, (6, 6), (6, 6)), (1, (0, 0), (0, 1))):
        win = d[r, labels[r], y0:y0 + 2, x0:x0 + 2]
        assert np.count_nonzero(win) <= 1 and (win[hot[0] - y0, hot[1] - x0] != 0 or not win.any())
    # this build's max_pool2d breaks ties the same way: its gradient lands on the same elements
    # (torch's sigmoid gradient p (1 - p) is an exact 0 at +40 where sigma(x) sigma(-x) is not: that window is looked
    # at through the pooling indices instead)
    _, _, dx, _, _, _ = _torch_stem(feats, pred, labels, weight, bias, 0, False, gy)
    soft = np.abs(np.nan_to_num(pred)) < 40
    assert np.array_equal((dx != 0) & soft, (d != 0) & soft)
    for dt in (torch.float32, torch.float64):
        p = torch.sigmoid(torch.from_numpy(pred[:2, labels[0]].copy()).to(dt))[:, None]
        _, where = TF.max_pool2d(p, 2, 2, return_indices=True)
        assert where[0, 0, 0, 0] == 0 and where[0, 0, 3, 3] == 6 * 8 + 6


# ---- the target ------------------------------------------------------------------------------------------------------
def _brute_bitmap(polys, h, w):
    px = np.arange(w).astype(F32) + F32(0.5)
    py = np.arange(h).astype(F32) + F32(0.5)
    out = np.zeros((h, w), bool)
    for p in polys:
        for y0 in range(0, h, 32):                      # rows in chunks: inside_polygon holds (edges, rows, w) at once
            out[y0:y0 + 32] |= MR.inside_polygon(px, py[y0:y0 + 32], p)
    return out


def test_bitmaps_equal_the_brute_force_point_test():
    xy, po, gpo = (t.numpy() for t in K.packed_polys())
    seen = 0
    for b in range(2):
        h, w = (int(v) for v in K.CANVASES[b])
        for g in range(MC.G):
            polys = MR.instance_polys(xy, po, gpo, b, g)
            got = R.instance_bitmap(polys, h, w)
            want = _brute_bitmap(polys, h, w)
            assert np.array_equal(got, want), (b, g, int((got != want).sum()))
            seen += int(got.sum())
    assert seen > 10000


def test_exact_polygon_full_count_in_rational_arithmetic():
    poly = [(Fraction(int(x)), Fraction(int(y))) for x, y in MC.EXACT_POLY]
    half = Fraction(1, 2)
    count = 0
    for y in range(30, 165):
        for x in range(90, 225):
            px, py, par = x + half, y + half, 0
            for (xa, ya), (xb, yb) in zip(poly, poly[1:] + poly[:1]):
                if (ya > py) != (yb > py) and px < xa + (py - ya) * (xb - xa) / (yb - ya):
                    par ^= 1
            count += par
    bitmap = R.instance_bitmap([MC.EXACT_POLY], 200, 260)
    assert int(bitmap.sum()) == count and count > 5000
    assert not bitmap[:30].any() and not bitmap[165:].any() and not bitmap[:, :90].any() and not bitmap[:, 225:].any()


def test_target_oracle_on_the_shared_rows():
    xy, po, gpo = (t.numpy() for t in K.packed_polys())
    rois, inds, targets, pred, labels = K.target_case(28)
    iou, info = R.mask_iou_target(rois, inds, xy, po, gpo, pred, labels, targets, K.CANVASES, 0.5)
    valid = info["valid"] == 1
    pos = iou > 0
    print("valid %d, positive %d, range %.4g .. %.4g, den == 0 on %d valid rows, full == 0 on %d" % (
        valid.sum(), pos.sum(), iou[pos].min(), iou[pos].max(), int((valid & (info["den"] == 0)).sum()),
        int((valid & (info["full"] == 0)).sum())))
    assert valid.sum() >= 30 and 2 * pos.sum() >= valid.sum() and not pos[~valid].any()
    assert np.all(iou[pos] <= 1) and np.all(np.isfinite(iou))
    assert valid[K.DEN0_ROW] and info["den"][K.DEN0_ROW] == 0 and iou[K.DEN0_ROW] == 0
    assert valid[K.FULL0_ROW] and info["full"][K.FULL0_ROW] == 0 and info["den"][K.FULL0_ROW] > 0
    assert not valid[list(K.BAD_LABEL_ROWS)].any()
    # counts against the brute-force bitmap, and mmdetection's formula on the boxes that lie inside their canvas
    checked = 0
    maps = {}
    for r in np.nonzero(valid)[0]:
        b, g = int(rois[r, 0]), int(inds[r])
        h, w = (int(v) for v in K.CANVASES[b])
        if (b, g) not in maps:
            maps[(b, g)] = _brute_bitmap(MR.instance_polys(xy, po, gpo, b, g), h, w)
        gt_mask = maps[(b, g)]
        assert info["full"][r] == gt_mask.sum()
        x1, y1, x2, y2 = (int(t) for t in MR.trunc_sat(rois[r, 1:]))
        if not (0 <= x1 <= x2 < w and 0 <= y1 <= y2 < h):
            continue
        assert info["inside"][r] == gt_mask[y1:y2 + 1, x1:x2 + 1].sum()
        ratio = F32(gt_mask[y1:y2 + 1, x1:x2 + 1].sum() / (gt_mask.sum() + 1e-7))     # numpy float64, then .float()
        mp = torch.from_numpy((pred[r, labels[r]] > 0.5).astype(F32))
        mt = torch.from_numpy(targets[r].astype(F32))
        want = (mp * mt).sum() / (mp.sum() + mt.sum() / (torch.tensor(ratio) + 1e-7) - (mp * mt).sum())
        want = 0.0 if torch.isnan(want) else float(want)
        assert abs(float(iou[r]) - want) <= 4 * 2.0 ** -24 * max(want, 1e-30), (r, float(iou[r]), want)
        checked += 1
    assert checked >= 10


def test_box_counts_clip_like_a_numpy_slice():
    bitmap = np.ones((5, 9), bool)
    for box, want in (([2, 1, 4, 3], 9), ([-3, -3, 1, 1], 4), ([7, 3, 20, 20], 4), ([4, 4, 2, 2], 0), ([9, 0, 12, 4], 0),
                      ([0, 5, 8, 9], 0), ([-9, -9, -1, -1], 0), ([np.nan, 0, 0.9, np.nan], 1), ([3e9, 0, 3e9, 4], 0),
                      ([-3e9, -3e9, 3e9, 3e9], 45)):
        assert R.box_counts(bitmap, np.array(box, F32)) == (45, want), box


# ---- the loss and the scores -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,C", [(24, 5), (300, 81), (1, 2), (5, 1)])
def test_loss_oracle_equals_torch_mse(R_, C):
    pred, labels, targets = K.loss_case(R_, C, 3 * R_ + C)
    ref = R.mask_iou_loss(pred, labels, targets, 0.5, g=1.5)
    live = ref["live"]
    assert C == 1 or R_ < 5 or (live.any() and not live.all())
    p = torch.from_numpy(np.nan_to_num(pred.astype(np.float64), posinf=0, neginf=0)).requires_grad_(True)
    if live.any():
        rows = torch.from_numpy(np.nonzero(live)[0])
        sel = p[rows, torch.from_numpy(labels[live])]
        loss = 0.5 * TF.mse_loss(sel, torch.from_numpy(targets[live].astype(np.float64)))
        (1.5 * loss).backward()
        assert abs(ref["loss"] - float(loss.detach())) <= 1e-14 * max(float(loss.detach()), 1)
        assert np.allclose(ref["dpred"], p.grad.numpy(), rtol=1e-13, atol=0)
    else:
        assert ref["loss"] == 0 and not ref["dpred"].any() and ref["D"] == 1


def test_loss_oracle_without_live_rows():
    pred, labels, targets = K.loss_case(24, 5, 1, none_live=True)
    ref = R.mask_iou_loss(pred, labels, targets)
    assert ref["loss"] == 0 and ref["D"] == 1 and not ref["dpred"].any() and np.isnan(pred).any()


def test_scores_oracle():
    pred, dets, labels, counts = K.scores_case(5)
    s = R.mask_scores(pred, dets, labels, counts)
    assert not s[0].any() and not s[2].any()
    assert s[1, 0] == 0 and s[1, 1] == 0 and s[1, 2] == 0
    assert s[1, 3] == pred[6 + 3, 0] * dets[1, 3, 4] and s[1, 4] == pred[6 + 4, labels[1, 4] + 1] * dets[1, 4, 4]


# ---- the module ------------------------------------------------------------------------------------------------------
def test_head_registry_keys_shapes_init():
    import torch_detection_amd as T
    assert T.HEADS.module_dict["MaskIoUHead"] is T.MaskIoUHead
    torch.manual_seed(0)
    h = T.MaskIoUHead()
    sd = h.state_dict()
    keys = ["convs.%d.%s" % (i, n) for i in range(4) for n in ("weight", "bias")] + \
           ["fcs.%d.%s" % (i, n) for i in range(2) for n in ("weight", "bias")] + ["fc_mask_iou.weight", "fc_mask_iou.bias"]
    assert list(sd) == keys
    assert tuple(sd["convs.0.weight"].shape) == (256, 257, 3, 3) and tuple(sd["convs.3.weight"].shape) == (256, 256, 3, 3)
    assert [c.stride for c in h.convs] == [(1, 1)] * 3 + [(2, 2)] and all(c.padding == (1, 1) for c in h.convs)
    assert tuple(sd["fcs.0.weight"].shape) == (1024, 256 * 7 * 7) and tuple(sd["fcs.1.weight"].shape) == (1024, 1024)
    assert tuple(sd["fc_mask_iou.weight"].shape) == (81, 1024)
    assert all(not sd[k].any() for k in keys if k.endswith("bias"))
    # kaiming normal (fan_out, relu): std = sqrt(2 / (Cout 9)); kaiming uniform (a = 1, fan_in): bound = sqrt(3 / fan_in)
    assert abs(float(sd["convs.1.weight"].std()) / (2.0 / (256 * 9)) ** 0.5 - 1) < 0.02
    bound = (3.0 / (256 * 49)) ** 0.5
    assert float(sd["fcs.0.weight"].abs().max()) <= bound and float(sd["fcs.0.weight"].abs().max()) > 0.99 * bound
    assert abs(float(sd["fc_mask_iou.weight"].std()) / 0.01 - 1) < 0.05
    assert h.loss_weight == 0.5
    built = T.HEADS.build(dict(type="MaskIoUHead", num_convs=2, roi_feat_size=4, in_channels=64, conv_out_channels=64,
                               fc_out_channels=64, num_classes=5))
    assert tuple(built.fcs[0].weight.shape) == (64, 64 * 2 * 2)
    h2 = T.MaskIoUHead(num_convs=2, roi_feat_size=4, in_channels=64, conv_out_channels=64, fc_out_channels=64,
                       num_classes=5)
    h2.load_state_dict(built.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(h2.state_dict().values(), built.state_dict().values()))


@pytest.mark.parametrize("kw,msg", [(dict(in_channels=96), "multiples of 64"), (dict(conv_out_channels=100), "multiples"),
                                    (dict(num_convs=1), "num_convs"), (dict(roi_feat_size=7), "odd roi_feat_size"),
                                    (dict(loss_iou=dict(type="SmoothL1Loss", loss_weight=1.0)), "loss_iou")])
def test_head_constructs_and_refuses_in_forward(kw, msg):
    import torch_detection_amd as T
    h = T.MaskIoUHead(**kw)
    S = h.roi_feat_size
    with pytest.raises(NotImplementedError, match=msg):
        h(torch.zeros(2, h.in_channels, S, S, dtype=torch.bfloat16), torch.zeros(2, 5, 2 * S, 2 * S),
          torch.ones(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        T.MaskIoUHead(num_convs=0)


# ---- the wrappers' refusals need no GPU ------------------------------------------------------------------------------------
def _target_args(M=7, C=5):
    rois, inds, targets, pred, labels = K.target_case(M, C)
    t = lambda a: torch.from_numpy(np.array(a))
    xy, po, gpo = K.packed_polys()
    return [t(rois), t(inds), xy, po, gpo, t(pred), t(labels), t(targets), t(K.CANVASES)]


def _refuses(fn, args, pos, bad, match):
    a = list(args)
    a[pos] = bad
    with pytest.raises(ValueError, match=match):
        fn(*a)


def test_target_value_errors():
    import torch_detection_amd as T
    a = _target_args()
    fn = T.mask_iou_target
    _refuses(fn, a, 0, a[0][:, :4], "rois must be")
    _refuses(fn, a, 0, a[0].double(), "rois must be")
    _refuses(fn, a, 1, a[1][:-1], "pos_assigned_gt_inds must be")
    _refuses(fn, a, 1, a[1].long(), "pos_assigned_gt_inds must be")
    _refuses(fn, a, 2, a[2].reshape(-1), "poly_xy must be")
    _refuses(fn, a, 3, a[3][:0], "at least one entry")
    _refuses(fn, a, 4, a[4].repeat(65, 1), "batch size")
    _refuses(fn, a, 5, a[5][:-1], "mask_pred must be")
    _refuses(fn, a, 5, a[5][:, :, :, :6], "mask_pred must be")
    _refuses(fn, a, 5, a[5].double(), "mask_pred must be")
    _refuses(fn, a, 5, a[5].permute(0, 1, 3, 2), "NCHW-contiguous or channels_last")
    _refuses(fn, a, 5, torch.zeros(40, 5, 57, 57), "M in 1..56")
    _refuses(fn, a, 6, a[6].int(), "labels must be")
    _refuses(fn, a, 7, a[7].float(), "mask_targets must be")
    _refuses(fn, a, 7, torch.zeros(40, 8, 8, dtype=torch.uint8), "mask_targets must be")
    _refuses(fn, a, 8, a[8][:1], "img_shapes must be")
    _refuses(fn, a, 8, a[8].long(), "img_shapes must be")
    with pytest.raises(ValueError, match="thr must be"):
        fn(*a, thr=float("nan"))
    with pytest.raises(ValueError, match="thr must be"):
        fn(*a, thr=torch.tensor(0.5))
    with pytest.raises(ValueError, match="rois must be a CUDA tensor"):
        fn(*a)                                          # all shapes are right: the device is asked last
    a1 = _target_args(7, 1)
    a1[5] = a1[5][:, 0]                                 # (R, M, M) is C = 1
    with pytest.raises(ValueError, match="rois must be a CUDA tensor"):
        fn(*a1)


def test_loss_and_scores_value_errors():
    import torch_detection_amd as T
    t = lambda a: torch.from_numpy(np.array(a))
    pred, labels, targets = (t(a) for a in K.loss_case(24, 5, 1))
    fn = T.mask_iou_loss
    a = [pred, labels, targets]
    _refuses(fn, a, 0, pred.double(), "mask_iou_pred must be")
    _refuses(fn, a, 0, pred.t(), "mask_iou_pred must be")
    _refuses(fn, a, 0, torch.zeros(24, 1025), "columns")
    _refuses(fn, a, 1, labels.int(), "labels must be")
    _refuses(fn, a, 1, labels[:-1], "labels must be")
    _refuses(fn, a, 2, targets.double(), "mask_iou_targets must be")
    for lw in (float("inf"), torch.tensor(0.5), (0.5,)):
        with pytest.raises(ValueError, match="loss_weight must be"):
            fn(*a, loss_weight=lw)
    with pytest.raises(ValueError, match="mask_iou_pred must be a CUDA tensor"):
        fn(*a)
    pred, dets, labels, counts = (t(x) for x in K.scores_case(5))
    fn = T.mask_scores
    a = [pred, dets, labels, counts]
    _refuses(fn, a, 0, pred[:-1], "mask_iou_pred must be")
    _refuses(fn, a, 1, dets[:, :, :4], "dets must be")
    _refuses(fn, a, 1, dets.repeat(30, 1, 1), "batch size")
    _refuses(fn, a, 2, labels.int(), "labels must be")
    _refuses(fn, a, 3, counts.long(), "counts must be")
    with pytest.raises(ValueError, match="mask_iou_pred must be a CUDA tensor"):
        fn(*a)


def test_stem_value_errors():
    import torch_detection_amd as T
    CL = torch.channels_last
    feats, pred, labels, weight, bias, _ = (torch.from_numpy(a) for a in K.stem_case(4, 5, 1))
    feats = feats.to(torch.bfloat16).contiguous(memory_format=CL)
    fn = T.mask_iou_stem
    a = [feats, pred, labels, weight, bias]
    _refuses(fn, a, 0, feats.float(), "mask_feats must be")
    _refuses(fn, a, 0, feats.contiguous(), "channels_last")
    _refuses(fn, a, 0, feats[:, :, :, :3], "channels_last")
    _refuses(fn, a, 1, pred[:, :, :6, :6].contiguous(), "2S")
    _refuses(fn, a, 1, torch.zeros(7, 5, 7, 7), "2S")
    _refuses(fn, a, 1, pred[:-1], "mask_pred must be")
    _refuses(fn, a, 1, pred.double(), "mask_pred must be")
    _refuses(fn, a, 2, labels.int(), "labels must be")
    _refuses(fn, a, 3, weight[:, :64], "weight must be")
    with pytest.raises(ValueError, match="Cout must be a multiple of 64"):
        fn(feats, pred, labels, weight[:32].contiguous(), bias[:32].contiguous())
    with pytest.raises(ValueError, match="Cout must be a multiple of 64 in 64..512"):
        fn(feats, pred, labels, torch.zeros(576, 65, 3, 3), torch.zeros(576))
    _refuses(fn, a, 3, weight.permute(0, 1, 3, 2), "weight must be")
    _refuses(fn, a, 4, bias[:-1], "bias must be")
    f96 = torch.zeros(7, 96, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=CL)
    with pytest.raises(ValueError, match="multiple of 64"):
        fn(f96, pred, labels, torch.zeros(64, 97, 3, 3), bias)
    with pytest.raises(ValueError, match="label_offset must be"):
        fn(*a, label_offset=2)
    with pytest.raises(ValueError, match="mask_feats must be a CUDA tensor"):
        fn(*a)
    with pytest.raises(ValueError, match="mask_feats must be a CUDA tensor"):
        fn(feats, pred[:, 0].contiguous(), labels, weight, bias)     # (R, 2S, 2S) is C = 1
