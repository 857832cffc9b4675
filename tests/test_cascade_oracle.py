"""CPU: the Cascade R-CNN oracle tests/cascade_ref.py against an independently written torch formulation of
mmdetection v1's regress_by_class / refine_bboxes / logit averaging (boxes and counts bit-equal), known-answer cases, and
the constructor, state-dict keys and registry entry of CascadeRoIHead (the package only: no GPU, no kernels)."""
import numpy as np
import pytest
import torch

import cascade_cases as K
import cascade_ref as CR
import detect_ref as D

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- mmdetection v1, restated in torch ------------------------------------------------------------------------------
def mm_delta2bbox(rois, deltas, means, stds, max_shape, wh_ratio_clip=16 / 1000):
    """mmdet/core/bbox/transforms.py delta2bbox, with exp evaluated as the oracle defines it (float64, rounded)."""
    means = deltas.new_tensor(means).repeat(1, deltas.size(1) // 4)
    stds = deltas.new_tensor(stds).repeat(1, deltas.size(1) // 4)
    den = deltas * stds + means
    dx, dy, dw, dh = den[:, 0::4], den[:, 1::4], den[:, 2::4], den[:, 3::4]
    max_ratio = float(f32(np.abs(np.log(wh_ratio_clip))))
    dw, dh = dw.clamp(min=-max_ratio, max=max_ratio), dh.clamp(min=-max_ratio, max=max_ratio)
    px = ((rois[:, 0] + rois[:, 2]) * 0.5).unsqueeze(1).expand_as(dx)
    py = ((rois[:, 1] + rois[:, 3]) * 0.5).unsqueeze(1).expand_as(dy)
    pw = (rois[:, 2] - rois[:, 0] + 1.0).unsqueeze(1).expand_as(dw)
    ph = (rois[:, 3] - rois[:, 1] + 1.0).unsqueeze(1).expand_as(dh)
    gw, gh = pw * dw.double().exp().float(), ph * dh.double().exp().float()
    gx, gy = px + pw * dx, py + ph * dy
    x1, y1 = gx - gw * 0.5 + 0.5, gy - gh * 0.5 + 0.5
    x2, y2 = gx + gw * 0.5 - 0.5, gy + gh * 0.5 - 0.5
    x1, x2 = x1.clamp(min=0, max=max_shape[1] - 1), x2.clamp(min=0, max=max_shape[1] - 1)
    y1, y2 = y1.clamp(min=0, max=max_shape[0] - 1), y2.clamp(min=0, max=max_shape[0] - 1)
    return torch.stack([x1, y1, x2, y2], dim=-1).view_as(deltas)


def mm_regress_by_class(rois, label, bbox_pred, img_shape, stds):
    """BBoxHead.regress_by_class: rois (n, 5)."""
    if bbox_pred.size(1) != 4:
        inds = torch.stack((label * 4, label * 4 + 1, label * 4 + 2, label * 4 + 3), 1)
        bbox_pred = torch.gather(bbox_pred, 1, inds)
    new = mm_delta2bbox(rois[:, 1:], bbox_pred, K.MEANS, stds, img_shape)
    return torch.cat((rois[:, [0]], new), dim=1)


def mm_refine_bboxes(rois, labels, bbox_pred, pos_is_gts, shapes, stds):
    """BBoxHead.refine_bboxes: per image, regress and drop the ground truths -> a list of (n_i, 4)."""
    out = []
    for i in range(len(shapes)):
        inds = torch.nonzero(rois[:, 0].long() == i).squeeze(1)       # exact integer indices in these cases
        r = mm_regress_by_class(rois[inds], labels[inds], bbox_pred[inds], shapes[i], stds)
        keep = pos_is_gts[inds] == 0
        out.append(r[keep][:, 1:])
    return out


@pytest.mark.parametrize("dt", sorted(K.DTYPES))
@pytest.mark.parametrize("C,agnostic", [(1, True), (2, False), (81, False), (81, True)])
def test_reference_matches_the_torch_formulation(C, agnostic, dt):
    R, B, P = 300, 3, 60
    c = K.refine_case(R, B, C, agnostic, dt, seed=C + len(dt), pad=0.15)
    c["rois"][2, 0] = -1                                                # integer indices only, for the torch side
    c["is_gt"][2] = False
    stds = (0.05, 0.05, 0.1, 0.1)
    reg = K.widen(c["reg"])
    for labels in (c["labels"], None):
        cls = None if labels is not None else K.widen(c["cls"])
        lab = labels if labels is not None else torch.from_numpy(cls).argmax(dim=1).numpy()
        props, counts = CR.refine_bboxes(c["rois"], reg, c["shapes"], labels, cls, c["gt_inds"], c["gt"], P, K.MEANS, stds)
        rows = CR.refine_bboxes(c["rois"], reg, c["shapes"], labels, cls, target_means=K.MEANS, target_stds=stds)
        rois_t = torch.from_numpy(c["rois"])
        ok = (rois_t[:, 0] >= 0) & (rois_t[:, 0] < B)
        sel = torch.nonzero(ok).squeeze(1)
        mm = mm_refine_bboxes(rois_t[sel], torch.from_numpy(lab)[sel], torch.from_numpy(reg)[sel],
                              torch.from_numpy(c["is_gt"].astype(np.uint8))[sel], c["shapes"], stds)
        assert (counts > 0).all() and (counts == [min(P, m.shape[0]) for m in mm]).all()
        assert any(m.shape[0] > P for m in mm) or P >= R
        for b in range(B):
            n = counts[b]
            assert np.array_equal(_bits(props[b, :n, :4]), _bits(mm[b][:n].numpy()))
            assert not props[b, n:].any() and not props[b, :, 4].any()
        # row-aligned: every valid row, ground truths included, in place
        full = mm_refine_bboxes(rois_t[sel], torch.from_numpy(lab)[sel], torch.from_numpy(reg)[sel],
                                torch.zeros(len(sel), dtype=torch.uint8), c["shapes"], stds)
        for b in range(B):
            mine = np.nonzero(c["img"] == b)[0]
            mine = mine[mine != 2]
            assert np.array_equal(_bits(rows[mine, 1:]), _bits(full[b].numpy()))
            assert (rows[mine, 0] == b).all()
        off = np.nonzero(~ok.numpy())[0]
        assert (rows[off, 0] == -1).all() and not rows[off, 1:].any()


def test_average_matches_torch_and_one_stage_is_bbox_head_detections():
    for dt in sorted(K.DTYPES):
        rois, logits, reg, shapes = K.detect_case(120, 2, 7, 3, False, dt, seed=5)
        acc = logits[0].float()
        for x in logits[1:]:
            acc = acc + x.float()
        mm = (acc / float(len(logits))).numpy()
        assert np.array_equal(_bits(CR.average_logits([K.widen(x) for x in logits])), _bits(mm))
        st = {}
        one = CR.cascade_detections(rois, [K.widen(logits[0])], K.widen(reg), shapes, 1.25, stats=st)
        ref = D.bbox_head_detections(rois, K.widen(logits[0]), K.widen(reg), shapes, 1.25)
        assert sum(st["suppressed"]) > 0 and (one[3] > 0).all()
        for a, b in zip(one, ref):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        three = CR.cascade_detections(rois, [K.widen(x) for x in logits], K.widen(reg), shapes, 1.25)
        assert not np.array_equal(three[4], one[4])


# ---- known answers ---------------------------------------------------------------------------------------------------
SH = [(100, 200), (100, 200)]


def _rois(rows):
    return np.asarray(rows, f32)


def test_all_ground_truth_image_counts_zero():
    gt = np.asarray([[[10, 10, 50, 50], [60, 20, 90, 80]], [[5, 5, 30, 30], [0, 0, 0, 0]]], f32)
    rois = _rois([[0, 10, 10, 50, 50], [0, 60, 20, 90, 80], [1, 5, 5, 30, 30], [1, 40, 40, 60, 60]])
    gi = np.asarray([0, 1, 0, -1], np.int32)
    props, counts = CR.refine_bboxes(rois, np.zeros((4, 4), f32), SH, labels=np.zeros(4, np.int64),
                                     pos_assigned_gt_inds=gi, gt_bboxes=gt, max_per_img=3)
    assert counts.tolist() == [0, 1] and not props[0].any()
    assert props[1, 0].tolist() == [40, 40, 60, 60, 0] and not props[1, 1:].any()
    # the index decides: the same coordinates under another ground truth's index stay
    gi2 = np.asarray([1, 0, 0, -1], np.int32)
    assert CR.refine_bboxes(rois, np.zeros((4, 4), f32), SH, labels=np.zeros(4, np.int64), pos_assigned_gt_inds=gi2,
                            gt_bboxes=gt, max_per_img=3)[1].tolist() == [2, 1]


def test_truncation_and_interleaved_padding():
    rows = []
    for i in range(6):
        rows += [[0, 10 + i, 10, 40 + i, 50], [-1, 0, 0, 0, 0], [1, 20, 10 + i, 60, 40 + i], [2, 1, 1, 2, 2]]
    rois = _rois(rows)
    props, counts = CR.refine_bboxes(rois, np.zeros((24, 4), f32), SH, labels=np.zeros(24, np.int64), max_per_img=4)
    assert counts.tolist() == [4, 4]
    assert props[0, :, 0].tolist() == [10, 11, 12, 13] and props[1, :, 1].tolist() == [10, 11, 12, 13]
    out = CR.refine_bboxes(rois, np.zeros((24, 4), f32), SH, labels=np.zeros(24, np.int64))
    assert out[:, 0].tolist() == [0, -1, 1, -1] * 6 and not out[1::4].any(where=[False, True, True, True, True])
    assert np.array_equal(out[0::4, 1:], rois[0::4, 1:])


def test_argmax_tie_goes_to_the_lower_class_and_labels_pick_columns():
    cls = np.asarray([[0.5, 1.0, 1.0], [1.0, 0.5, 1.0], [-np.inf, -np.inf, -np.inf]], f32)
    assert CR.argmax_labels(cls).tolist() == [1, 0, 0]
    rois = _rois([[0, 10, 10, 29, 29]] * 3)
    reg = np.zeros((3, 12), f32)
    reg[:, 4] = 1.0                                  # class 1: dx = 1 * 0.1 * 20 = 2 pixels
    out = CR.refine_bboxes(rois, reg, SH, cls_score=cls)
    assert out[:, 1].tolist() == [12, 10, 10]
    out = CR.refine_bboxes(rois, reg, SH, labels=np.asarray([1, 3, -1], np.int64))
    assert out[:, 0].tolist() == [0, -1, -1]         # a label outside [0, C) makes the row padding
    # clipped at w - 1 / h - 1 and at 0; dw beyond wh_ratio_clip
    big = np.zeros((1, 4), f32)
    big[0, 2:] = 50.0
    assert CR.refine_bboxes(rois[:1], big, SH, labels=np.zeros(1, np.int64))[0].tolist() == [0, 0, 0, 199, 99]


# ---- the module (package only) --------------------------------------------------------------------------------------
def test_cascade_roi_head_constructor_registry_and_keys():
    import torch_detection_amd as T
    from torch_detection_amd.cascade import STAGE_STDS
    assert T.HEADS.module_dict["CascadeRoIHead"] is T.CascadeRoIHead
    small = dict(type="BBoxHead", num_fcs=2, in_channels=8, fc_out_channels=16, roi_feat_size=7, num_classes=5)
    ext = dict(type="SingleRoIExtractor", roi_layer=dict(type="RoIAlign", out_size=7, sample_num=2), out_channels=8,
               featmap_strides=[4, 8])
    h = T.HEADS.build(dict(type="CascadeRoIHead", bbox_head=small, bbox_roi_extractor=ext))
    assert h.num_stages == 3 and h.stage_loss_weights == (1.0, 0.5, 0.25)
    assert [c["pos_iou_thr"] for c in h.train_cfg] == [0.5, 0.6, 0.7]
    assert [c["min_pos_iou"] for c in h.train_cfg] == [0.5, 0.6, 0.7] and all(c["num"] == 512 for c in h.train_cfg)
    assert h.target_stds == [tuple(s) for s in STAGE_STDS] and h.target_means == [(0.0,) * 4] * 3
    keys = set(h.state_dict())
    assert keys == {"bbox_head.%d.%s.%s" % (i, m, p) for i in range(3)
                    for m in ("shared_fcs.0", "shared_fcs.1", "fc_cls", "fc_reg") for p in ("weight", "bias")}
    assert all(b.reg_class_agnostic and b.fc_reg.weight.shape[0] == 4 for b in h.bbox_head)
    assert len(h.bbox_roi_extractor) == 3 and h.bbox_roi_extractor[1].featmap_strides == (4, 8)
    # lists per stage, two stages
    h2 = T.CascadeRoIHead(num_stages=2, stage_loss_weights=(1, 0.5), bbox_head=[small, dict(small, num_fcs=1)],
                          bbox_roi_extractor=[ext, ext],
                          train_cfg=[dict(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, num=64, pos_fraction=0.25,
                                          add_gt_as_proposals=True)] * 2)
    assert len(h2.bbox_head[1].shared_fcs) == 1 and h2.target_stds == [tuple(s) for s in STAGE_STDS[:2]]
    with pytest.raises(ValueError):
        T.CascadeRoIHead(num_stages=2)                                   # three loss weights for two stages
    with pytest.raises(ValueError):
        T.CascadeRoIHead(num_stages=4, stage_loss_weights=(1, 1, 1, 1), bbox_head=small, bbox_roi_extractor=ext)
    # unsupported configurations are accepted here and refused in the call
    for kw in (dict(mask_head=dict(type="FCNMaskHead")), dict(shared_head=dict(type="ResLayer")),
               dict(bbox_roi_extractor=dict(ext, roi_layer=dict(type="RoIPool", out_size=7)))):
        hm = T.CascadeRoIHead(**dict(dict(bbox_head=small, bbox_roi_extractor=ext), **kw))
        with pytest.raises(NotImplementedError):
            hm.simple_test(None, None, None, None)
        with pytest.raises(NotImplementedError):
            hm.forward_train(None, None, None, None, None, None, None)


def test_wrappers_refuse_bad_arguments_without_a_gpu():
    import torch_detection_amd as T
    rois, reg = torch.zeros(6, 5), torch.zeros(6, 12)
    ish = torch.tensor([[10, 10]], dtype=torch.int32)
    lab, cls = torch.zeros(6, dtype=torch.int64), torch.zeros(6, 3)
    cases = [
        (lambda: T.refine_bboxes(rois, reg, ish), "exactly one of labels and cls_score"),
        (lambda: T.refine_bboxes(rois, reg, ish, labels=lab, cls_score=cls), "exactly one of labels and cls_score"),
        (lambda: T.refine_bboxes(rois, reg[:, :6].contiguous(), ish, labels=lab), "4C columns"),
        (lambda: T.refine_bboxes(rois, reg, ish, cls_score=torch.zeros(6, 2)), "neither 4 nor 4"),
        (lambda: T.refine_bboxes(rois, reg, ish, labels=lab, max_per_img=0), "max_per_img must be in 1..8192"),
        (lambda: T.refine_bboxes(rois, reg, ish, labels=lab, pos_assigned_gt_inds=torch.zeros(6, dtype=torch.int32)),
         "go together"),
        (lambda: T.refine_bboxes(rois, reg, ish, labels=lab, pos_assigned_gt_inds=torch.zeros(6, dtype=torch.int32),
                                 gt_bboxes=torch.zeros(1, 2, 4)), "compacted mode only"),
        (lambda: T.refine_bboxes(rois, reg, ish, labels=lab), "rois must be a CUDA tensor"),
        (lambda: T.cascade_detections(rois, [], reg, ish), "list of 1..8"),
        (lambda: T.cascade_detections(rois, [cls] * 9, reg, ish), "list of 1..8"),
        (lambda: T.cascade_detections(rois, [cls, cls.half()], reg, ish), r"cls_scores\[1\] must be"),
        (lambda: T.cascade_detections(rois, [cls, cls], reg, ish), "rois must be a CUDA tensor"),
    ]
    for fn, msg in cases:
        with pytest.raises(ValueError, match=msg):
            fn()
