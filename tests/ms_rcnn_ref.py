"""NumPy restatement of the Mask Scoring R-CNN spec: the CPU oracle of csrc/mask_iou.hip.

The mask-IoU target is float32, operation for operation and in the spec's order, on integer counts: it must match the
device bit for bit, and so must ``mask_scores``.  The instance bitmap is built row by row from the crossings of §4g: for
an edge that straddles the row of centres y + 0.5 the pixels whose centre compares ``< xi`` are a prefix of the row, found
here by a binary search over the float32 centres themselves (the device derives the same prefix from ``trunc(xi)``);
tests/test_ms_rcnn_oracle.py checks the bitmap against the brute-force point test ``mask_ref.inside_polygon``.

The first layer of the MaskIoUHead (``stem``) and the loss are float64: the device's values are compared with them under
the bounds of tests/ms_rcnn_cases.py.
"""
import numpy as np

import loss_ref as L
import mask_ref as MR

F32 = np.float32
EPS = F32(1e-7)
CANVAS_MAX = 8192


# ---- the target ------------------------------------------------------------------------------------------------------
def polygon_rows(poly, h, w):
    """(h, w) bool: pixel (x, y) is inside ``poly`` (n, 2) by the even-odd rule on the centres (x + 0.5, y + 0.5)."""
    poly = np.asarray(poly, F32).reshape(-1, 2)
    out = np.zeros((h, w), bool)
    if poly.shape[0] < 3 or h == 0 or w == 0:
        return out
    a, b = poly, np.roll(poly, -1, 0)
    xa, ya, xb, yb = (v[:, None] for v in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))           # (n, 1)
    py = (np.arange(h).astype(F32) + F32(0.5))[None, :]                                  # (1, h)
    centres = np.arange(w).astype(F32) + F32(0.5)
    with np.errstate(all="ignore"):
        straddle = (ya > py) != (yb > py)                                                # (n, h)
        xi = xa + ((py - ya) * (xb - xa)) / (yb - ya)                                    # (n, h) float32
    assert xi.dtype == F32
    npre = np.searchsorted(centres, xi.reshape(-1), side="left").reshape(xi.shape)       # centres < xi
    npre[np.isnan(xi)] = 0
    e, y = np.nonzero(straddle)
    cnt = np.zeros((h, w + 1), np.int64)
    np.add.at(cnt, (y, npre[e, y]), 1)
    # pixel x is toggled by the edges whose prefix is longer than x
    longer = cnt.sum(1, keepdims=True) - np.cumsum(cnt, 1)[:, :w]
    return (longer & 1).astype(bool)


def instance_bitmap(polys, h, w):
    out = np.zeros((h, w), bool)
    for p in polys:
        out |= polygon_rows(p, h, w)
    return out


def box_counts(bitmap, box):
    """(full, in): the bitmap's population count and the count inside numpy's ``[y1:y2+1, x1:x2+1]`` of the truncated
    float32 box clipped to the canvas (an empty range counts 0)."""
    h, w = bitmap.shape
    x1, y1, x2, y2 = (int(t) for t in MR.trunc_sat(box))
    xa, xb, ya, yb = max(x1, 0), min(x2, w - 1), max(y1, 0), min(y2, h - 1)
    inside = int(bitmap[ya:yb + 1, xa:xb + 1].sum()) if xa <= xb and ya <= yb else 0
    return int(bitmap.sum()), inside


def iou_from_counts(full, inside, pa, ov, ts):
    """The spec's float32 arithmetic, one rounding per operation."""
    with np.errstate(all="ignore"):
        ratio = F32(inside) / (F32(full) + EPS)
        gf = F32(ts) / (ratio + EPS)
        den = (F32(pa) + gf) - F32(ov)
        return (F32(ov) / den if den > 0 else F32(0)), den


def mask_iou_target(rois, gt_inds, poly_xy, poly_offsets, gt_poly_offsets, pred, labels, targets, img_shapes, thr=0.5):
    """-> (iou (R,) float32, info: dict of per-row integer arrays ``valid, full, inside, pa, ov, ts`` and float32 ``den``).
    ``pred``: (R, C, M, M) float32 array of the STORED logits."""
    rois = np.asarray(rois, F32)
    R = rois.shape[0]
    C = pred.shape[1]
    B, G = gt_poly_offsets.shape[0], gt_poly_offsets.shape[1] - 1
    ch, ok = MR.row_channels(labels, C)
    thr = F32(thr)
    iou = np.zeros(R, F32)
    info = {k: np.zeros(R, np.int64) for k in ("valid", "full", "inside", "pa", "ov", "ts")}
    info["den"] = np.zeros(R, F32)
    cache = {}
    for r in range(R):
        b, g = MR.row_batch(rois[r, 0], B), int(gt_inds[r])
        if b is None or not 0 <= g < G or not ok[r]:
            continue
        h, w = (int(np.clip(v, 0, CANVAS_MAX)) for v in img_shapes[b])
        if (b, g) not in cache:
            cache[(b, g)] = instance_bitmap(MR.instance_polys(poly_xy, poly_offsets, gt_poly_offsets, b, g), h, w)
        full, inside = box_counts(cache[(b, g)], rois[r, 1:])
        with np.errstate(invalid="ignore"):
            on = pred[r, ch[r]].astype(F32) > thr
        t = targets[r] == 1
        pa, ov, ts = int(on.sum()), int((on & t).sum()), int(t.sum())
        iou[r], den = iou_from_counts(full, inside, pa, ov, ts)
        for k, v in (("valid", 1), ("full", full), ("inside", inside), ("pa", pa), ("ov", ov), ("ts", ts)):
            info[k][r] = v
        info["den"][r] = den
    return iou, info


# ---- the loss and the scores -------------------------------------------------------------------------------------------
def mask_iou_loss(pred, labels, targets, loss_weight=0.5, g=1.0):
    """float64.  ``pred``: (R, C) float32 array of the STORED values.  Returns a dict: ``loss``, ``D``, ``live`` (R,) bool,
    ``dpred`` (R, C), ``unit`` (R,) = |2 lw g (p - t)| / D: the magnitude the gradient's bound is stated in."""
    R, C = pred.shape
    labels = np.asarray(labels, np.int64)
    with np.errstate(invalid="ignore"):
        live = (targets > 0) & (labels >= 1) & (labels < C)
    D = max(int(live.sum()), 1)
    lw, gg = float(F32(loss_weight)), float(F32(g))
    rows = np.arange(R)[live]
    d = pred[rows, labels[live]].astype(np.float64) - targets[live].astype(np.float64)
    dpred = np.zeros((R, C))
    dpred[rows, labels[live]] = 2.0 * lw * gg * d / D
    unit = np.zeros(R)
    unit[rows] = np.abs(2.0 * lw * gg * d / D)
    return dict(loss=lw * float((d * d).sum()) / D, D=D, live=live, dpred=dpred, unit=unit)


def mask_scores(pred, dets, labels, counts):
    """float32, one product.  ``pred``: (B * N, C) float32 array of the stored values."""
    B, N, _ = dets.shape
    C = pred.shape[1]
    out = np.zeros((B, N), F32)
    for b in range(B):
        for d in range(min(max(int(counts[b]), 0), N)):
            lab = int(labels[b, d])
            if 0 <= lab + 1 < C:
                with np.errstate(all="ignore"):
                    out[b, d] = F32(pred[b * N + d, lab + 1]) * F32(dets[b, d, 4])
    return out


# ---- the first layer ---------------------------------------------------------------------------------------------------
def stem_channels(labels, C, label_offset=0):
    return MR.row_channels(np.asarray(labels, np.int64) + label_offset, C)


def pooled(pred, labels, label_offset=0):
    """-> (P (R, S, S) float64, idx (R, S, S) int: the window's first maximum 2 dy + dx, -1 on rows without a channel,
    ch, ok).  ``pred``: (R, C, 2S, 2S) array of the stored logits."""
    R, C, M, _ = pred.shape
    S = M // 2
    ch, ok = stem_channels(labels, C, label_offset)
    P = np.zeros((R, S, S))
    idx = np.full((R, S, S), -1)
    for r in range(R):
        if not ok[r]:
            continue
        p = L.sigma(pred[r, ch[r]].astype(np.float64))
        win = p.reshape(S, 2, S, 2).transpose(0, 2, 1, 3).reshape(S, S, 4)            # row-major inside the window
        idx[r] = np.argmax(win, -1)                                                  # numpy: the FIRST maximum
        P[r] = np.take_along_axis(win, idx[r][..., None], -1)[..., 0]
    return P, idx, ch, ok


def _taps(a, S):
    """(R, S, S) -> (R, S, S, 3, 3): a[i + ky - 1, j + kx - 1], 0 outside."""
    pad = np.pad(a, ((0, 0), (1, 1), (1, 1)))
    return np.stack([np.stack([pad[:, ky:ky + S, kx:kx + S] for kx in range(3)], -1) for ky in range(3)], -2)


def stem(feats, pred, labels, weight, bias, label_offset=0, relu=True, gy=None):
    """float64 forward and, with the cotangent ``gy`` (R, Cout, S, S), all four gradients, written out by hand (checked
    against torch autograd in tests/test_ms_rcnn_oracle.py).  Returns a dict: ``a`` (R, Cout, S, S) the mask channel's
    addend and ``a_abs`` = sum |w| |P|; ``y``; ``P``, ``idx``; and with ``gy``: ``gz``, ``dfeats``, ``dpred`` with
    ``dpred_abs`` = sigma(x) sigma(-x) sum |w| |gz| at the hot elements, ``dweight`` with ``dw1_abs`` = sum |gz| |P|,
    ``dbias``."""
    import torch
    import torch.nn.functional as TF
    feats, weight, bias = (np.asarray(t, np.float64) for t in (feats, weight, bias))
    R, Cf, S, _ = feats.shape
    Cout = weight.shape[0]
    P, idx, ch, ok = pooled(pred, labels, label_offset)
    w1 = weight[:, Cf]                                                               # (Cout, 3, 3)
    T = _taps(P, S)                                                                  # (R, S, S, 3, 3)
    a = np.einsum("rijyx,oyx->roij", T, w1)
    a_abs = np.einsum("rijyx,oyx->roij", np.abs(T), np.abs(w1))
    conv = TF.conv2d(torch.from_numpy(feats), torch.from_numpy(np.ascontiguousarray(weight[:, :Cf])),
                     torch.from_numpy(bias), 1, 1).numpy()
    z = conv + a
    y = np.maximum(z, 0) if relu else z
    out = dict(a=a, a_abs=a_abs, y=y, P=P, idx=idx, ch=ch, ok=ok)
    if gy is None:
        return out
    gz = np.asarray(gy, np.float64) * ((z > 0) if relu else 1.0)
    out.update(stem_backward(feats, pred, weight, P, idx, ch, ok, gz))
    out["gz"] = gz
    return out


def stem_backward(feats, pred, weight, P, idx, ch, ok, gz):
    """The four gradients from the masked cotangent ``gz`` (R, Cout, S, S), float64."""
    import torch
    feats, weight, gz = (np.asarray(t, np.float64) for t in (feats, weight, gz))
    R, Cf, S, _ = feats.shape
    C, M = pred.shape[1], pred.shape[2]
    w1 = weight[:, Cf]
    wf = torch.from_numpy(np.ascontiguousarray(weight[:, :Cf]))
    tg = torch.from_numpy(np.ascontiguousarray(gz))
    dfeats = torch.nn.grad.conv2d_input(feats.shape, wf, tg, 1, 1).numpy()
    dwf = torch.nn.grad.conv2d_weight(torch.from_numpy(feats), wf.shape, tg, 1, 1).numpy()
    # dP[r, i, j] = sum_taps sum_co w1[co, ky, kx] gz[r, co, i - ky + 1, j - kx + 1]
    gpad = np.pad(gz, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dP = np.zeros((R, S, S))
    dP_abs = np.zeros((R, S, S))
    for ky in range(3):
        for kx in range(3):
            sh = gpad[:, :, 2 - ky:2 - ky + S, 2 - kx:2 - kx + S]                     # gz[i - ky + 1, j - kx + 1]
            dP += np.einsum("o,roij->rij", w1[:, ky, kx], sh)
            dP_abs += np.einsum("o,roij->rij", np.abs(w1[:, ky, kx]), np.abs(sh))
    dpred = np.zeros(pred.shape)
    dpred_abs = np.zeros(pred.shape)
    ii, jj = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    for r in range(R):
        if not ok[r]:
            continue
        yy, xx = 2 * ii + idx[r] // 2, 2 * jj + idx[r] % 2
        x = pred[r, ch[r]].astype(np.float64)[yy, xx]
        s = L.sigma(x) * L.sigma(-x)
        dpred[r, ch[r], yy, xx] = dP[r] * s
        dpred_abs[r, ch[r], yy, xx] = dP_abs[r] * s
    T = _taps(P, S)
    dw1 = np.einsum("roij,rijyx->oyx", gz, T)
    dw1_abs = np.einsum("roij,rijyx->oyx", np.abs(gz), np.abs(T))
    dweight = np.concatenate([dwf, dw1[:, None]], 1)
    return dict(dfeats=dfeats, dpred=dpred, dpred_abs=dpred_abs, dP=dP, dweight=dweight, dw1_abs=dw1_abs,
                dbias=gz.sum((0, 2, 3)))
