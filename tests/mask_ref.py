"""NumPy restatement of the mask-branch spec: the CPU oracle of csrc/mask.hip.

The mask targets and the geometry of the paste (box truncation, cell centres, edge crossings, sample positions and the
bilinear fractions) are float32, operation for operation and in the spec's order, so the targets must match the device
bit for bit.  The loss, its gradient, sigmoid and the four-term interpolation are float64: the device's float32 values
are compared with them under the bounds §4g derives.  ``dtype=np.float64`` evaluates the target formula in float64
instead (tests/test_mask_oracle.py compares the two).
"""
import numpy as np

import loss_ref as L

F32 = np.float32
HALF = F32(0.5)


def trunc_sat(v):
    """float32 -> integer (int64 array): truncation toward zero, saturating at the ends of int32, NaN -> 0."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        t = np.trunc(np.where(np.isnan(v), F32(0), v).astype(np.float64))
    return np.clip(t, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def int_box(c):
    """(x1, y1, w, h) of a float32 (x1, y1, x2, y2) row as Python ints: w = max(x2 - x1 + 1, 1), h alike."""
    x1, y1, x2, y2 = (int(t) for t in trunc_sat(c))
    return x1, y1, max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)


def row_batch(bf, B):
    """The truncated batch index, or None when it is outside [0, B) (NaN included): §4c step 1."""
    bf = F32(bf)
    if not (bf > F32(-1) and bf < F32(B)):
        return None
    return int(bf)


def cell_centres(box, M, dtype=F32):
    """(px (M,), py (M,)) of the M x M grid over an ``int_box``."""
    x1, y1, w, h = box
    T = dtype
    k = np.arange(M).astype(T) + T(0.5)
    return T(x1) + (k * T(w)) / T(M), T(y1) + (k * T(h)) / T(M)


def inside_polygon(px, py, poly, dtype=F32):
    """Even-odd rule for the points (px[j], py[i]) against one polygon (n, 2): an (M, M) boolean array.  Edge a -> b
    (the closing edge included) flips a point's parity when ``(ya > py) != (yb > py)`` and
    ``px < xa + ((py - ya) * (xb - xa)) / (yb - ya)``; the quotient is looked at only where the first holds."""
    T = dtype
    poly = np.asarray(poly, T).reshape(-1, 2)
    n = poly.shape[0]
    out = np.zeros((py.shape[0], px.shape[0]), bool)
    if n < 3:
        return out
    a, b = poly, np.roll(poly, -1, 0)
    xa, ya, xb, yb = (v[:, None] for v in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))        # (n, 1)
    with np.errstate(all="ignore"):
        straddle = (ya > py[None, :]) != (yb > py[None, :])                              # (n, M) over rows i
        xi = xa + ((py[None, :] - ya) * (xb - xa)) / (yb - ya)                           # (n, M)
        cross = straddle[:, :, None] & (px[None, None, :] < xi[:, :, None])              # (n, M, M)
    return (cross.sum(0) & 1).astype(bool)


def instance_mask(box, polys, M, dtype=F32):
    """The union over ``polys`` (a list of (n, 2) arrays) of the even-odd interiors, on the grid of ``box``."""
    px, py = cell_centres(box, M, dtype)
    out = np.zeros((M, M), bool)
    for p in polys:
        out |= inside_polygon(px, py, p, dtype)
    return out


def instance_polys(poly_xy, poly_offsets, gt_poly_offsets, b, g):
    """The polygons of ground truth g of image b, every offset clamped to its array as the device does."""
    P, Q = poly_xy.shape[0], poly_offsets.shape[0] - 1
    q0, q1 = (int(np.clip(v, 0, Q)) for v in gt_poly_offsets[b, g:g + 2])
    out = []
    for q in range(q0, q1):
        s, e = (int(np.clip(v, 0, P)) for v in poly_offsets[q:q + 2])
        out.append(poly_xy[s:max(e, s)])
    return out


def mask_target(rois, gt_inds, poly_xy, poly_offsets, gt_poly_offsets, M, dtype=F32):
    """-> (mask_targets (R, M, M) uint8, mask_weights (R,) float32)."""
    rois = np.asarray(rois, F32)
    R = rois.shape[0]
    B, G = gt_poly_offsets.shape[0], gt_poly_offsets.shape[1] - 1
    targets = np.zeros((R, M, M), np.uint8)
    weights = np.zeros(R, F32)
    for r in range(R):
        b, g = row_batch(rois[r, 0], B), int(gt_inds[r])
        if b is None or not 0 <= g < G:
            continue
        polys = instance_polys(poly_xy, poly_offsets, gt_poly_offsets, b, g)
        targets[r] = instance_mask(int_box(rois[r, 1:]), polys, M, dtype)
        weights[r] = 1
    return targets, weights


def row_channels(labels, C):
    """(channel per row, valid per row): label in 1..C-1, or channel 0 of a class-agnostic head."""
    labels = np.asarray(labels, np.int64)
    if C == 1:
        return np.zeros_like(labels), np.ones(labels.shape, bool)
    ok = (labels >= 1) & (labels < C)
    return np.where(ok, labels, 0), ok


def mask_head_loss(pred, targets, labels, weights, avg_factor=None, g=1.0):
    """float64 loss and gradient.  ``pred``: (R, C, M, M) float32 array of the STORED values.  Returns a dict: ``loss``,
    ``mag`` = sum |w l| / (D M^2), ``avg`` = D (float32), ``dpred`` (R, C, M, M), ``unit`` (R,) = |g w| / (D M^2)."""
    R, C, M, _ = pred.shape
    ch, ok = row_channels(labels, C)
    avg = L.divisor(avg_factor, (weights > 0).sum())
    w = np.where(ok, weights, F32(0)).astype(np.float64)
    live = w != 0
    x = np.zeros((R, M, M))
    x[live] = pred[np.arange(R)[live], ch[live]].astype(np.float64)
    t = targets != 0
    l = np.where(t, L.sp(-x), L.sp(x))
    dl = np.where(t, -L.sigma(-x), L.sigma(x))
    den = float(avg) * M * M
    gg = float(F32(g))
    wl = np.where(live[:, None, None], w[:, None, None] * l, 0.0)
    dpred = np.zeros((R, C, M, M))
    dpred[np.arange(R)[live], ch[live]] = (gg * w[live, None, None] * dl[live]) / den
    return dict(loss=wl.sum() / den, mag=np.abs(wl).sum() / den, avg=avg, dpred=dpred, unit=np.abs(gg * w) / den)


def rois_from_detections(dets, counts, scale_factors=None):
    dets = np.asarray(dets, F32)
    B, N, _ = dets.shape
    s = np.ones(B, F32) if scale_factors is None else np.broadcast_to(np.asarray(scale_factors, F32), (B,))
    out = np.zeros((B, N, 5), F32)
    out[..., 0] = -1
    for b in range(B):
        n = max(int(counts[b]), 0)
        out[b, :n, 0] = b
        out[b, :n, 1:] = dets[b, :n, :4] * s[b]
    return out.reshape(B * N, 5)


def paste_axis(off, extent, M):
    """One axis of the sample for the canvas offsets ``off`` (int64 array) from the box's first pixel: (lo, hi, l, h),
    float32 as the spec writes it."""
    s = ((off.astype(F32) + HALF) * F32(M)) / F32(extent) - HALF
    s = np.where(s > 0, s, F32(0)).astype(F32)
    lo = s.astype(np.int64)
    top = lo >= M - 1
    lo = np.where(top, M - 1, lo)
    hi = np.where(top, M - 1, lo + 1)
    l = np.where(top, F32(0), s - lo.astype(F32)).astype(F32)
    return lo, hi, l, (F32(1) - l).astype(F32)


def mask_head_masks(pred, dets, labels, counts, out_shape, img_shapes=None, thr=0.5):
    """-> (masks (B*N, H, W) uint8 decided by the float64 value, v (B*N, H, W) float64: the interpolated probability
    inside the clipped boxes, NaN elsewhere).  ``pred``: (B*N, C, M, M) float32 array of the stored values."""
    dets = np.asarray(dets, F32)
    B, N, _ = dets.shape
    _, C, M, _ = pred.shape
    H, W = out_shape
    thr = float(F32(thr))
    masks = np.zeros((B * N, H, W), np.uint8)
    v = np.full((B * N, H, W), np.nan)
    for b in range(B):
        LH, LW = (H, W) if img_shapes is None else (int(np.clip(img_shapes[b, 0], 0, H)),
                                                    int(np.clip(img_shapes[b, 1], 0, W)))
        for d in range(min(max(int(counts[b]), 0), N)):
            n = b * N + d
            lab = int(labels[b, d])
            if C > 1 and not 0 <= lab < C - 1:
                continue
            ch = lab + 1 if C > 1 else 0
            x1, y1, w, h = int_box(dets[b, d, :4])
            xa, xb, ya, yb = max(x1, 0), min(x1 + w, LW), max(y1, 0), min(y1 + h, LH)
            if xa >= xb or ya >= yb:
                continue
            with np.errstate(all="ignore"):
                p = L.sigma(pred[n, ch].astype(np.float64))
            xl, xh, lx, hx = paste_axis(np.arange(xa, xb, dtype=np.int64) - x1, w, M)
            yl, yh, ly, hy = paste_axis(np.arange(ya, yb, dtype=np.int64) - y1, h, M)
            lx, hx, ly, hy = (a.astype(np.float64) for a in (lx, hx, ly, hy))
            w1, w2, w3, w4 = np.outer(hy, hx), np.outer(hy, lx), np.outer(ly, hx), np.outer(ly, lx)
            val = ((w1 * p[np.ix_(yl, xl)] + w2 * p[np.ix_(yl, xh)]) + w3 * p[np.ix_(yh, xl)]) + w4 * p[np.ix_(yh, xh)]
            v[n, ya:yb, xa:xb] = val
            with np.errstate(invalid="ignore"):
                masks[n, ya:yb, xa:xb] = val > thr
    return masks, v


def pack_bits(masks):
    """(..., W) 0/1 -> (..., 8 * ceil(W / 64)) uint8: bit x % 8 of byte x // 8 is pixel x, padding bits 0."""
    W = masks.shape[-1]
    pw = 8 * ((W + 63) // 64)
    bits = np.packbits(masks.astype(np.uint8), axis=-1, bitorder="little")
    out = np.zeros(masks.shape[:-1] + (pw,), np.uint8)
    out[..., :bits.shape[-1]] = bits
    return out
