"""NumPy restatement of the multi-level RoIAlign spec: the CPU oracle of csrc/roi_align.hip.

Geometry, weights and the forward are fp32 in the spec's operation order (NumPy float32 operations are correctly
rounded IEEE); the backward and the float64 forward (``exact64``, for the adjoint check) take the same fp32 weights
and combine them in float64.  Features are (B, C, H, W) arrays holding 16-bit values exactly (float32 or float64)."""
import numpy as np

f32 = np.float32
MAX_SAMPLES = 512


def map_levels(rois, num_levels, finest_scale=56):
    """(R,) int64 level of every row of ``rois`` (R, 5) or (R, 4+): floor(log2(s)) from the exponent of
    s = sqrt((x2-x1+1) * (y2-y1+1)) / finest_scale + 1e-6 (fp32), clamped; non-positive / non-normal s -> 0."""
    r = np.asarray(rois, f32)
    x1, y1, x2, y2 = (r[:, k] for k in (-4, -3, -2, -1))
    with np.errstate(invalid="ignore", over="ignore"):
        w = (x2 - x1) + f32(1)
        h = (y2 - y1) + f32(1)
        s = np.sqrt(w * h) / f32(finest_scale) + f32(1e-6)
    u = s.view(np.uint32)
    e = ((u >> 23) & 0xFF).astype(np.int64)
    lvl = e - 127
    bad = ((u >> 31) != 0) | (e == 0) | (e == 255)
    lvl = np.where(bad, 0, lvl)
    return np.clip(lvl, 0, num_levels - 1).astype(np.int64)


def batch_index(v, B):
    """(int)v if the truncation lands in [0, B), else -1 (NaN included)."""
    v = f32(v)
    return int(v) if (v > -1 and v < B) else -1


def geometry(roi, scale, S, sampling_ratio):
    """(sw, sh, bw, bh, gw, gh) of one RoI on a level of spatial scale ``scale`` (all fp32 but the counts)."""
    x1, y1, x2, y2 = (f32(v) for v in roi)
    sc = f32(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        sw, sh = x1 * sc, y1 * sc
        ew, eh = (x2 + f32(1)) * sc, (y2 + f32(1)) * sc
        rw, rh = ew - sw, eh - sh
    rw = rw if rw > 0 else f32(0)
    rh = rh if rh > 0 else f32(0)
    bw, bh = rw / f32(S), rh / f32(S)

    def samples(b):
        c = np.ceil(b)
        return int(c) if c < MAX_SAMPLES else MAX_SAMPLES
    gw = sampling_ratio if sampling_ratio > 0 else samples(bw)
    gh = sampling_ratio if sampling_ratio > 0 else samples(bh)
    return sw, sh, bw, bh, gw, gh


def sample_axis(s0, b, S, g, n):
    """Sample coordinates of one axis in (bin, sample) order and their bilinear corners: (ok, lo, hi, l, h), each
    (S*g,).  v = (s0 + p*b) + ((i + 0.5)*b) / g; out of [-1, n] -> not ok; clamp at 0; lo = (int)v, at the far edge
    lo = hi = n-1 and v = lo."""
    p = np.repeat(np.arange(S, dtype=f32), g)
    i = np.tile(np.arange(g, dtype=f32), S)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (f32(s0) + p * f32(b)) + ((i + f32(0.5)) * f32(b)) / f32(g)
    ok = ~((v < -1) | (v > n))
    v = np.where(v > 0, v, f32(0)).astype(f32)
    v = np.where(ok, v, f32(0)).astype(f32)
    lo = v.astype(np.int64)
    edge = lo >= n - 1
    lo = np.where(edge, n - 1, lo)
    hi = np.where(edge, n - 1, lo + 1)
    v = np.where(edge, lo.astype(f32), v).astype(f32)
    l = (v - lo.astype(f32)).astype(f32)
    h = (f32(1) - l).astype(f32)
    return ok, lo, hi, l, h


def _rows(feats, rois, featmap_strides, S, sampling_ratio, finest_scale):
    L = len(feats)
    B = feats[0].shape[0]
    rois = np.asarray(rois, f32)
    levels = map_levels(rois, L, finest_scale)
    for r in range(rois.shape[0]):
        b = batch_index(rois[r, 0], B)
        if b < 0:
            continue
        lv = int(levels[r])
        H, W = feats[lv].shape[2], feats[lv].shape[3]
        sw, sh, bw, bh, gw, gh = geometry(rois[r, 1:], f32(1.0 / featmap_strides[lv]), S, sampling_ratio)
        ay = sample_axis(sh, bh, S, gh, H)
        ax = sample_axis(sw, bw, S, gw, W)
        yield r, b, lv, ay, ax, gh, gw


def roi_align_forward(feats, rois, featmap_strides=(4, 8, 16, 32), out_size=7, sampling_ratio=2, finest_scale=56,
                      exact64=False):
    """(R, C, S, S): fp32 (before the one rounding to the feature dtype), or float64 with ``exact64``."""
    S = out_size
    dt = np.float64 if exact64 else f32
    R, C = np.asarray(rois).shape[0], feats[0].shape[1]
    out = np.zeros((R, C, S, S), dt)
    for r, b, lv, (oky, yl, yh, ly, hy), (okx, xl, xh, lx, hx), gh, gw in _rows(feats, rois, featmap_strides, S,
                                                                                   sampling_ratio, finest_scale):
        F = feats[lv][b]                                               # (C, H, W)
        if F.dtype != dt:
            F = F.astype(dt)
        if exact64:
            hy, ly, hx, lx = (a.astype(np.float64) for a in (hy, ly, hx, lx))
        w1, w2 = hy[:, None] * hx[None, :], hy[:, None] * lx[None, :]
        w3, w4 = ly[:, None] * hx[None, :], ly[:, None] * lx[None, :]
        v1, v2 = F[:, yl[:, None], xl[None, :]], F[:, yl[:, None], xh[None, :]]
        v3, v4 = F[:, yh[:, None], xl[None, :]], F[:, yh[:, None], xh[None, :]]
        val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4                # (C, S*gh, S*gw)
        val = np.where((oky[:, None] & okx[None, :])[None], val, dt(0)).astype(dt)
        val = val.reshape(C, S, gh, S, gw)
        acc = np.zeros((C, S, S), dt)
        for iy in range(gh):
            for ix in range(gw):
                acc = (acc + val[:, :, iy, :, ix]).astype(dt)
        out[r] = acc / dt(max(gh * gw, 1))
    return out


def roi_align_backward(feat_shapes, rois, dout, featmap_strides=(4, 8, 16, 32), out_size=7, sampling_ratio=2,
                       finest_scale=56):
    """float64 level gradients (B, C, H, W) of ``dout`` (R, C, S, S), each term (g / count) * w_k with the spec's
    fp32 weights; also, per pixel, the number of terms n (B, 1, H, W) and the sum of |terms| (B, C, H, W)."""
    S = out_size
    dout = np.asarray(dout, np.float64)
    grads = [np.zeros(s, np.float64) for s in feat_shapes]
    nterm = [np.zeros((s[0], 1, s[2], s[3]), np.float64) for s in feat_shapes]
    absum = [np.zeros(s, np.float64) for s in feat_shapes]
    dummy = [np.zeros((s[0], 1, s[2], s[3]), f32) for s in feat_shapes]
    for r, b, lv, (oky, yl, yh, ly, hy), (okx, xl, xh, lx, hx), gh, gw in _rows(dummy, rois, featmap_strides, S,
                                                                                   sampling_ratio, finest_scale):
        if gh == 0 or gw == 0:
            continue
        y0, y1 = int(min(yl.min(), yh.min())), int(max(yl.max(), yh.max())) + 1
        x0, x1 = int(min(xl.min(), xh.min())), int(max(xl.max(), xh.max())) + 1
        # corner-weight matrices of the window: My[s, y] = weight of sample row s on pixel row y (duplicates add)
        My = np.zeros((len(yl), y1 - y0))
        Iy = np.zeros_like(My)
        for lo_hi, wgt in ((yl, hy), (yh, ly)):
            np.add.at(My, (np.arange(len(yl)), lo_hi - y0), np.where(oky, wgt.astype(np.float64), 0.0))
            np.add.at(Iy, (np.arange(len(yl)), lo_hi - y0), oky.astype(np.float64))
        Mx = np.zeros((len(xl), x1 - x0))
        Ix = np.zeros_like(Mx)
        for lo_hi, wgt in ((xl, hx), (xh, lx)):
            np.add.at(Mx, (np.arange(len(xl)), lo_hi - x0), np.where(okx, wgt.astype(np.float64), 0.0))
            np.add.at(Ix, (np.arange(len(xl)), lo_hi - x0), okx.astype(np.float64))
        gc = dout[r] / float(max(gh * gw, 1))                          # (C, S, S)
        G = np.repeat(np.repeat(gc, gh, axis=1), gw, axis=2)           # (C, S*gh, S*gw)
        grads[lv][b, :, y0:y1, x0:x1] += np.einsum("sy,csx,xw->cyw", My, G, Mx, optimize=True)
        absum[lv][b, :, y0:y1, x0:x1] += np.einsum("sy,csx,xw->cyw", My, np.abs(G), Mx, optimize=True)
        nterm[lv][b, 0, y0:y1, x0:x1] += Iy.T @ np.ones((len(yl), len(xl))) @ Ix
    return grads, nterm, absum
