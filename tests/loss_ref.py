"""NumPy restatement of the loss spec: the CPU oracle of csrc/loss.hip.

Twice: in float64 for the values (losses and every gradient), and in float32 with the spec's operation order for what
must match bit for bit (the smooth-L1 gradients: a subtraction, a division by beta or a sign, two multiplications and
the one division ``s = g / avg``).  ``beta``, ``gamma`` and ``alpha`` are rounded to float32 once, as the C ABI carries
them; ``1 - alpha`` is a float32 subtraction.  Head outputs come as float32 arrays holding the STORED values (a bf16 /
fp16 tensor converted exactly).

Every function returns a dict: ``losses`` (2,) float64 = sums / avg, ``mag`` (2,) = sum |w * l| / avg, ``avg`` (the
float32 divisor), the float64 gradients, the float32 smooth-L1 gradients, and ``scale`` / ``D``: per element |w * s|
and the focal factor ``gamma * max(sp(x), sp(-x)) + 1`` (1 for BCE and CE) of the error bound.
"""
import numpy as np

F32 = np.float32


def divisor(avg_factor, count=None):
    """The float32 divisor: a number as it is; integer arrays: their sum, at least 1; None: ``count``, at least 1."""
    if avg_factor is None:
        return F32(max(int(count), 1))
    if isinstance(avg_factor, (tuple, list)) or isinstance(avg_factor, np.ndarray):
        parts = avg_factor if isinstance(avg_factor, (tuple, list)) else (avg_factor,)
        return F32(max(sum(int(np.asarray(p, np.int64).sum()) for p in parts), 1))
    return F32(avg_factor)


def _e(z):
    return np.exp(-np.abs(z))


def sp(z):
    return np.maximum(z, 0) + np.log1p(_e(z))


def sigma(z):
    e = _e(z)
    return np.where(z >= 0, 1 / (1 + e), e / (1 + e))


def cls_elem(x, t, gamma, alpha):
    """(loss, d loss / d x) per element in float64; ``t`` boolean; ``gamma`` None: binary cross entropy."""
    x = np.asarray(x, np.float64)
    if gamma is None:
        return np.where(t, sp(-x), sp(x)), np.where(t, -sigma(-x), sigma(x))
    g, a = float(F32(gamma)), float(F32(alpha))
    na = float(F32(1) - F32(alpha))
    p = sigma(x)
    l1 = a * np.exp(-g * sp(x)) * sp(-x)
    d1 = -a * np.exp(-g * sp(x)) * (g * p * sp(-x) + sigma(-x))
    l0 = na * np.exp(-g * sp(-x)) * sp(x)
    d0 = na * np.exp(-g * sp(-x)) * (g * sigma(-x) * sp(x) + p)
    return np.where(t, l1, l0), np.where(t, d1, d0)


def smooth_l1(pred, target, beta):
    """(loss, gradient) in float64 on the float32 difference's exact operands."""
    b = float(F32(beta))
    d = np.asarray(pred, np.float64) - np.asarray(target, np.float64)
    ad = np.abs(d)
    return np.where(ad < b, 0.5 * d * d / b, ad - 0.5 * b), np.where(ad < b, d / b, np.sign(d))


def smooth_l1_grad32(pred, target, w, s, beta):
    """``(w * dl) * s`` in float32, operation by operation; elements with w == 0 are exactly 0."""
    b = F32(beta)
    with np.errstate(all="ignore"):
        d = pred.astype(F32) - target.astype(F32)
        dl = np.where(np.abs(d) < b, d / b, np.sign(d)).astype(F32)
        out = (w.astype(F32) * dl) * F32(s)
    return np.where(w != 0, out, F32(0)).astype(F32)


def flatten_head(x, A, K):
    """(B, A*K, H, W) -> (B, H*W*A, K): anchor (h*W + w)*A + a, channel a*K + k."""
    B, _, H, W = x.shape
    return x.reshape(B, A, K, H, W).transpose(0, 3, 4, 1, 2).reshape(B, H * W * A, K)


def unflatten_head(y, A, K, H, W):
    B = y.shape[0]
    return y.reshape(B, H, W, A, K).transpose(0, 3, 4, 1, 2).reshape(B, A * K, H, W)


def _masked(w, f):
    """``f`` where w != 0, else exactly 0 — whatever ``f`` holds there (NaN, Inf)."""
    with np.errstate(all="ignore"):
        return np.where(w != 0, f, 0.0)


def anchor_head_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, avg_factor,
                     num_classes=1, beta=1.0 / 9.0, gamma=None, alpha=0.25, g=(1.0, 1.0)):
    C = int(num_classes)
    A = cls_scores[0].shape[1] // C
    avg = divisor(avg_factor)
    g32 = np.asarray(g, F32)
    s32 = g32 / avg
    s64 = s32.astype(np.float64)
    x = np.concatenate([flatten_head(np.asarray(c, np.float64), A, C) for c in cls_scores], 1)      # (B, N, C)
    r = np.concatenate([flatten_head(np.asarray(c, F32), A, 4) for c in bbox_preds], 1)             # (B, N, 4)
    t = labels[..., None] == np.arange(1, C + 1)
    w = np.broadcast_to(label_weights[..., None].astype(np.float64), x.shape)
    with np.errstate(all="ignore"):
        l, dl = cls_elem(x, t, gamma, alpha)
        rl, rdl = smooth_l1(r, bbox_targets, beta)
    bw64 = bbox_weights.astype(np.float64)
    with np.errstate(all="ignore"):
        wl, wr = _masked(w, w * l), _masked(bbox_weights, bbox_weights * rl)
        dx = _masked(w, (w * dl) * s64[0])
        dr = _masked(bbox_weights, (bw64 * rdl) * s64[1])
    dr32 = smooth_l1_grad32(r, bbox_targets, bbox_weights, s32[1], beta)
    if gamma is None:
        D = np.ones_like(x)
    else:
        with np.errstate(all="ignore"):
            D = _masked(w, float(F32(gamma)) * np.maximum(sp(x), sp(-x)) + 1.0)
    out = dict(avg=avg, losses=np.array([wl.sum(), wr.sum()]) / float(avg),
               mag=np.array([np.abs(wl).sum(), np.abs(wr).sum()]) / float(avg),
               dcls=[], dreg=[], dreg32=[], scale_cls=[], scale_reg=[], D=[])
    n0 = 0
    for c in cls_scores:
        H, W = c.shape[2:]
        n1 = n0 + H * W * A
        out["dcls"].append(unflatten_head(dx[:, n0:n1], A, C, H, W))
        out["D"].append(unflatten_head(D[:, n0:n1], A, C, H, W))
        out["scale_cls"].append(unflatten_head(np.abs(w[:, n0:n1] * s64[0]), A, C, H, W))
        out["dreg"].append(unflatten_head(dr[:, n0:n1], A, 4, H, W))
        out["dreg32"].append(unflatten_head(dr32[:, n0:n1], A, 4, H, W))
        out["scale_reg"].append(unflatten_head(np.abs(bw64[:, n0:n1] * s64[1]), A, 4, H, W))
        n0 = n1
    assert n0 == labels.shape[1]
    return out


def bbox_head_loss(cls_score, bbox_pred, labels, label_weights, bbox_targets, bbox_weights, avg_factor=None,
                   beta=1.0, g=(1.0, 1.0)):
    R, C = cls_score.shape
    cols = bbox_pred.shape[1]
    avg = divisor(avg_factor, (label_weights > 0).sum())
    g32 = np.asarray(g, F32)
    s32 = g32 / avg
    s64 = s32.astype(np.float64)
    inside = (labels >= 0) & (labels < C)
    w = np.where(inside, label_weights, F32(0)).astype(np.float64)            # a label out of range: weight 0
    lab = np.where(inside, labels, 0)
    rows = np.arange(R)
    x = np.asarray(cls_score, np.float64)
    with np.errstate(all="ignore"):
        z = x - x.max(1, keepdims=True)
        ez = np.exp(z)
        S = ez.sum(1, keepdims=True)
        l = np.log(S[:, 0]) - z[rows, lab]
        dl = ez / S
        dl[rows, lab] -= 1.0
    with np.errstate(all="ignore"):
        wl = _masked(w, w * l)
        dcls = _masked(w[:, None], (w[:, None] * dl) * s64[0])
    col = (4 * lab[:, None] if cols != 4 else np.zeros((R, 1), np.int64)) + np.arange(4)
    pred = np.asarray(bbox_pred, F32)[rows[:, None], col]                      # (R, 4)
    bw = np.where(inside[:, None], bbox_weights, F32(0)).astype(F32)
    with np.errstate(all="ignore"):
        rl, rdl = smooth_l1(pred, bbox_targets, beta)
        wr = _masked(bw, bw * rl)
        dreg_v = _masked(bw, (bw.astype(np.float64) * rdl) * s64[1])
    dreg = np.zeros((R, cols))
    dreg32 = np.zeros((R, cols), F32)
    scale_reg = np.zeros((R, cols))
    dreg[rows[:, None], col] = dreg_v
    dreg32[rows[:, None], col] = smooth_l1_grad32(pred, bbox_targets, bw, s32[1], beta)
    scale_reg[rows[:, None], col] = np.abs(bw.astype(np.float64) * s64[1])
    return dict(avg=avg, losses=np.array([wl.sum(), wr.sum()]) / float(avg),
                mag=np.array([np.abs(wl).sum(), np.abs(wr).sum()]) / float(avg),
                dcls=dcls, dreg=dreg, dreg32=dreg32, scale_cls=np.abs(w * s64[0])[:, None] * np.ones((1, C)),
                scale_reg=scale_reg, D=np.ones((R, C)))
