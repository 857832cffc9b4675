"""CPU oracle of the gradient-harmonised losses (csrc/ghm.hip): the spec restated operation for operation
in numpy float32, so that counts, tot, acc, beta, both gradients and every GHM-R element loss can be compared with the
device as bit patterns.  Only GHM-C's element loss goes through a ``log1p`` that the device's ``log1pf`` need not repeat
bit for bit: the oracle gives it in float64 (from the float32 logits, with the float32 beta) and the tests bound the
difference (``K`` below).  ``tests/test_ghm_oracle.py`` pins this file to an independent torch float64 restatement
written the way mmdetection writes it.
"""
import numpy as np

from loss_ref import flatten_head, unflatten_head
from soft_nms_ref import soft_exp

f32 = np.float32
U = 2.0 ** -24
# GHM-C's loss value, in units of u of the sum of the absolute terms: soft_exp 4u; log1pf 2u of its own
# + the 4u it carries; the sum with the exact max 1u; the product with beta 1u
K = 8
MAX_BINS = 64
TABLE_STRIDE = 136


def edges(bins, reg):
    """edge[i] = fp32(i) / fp32(bins), i = 0..bins; GHM-R's last edge is mmdetection's 1e3."""
    e = (np.arange(bins + 1, dtype=f32) / f32(bins)).astype(f32)
    if reg:
        e[bins] = f32(1000.0)
    return e


def bin_of(g, bins, reg=False):
    """The i with edge[i] <= g < edge[i+1], the last bin closed above; -1 for a NaN.  g <= 1 by construction."""
    g = np.asarray(g, f32)
    e = edges(bins, reg)
    ok = ~np.isnan(g)
    assert np.all(g[ok] >= 0) and np.all(g[ok] <= e[bins])
    i = np.searchsorted(e[1:bins], np.where(ok, g, 0), side="right")       # interior edges <= g
    return np.where(ok, i, -1).astype(np.int64)


def elem_cls(x, t):
    """-> (g, l as float64, dl) of GHM-C for float32 logits x and boolean targets t (all evaluated; NaN stays NaN)."""
    x = np.asarray(x, f32)
    t = np.asarray(t, bool)
    with np.errstate(all="ignore"):
        e = soft_exp(-np.abs(x))
        den = (f32(1) + e).astype(f32)
        z = np.where(t, -x, x)                                              # sigma's argument
        g = (np.where(z >= 0, f32(1), e).astype(f32) / den).astype(f32)
        g = np.where(np.isnan(x), x, g).astype(f32)
        dl = np.where(t, -g, g).astype(f32)
        x64 = x.astype(np.float64)
        l = np.maximum(np.where(t, -x64, x64), 0.0) + np.log1p(np.exp(-np.abs(x64)))
        l = np.where(np.isnan(x), np.nan, l)
    return g, l, dl


def elem_reg(pred, target, mu):
    """-> (g, l, dl) of GHM-R, float32 operation for operation."""
    pred, target = np.asarray(pred, f32), np.asarray(target, f32)
    mu = f32(mu)
    mu2 = f32(np.float64(mu) * np.float64(mu))
    with np.errstate(all="ignore"):
        d = (pred - target).astype(f32)
        dd = (d * d).astype(f32)
        q = np.sqrt((dd + mu2).astype(f32)).astype(f32)
        g = (np.abs(d) / q).astype(f32)
        l = (dd / (q + mu).astype(f32)).astype(f32)
        dl = (d / q).astype(f32)
    return g, l, dl


def advance(cnt, tot, acc, momentum):
    """One row's weights: cnt int64 [bins], tot int; acc float32 [bins] is advanced in place (momentum > 0).
    -> (beta float32 [bins], number of non-empty bins)."""
    bins = len(cnt)
    mmt = f32(momentum)
    omm = f32(f32(1) - mmt)
    n = int((cnt != 0).sum())
    beta = np.zeros(bins, f32)
    for i in range(bins):
        if cnt[i] == 0:
            continue
        fc = f32(int(cnt[i]))
        if mmt > 0:
            acc[i] = f32(f32(mmt * acc[i]) + f32(omm * fc))
            w = f32(f32(tot) / acc[i])
        else:
            w = f32(f32(tot) / fc)
        beta[i] = f32(w / f32(n))
    return beta, n


def ghm_head_loss(cls_scores, bbox_preds, labels, label_weights, bbox_targets, bbox_weights, acc_cls, acc_reg,
                  num_classes, bins_cls=30, bins_reg=10, momentum_cls=0.75, momentum_reg=0.7, mu=0.02, scope="level",
                  g=(1.0, 1.0)):
    """numpy float32 head outputs (B, A*C, H, W) / (B, 4A, H, W) per level and ``anchor_target_all``'s targets.
    ``acc_cls`` / ``acc_reg``: float32 arrays advanced IN PLACE (None with momentum 0).  Returns a dict:
      losses    float32 [2]: GHM-R's from its float32 summands, GHM-C's from the float64 element losses
      losses64  the same before the rounding; mag [2]: the sums of the absolute terms, for GHM-C's bound
      cnt, beta [2][rows][64], tot, n, nan [2][rows]: the table
      dcls, dreg   float32 gradients of g[0] loss_cls + g[1] loss_bbox, one per level in the head's shape
      terms_reg    per level the float32 products beta * l of the valid box elements (0 elsewhere), head-shaped"""
    C = int(num_classes)
    L = len(cls_scores)
    B = cls_scores[0].shape[0]
    A = cls_scores[0].shape[1] // C
    rows = 1 if scope == "batch" else L
    bins, mmt, acc = (bins_cls, bins_reg), (momentum_cls, momentum_reg), (acc_cls, acc_reg)
    # per level and kind: flattened (B, n_l, K) views of g, l, dl, valid, bin
    per, n0 = [], 0
    for l in range(L):
        _, _, H, W = cls_scores[l].shape
        n1 = n0 + H * W * A
        x = flatten_head(np.asarray(cls_scores[l], f32), A, C)
        t = labels[:, n0:n1, None] == np.arange(1, C + 1)[None, None, :]
        vc = np.broadcast_to((label_weights[:, n0:n1] > 0)[..., None], x.shape)
        gc, lc, dc = elem_cls(x, t)
        p = flatten_head(np.asarray(bbox_preds[l], f32), A, 4)
        vr = bbox_weights[:, n0:n1] > 0
        gr, lr, dr = elem_reg(p, bbox_targets[:, n0:n1], mu)
        lev = []
        for k, (gg, ll, dd, vv) in enumerate(((gc, lc, dc, vc), (gr, lr, dr, vr))):
            bb = np.full(gg.shape, -1, np.int64)
            bb[vv] = bin_of(gg[vv], bins[k], bool(k))
            lev.append(dict(g=gg, l=ll, dl=dd, valid=vv, bin=bb, shape=(H, W)))
        per.append(lev)
        n0 = n1
    out = dict(cnt=np.zeros((2, rows, MAX_BINS), np.int64), beta=np.zeros((2, rows, MAX_BINS), f32),
               tot=np.ones((2, rows), np.int64), n=np.zeros((2, rows), np.int64), nan=np.zeros((2, rows), np.int64),
               losses64=np.zeros(2), mag=np.zeros(2), dcls=[None] * L, dreg=[None] * L, terms_reg=[None] * L)
    for k in range(2):
        for r in range(rows):
            lv = range(L) if scope == "batch" else [r]
            cnt = np.zeros(bins[k], np.int64)
            valid = 0
            for l in lv:
                e = per[l][k]
                valid += int(e["valid"].sum())
                cnt += np.bincount(e["bin"][e["valid"] & (e["bin"] >= 0)], minlength=bins[k])
            tot = max(valid, 1)
            beta, n = advance(cnt, tot, acc[k], mmt[k])
            out["cnt"][k, r, :bins[k]], out["beta"][k, r, :bins[k]] = cnt, beta
            out["tot"][k, r], out["n"][k, r], out["nan"][k, r] = tot, n, valid - int(cnt.sum())
            s = f32(f32(g[k]) / f32(tot))
            rowsum, rowmag = 0.0, 0.0
            for l in lv:
                e = per[l][k]
                inb = e["valid"] & (e["bin"] >= 0)
                be = np.where(inb, beta[np.maximum(e["bin"], 0)], f32(0)).astype(f32)
                with np.errstate(all="ignore"):
                    if k == 0:
                        term = np.where(inb, be.astype(np.float64) * e["l"], 0.0)
                    else:
                        term = np.where(inb, (be * e["l"]).astype(f32), f32(0)).astype(f32)
                    grad = np.where(inb, ((be * e["dl"]).astype(f32) * s).astype(f32), f32(0)).astype(f32)
                outside = e["valid"] & (e["bin"] < 0)                        # a NaN g goes on as it is
                term = np.where(outside, np.nan, term)
                grad = np.where(outside, f32(np.nan), grad).astype(f32)
                rowsum += float(term.astype(np.float64).sum())
                rowmag += float(np.abs(term[~outside].astype(np.float64)).sum())
                H, W = e["shape"]
                if k == 0:
                    out["dcls"][l] = unflatten_head(grad, A, C, H, W)
                else:
                    out["dreg"][l] = unflatten_head(grad, A, 4, H, W)
                    out["terms_reg"][l] = unflatten_head(term, A, 4, H, W)
            out["losses64"][k] += rowsum / tot
            out["mag"][k] += rowmag / tot
    out["losses"] = out["losses64"].astype(f32)
    return out


def table(ref, rows_max=8):
    """The device's table (2, 8, 136) float32 as the oracle has it."""
    t = np.zeros((2, rows_max, TABLE_STRIDE), f32)
    rows = ref["tot"].shape[1]
    t[:, :, 2 * MAX_BINS] = 1
    t[:, :rows, :MAX_BINS] = ref["beta"]
    t[:, :rows, MAX_BINS:2 * MAX_BINS] = ref["cnt"].astype(f32)
    t[:, :rows, 2 * MAX_BINS] = ref["tot"].astype(f32)
    t[:, :rows, 2 * MAX_BINS + 1] = ref["n"].astype(f32)
    t[:, :rows, 2 * MAX_BINS + 2] = ref["nan"].astype(f32)
    return t
