"""NumPy restatement of the FCOS spec — the CPU oracle of torch_detection_amd.fcos.{fcos_points,
fcos_target, fcos_loss, fcos_detections}.

Points and targets are float32 in the spec's operation order (every numpy float32 operation rounds once, like the
kernels' __f*_rn): the comparison with the GPU is bit for bit.  Losses, gradients and the dense scores / boxes are
float64 from the STORED inputs (a bf16 / fp16 tensor converted exactly; ``scales`` float32), together with the
magnitudes that the a-priori error bounds of §4n are stated in.  The focal term is loss_ref's, the selection is
detect_ref.multiclass_nms, the key order is proposal_ref.key_order's rule.
"""
import numpy as np

import detect_ref as D
import loss_ref as R

f32 = np.float32
ONE, HALF = f32(1), f32(0.5)
U = 2.0 ** -24


# ---- points ---------------------------------------------------------------------------------------------------------------
def points(featmap_sizes, strides):
    """(N, 4) float32 rows (x, y, stride, level), level-major, point h*W + w at (w*s + s//2, h*s + s//2)."""
    out = []
    for l, ((H, W), s) in enumerate(zip(featmap_sizes, strides)):
        h, w = np.divmod(np.arange(H * W), W)
        out.append(np.stack([w * s + s // 2, h * s + s // 2, np.full(H * W, s), np.full(H * W, l)], 1).astype(f32))
    return np.concatenate(out)


# ---- targets --------------------------------------------------------------------------------------------------------------
def target(featmap_sizes, strides, regress_ranges, gt_bboxes, gt_labels, gt_counts, center_sample_radius=None,
           info=None):
    """-> (labels (B, N) i64, bbox_targets (B, N, 4) f32, assigned (B, N) i32, num_pos (B,) i32).  ``info`` (a dict)
    receives ``edge`` (point / ground-truth pairs with a distance of the inside test exactly 0) and ``ties`` (points whose
    winner shares its area with another candidate)."""
    pts = points(featmap_sizes, strides)
    x, y, lev = pts[:, 0], pts[:, 1], pts[:, 3].astype(np.int64)
    lo = np.asarray([r[0] for r in regress_ranges], f32)[lev][:, None]
    hi = np.asarray([r[1] for r in regress_ranges], f32)[lev][:, None]
    gt_all = np.asarray(gt_bboxes, f32)
    Bn, G = gt_all.shape[:2]
    N = pts.shape[0]
    labels, bt = np.zeros((Bn, N), np.int64), np.zeros((Bn, N, 4), f32)
    assigned, num_pos = np.zeros((Bn, N), np.int32), np.zeros((Bn,), np.int32)
    edge = ties = 0
    for b in range(Bn):
        cnt = min(max(int(gt_counts[b]), 0), G) if G else 0
        if cnt == 0:
            continue
        gt = gt_all[b, :cnt]
        x1, y1, x2, y2 = (gt[None, :, k] for k in range(4))
        dl, dt, dr, db = x[:, None] - x1, y[:, None] - y1, x2 - x[:, None], y2 - y[:, None]      # (N, cnt) float32
        if center_sample_radius is None:
            near = np.minimum(np.minimum(dl, dt), np.minimum(dr, db))
        else:
            rs = (f32(center_sample_radius) * pts[:, 2])[:, None]
            cx, cy = (x1 + x2) * HALF, (y1 + y2) * HALF
            bx1, by1 = np.maximum(cx - rs, x1), np.maximum(cy - rs, y1)
            bx2, by2 = np.minimum(cx + rs, x2), np.minimum(cy + rs, y2)
            near = np.minimum(np.minimum(x[:, None] - bx1, y[:, None] - by1),
                              np.minimum(bx2 - x[:, None], by2 - y[:, None]))
        far = np.maximum(np.maximum(dl, dt), np.maximum(dr, db))
        ok = (near > 0) & (far >= lo) & (far <= hi)
        area = ((x2 - x1) + ONE) * ((y2 - y1) + ONE)                                               # (1, cnt) float32
        cand = np.where(ok, np.broadcast_to(area, ok.shape), np.inf)
        j = cand.argmin(1)                                                                         # first of the smallest
        hit = ok.any(1)
        ip = np.nonzero(hit)[0]
        jj = j[ip]
        labels[b, ip] = 1 if gt_labels is None else np.asarray(gt_labels, np.int64)[b, jj]
        bt[b, ip] = np.stack([dl[ip, jj], dt[ip, jj], dr[ip, jj], db[ip, jj]], 1)
        assigned[b, ip] = jj + 1
        num_pos[b] = ip.shape[0]
        edge += int((near == 0).sum())
        ties += int(((cand == cand.min(1, keepdims=True)).sum(1)[ip] >= 2).sum())
    if info is not None:
        info["edge"], info["ties"] = info.get("edge", 0) + edge, info.get("ties", 0) + ties
    return labels, bt, assigned, num_pos


# ---- loss -----------------------------------------------------------------------------------------------------------------
def rows(t):
    """(B, Ch, H, W) -> (B, H*W, Ch), point h*W + w."""
    t = np.asarray(t)
    Bn, Ch, H, W = t.shape
    return t.reshape(Bn, Ch, H * W).transpose(0, 2, 1)


def unrows(y, H, W):
    Bn, _, Ch = y.shape
    return np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(Bn, Ch, H, W)


def centerness_target(t):
    """c* of (.., 4) float64 target distances (l*, t*, r*, b*)."""
    lr = np.minimum(t[..., 0], t[..., 2]) / np.maximum(t[..., 0], t[..., 2])
    tb = np.minimum(t[..., 1], t[..., 3]) / np.maximum(t[..., 1], t[..., 3])
    return np.sqrt(lr * tb)


def box_terms(d, t, giou, eps):
    """Predicted and target distances (P, 4) float64 -> (loss (P,), d loss / d d_j (P, 4), M (P, 4), iou (P,)).  ``M`` is
    the derivative with every subtraction turned into an addition: what the rounding errors are relative to."""
    wp, hp = d[:, 0] + d[:, 2] + 1, d[:, 1] + d[:, 3] + 1
    wt, ht = t[:, 0] + t[:, 2] + 1, t[:, 1] + t[:, 3] + 1
    m = np.minimum(d, t)
    wi, hi = m[:, 0] + m[:, 2] + 1, m[:, 1] + m[:, 3] + 1
    ap, at, I = wp * hp, wt * ht, wi * hi
    Un = ap + at - I
    iou = I / Un
    zero = np.zeros_like(iou)
    if giou:
        e = np.maximum(d, t)
        we, he = e[:, 0] + e[:, 2] + 1, e[:, 1] + e[:, 3] + 1
        E = we * he
        loss = 1 - (iou - (E - Un) / E)
        cI, cA, cE = 1 / E - (Un + I) / Un ** 2, I / Un ** 2 - 1 / E, Un / E ** 2
        aI, aA, aE = 1 / E + (Un + I) / Un ** 2, I / Un ** 2 + 1 / E, cE
    else:
        we = he = zero
        loss = -np.log(np.maximum(iou, eps))
        live = iou >= eps
        cI, cA, cE = np.where(live, -(Un + I) / (I * Un), 0.0), np.where(live, 1 / Un, 0.0), zero
        aI, aA, aE = -cI, cA, zero
    oA, oI, oE = (np.stack([v, h, v, h], 1) for v, h in ((hp, wp), (hi, wi), (he, we)))
    mI, mE = d <= t, (d >= t) & bool(giou)
    dd = cA[:, None] * oA + mI * cI[:, None] * oI + mE * cE[:, None] * oE
    M = aA[:, None] * oA + mI * aI[:, None] * oI + mE * aE[:, None] * oE
    return loss, dd, M, iou


# a-priori constants of DESIGN.md §4n, in units of u = 2^-24 (Dx = max_j |s x_j| of the point):
#   box loss  |dL| <= (LOSS_C + LOSS_D Dx + 2 |L| [iou]) u;  box gradient  <= (GRAD_C + GRAD_D Dx) u M |s s_box| c d_j
LOSS_C, LOSS_D = {False: 36.0, True: 86.0}, {False: 6.0, True: 14.0}
GRAD_C, GRAD_D = {False: 84.0, True: 102.0}, {False: 12.0, True: 14.0}
# §4e states its bounds with K = 16 where the operation count of the plain sigmoid terms gives 9: the same margin, 16/9, is
# applied to every count derived in §4n; the focal terms keep §4e's own K = 16 with its factor D
MARGIN = 16.0 / 9.0
K_FOCAL = 16.0


def loss(cls_scores, bbox_preds, centernesses, labels, bbox_targets, scales=None, loss_type="iou", gamma=2.0,
         alpha=0.25, eps=1e-6, g=(1.0, 1.0, 1.0)):
    """float64 losses and gradients of ``g . losses`` from the stored inputs.  Returns a dict: ``losses`` (3,), ``norm``
    (the three divisors), ``dcls`` / ``dreg`` / ``dctr`` (lists, (B, Ch, H, W)), ``dscale`` (L,) or None, ``num_pos``, and
    for the bounds ``bound_losses`` (3,), ``bound_dcls`` / ``bound_dreg`` / ``bound_dctr`` (lists) and ``bound_dscale``:
    the error bounds of §4n in absolute terms, margin included, WITHOUT the final rounding of the output; ``iou`` (P,)."""
    giou = loss_type == "giou"
    labels = np.asarray(labels, np.int64)
    Bn, N = labels.shape
    C = np.asarray(cls_scores[0]).shape[1]
    sizes = [np.asarray(c).shape[2:] for c in cls_scores]
    L = len(sizes)
    lev = np.concatenate([np.full(h * w, l) for l, (h, w) in enumerate(sizes)])
    s_lev = np.ones(L) if scales is None else np.asarray(scales, f32).astype(np.float64)
    x = np.concatenate([rows(np.asarray(c, np.float64)) for c in cls_scores], 1)                   # (B, N, C)
    r = np.concatenate([rows(np.asarray(c, np.float64)) for c in bbox_preds], 1)                   # (B, N, 4)
    z = np.concatenate([rows(np.asarray(c, np.float64)) for c in centernesses], 1)[..., 0]         # (B, N)
    assert x.shape[1] == N
    g32 = np.asarray(g, f32)
    pos = labels > 0
    npos = int(pos.sum())
    d_cls, d_ctr = f32(npos + Bn), f32(max(npos, 1))
    s_cls, s_ctr = float(g32[0] / d_cls), float(g32[2] / d_ctr)

    t1 = labels[..., None] == np.arange(1, C + 1)
    with np.errstate(all="ignore"):
        l, dl = R.cls_elem(x, t1, gamma, alpha)
        Df = float(f32(gamma)) * np.maximum(R.sp(x), R.sp(-x)) + 1.0
    dx = dl * s_cls

    bi, ii = np.nonzero(pos)
    sl = s_lev[lev[ii]][:, None]
    xr = r[bi, ii]
    sx = sl * xr
    d = np.exp(sx)
    tt = np.asarray(bbox_targets, f32).astype(np.float64)[bi, ii]
    c = centerness_target(tt)
    Lb, dd, M, iou = box_terms(d, tt, giou, float(f32(eps)))
    csum = float(c.sum())
    s_box = float(g32[1]) / csum if csum > 0 else 0.0
    zz = z[bi, ii]
    lc = R.sp(zz) - c * zz
    losses = np.array([l.sum() / float(d_cls), (c * Lb).sum() / csum if csum > 0 else 0.0, lc.sum() / float(d_ctr)])
    Dx = np.abs(sx).max(1) if npos else np.zeros(0)
    bl_box = (c * (LOSS_C[giou] + LOSS_D[giou] * Dx + (8.0 if not giou else 6.0) * np.abs(Lb))).sum() / csum \
        if csum > 0 else 0.0
    bound_losses = U * np.array([K_FOCAL * (l * Df).sum() / float(d_cls), MARGIN * bl_box,
                                 MARGIN * 6.0 * (R.sp(zz) + np.abs(c * zz)).sum() / float(d_ctr)])

    e = c[:, None] * dd * d                                                                         # (P, 4)
    dr = np.zeros((Bn, N, 4))
    dr[bi, ii] = e * sl * s_box
    b_dr = np.zeros((Bn, N, 4))
    k_grad = MARGIN * (GRAD_C[giou] + GRAD_D[giou] * Dx)[:, None] * U if npos else np.zeros((0, 1))
    b_dr[bi, ii] = k_grad * M * np.abs(sl * s_box) * c[:, None] * d
    dz = np.zeros((Bn, N))
    dz[bi, ii] = (R.sigma(zz) - c) * s_ctr
    b_dz = np.zeros((Bn, N))
    b_dz[bi, ii] = MARGIN * 8.0 * U * (R.sigma(zz) + c) * abs(s_ctr)
    dscale = b_dscale = None
    if scales is not None:
        dscale, b_dscale = np.zeros(L), np.zeros(L)
        np.add.at(dscale, lev[ii], (e * xr).sum(1) * s_box)
        np.add.at(b_dscale, lev[ii], (k_grad * M * c[:, None] * d * np.abs(xr)).sum(1) * abs(s_box))

    out = dict(losses=losses, norm=np.array([float(d_cls), csum, float(d_ctr)]), num_pos=npos, iou=iou,
               bound_losses=bound_losses, dscale=dscale, bound_dscale=b_dscale, dcls=[], dreg=[], dctr=[],
               bound_dcls=[], bound_dreg=[], bound_dctr=[])
    n0 = 0
    for H, W in sizes:
        n1 = n0 + H * W
        out["dcls"].append(unrows(dx[:, n0:n1], H, W))
        out["bound_dcls"].append(unrows(K_FOCAL * U * abs(s_cls) * Df[:, n0:n1], H, W))
        out["dreg"].append(unrows(dr[:, n0:n1], H, W))
        out["bound_dreg"].append(unrows(b_dr[:, n0:n1], H, W))
        out["dctr"].append(unrows(dz[:, n0:n1, None], H, W))
        out["bound_dctr"].append(unrows(b_dz[:, n0:n1, None], H, W))
        n0 = n1
    return out


# ---- detections -----------------------------------------------------------------------------------------------------------
SEG_MAX, MAX_ROWS = 4096, 1 << 18


def sg(v):
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def kept_points(keys, nms_pre, info=None):
    """The points kept of one (image, level), ascending: the nms_pre first by (key desc, point asc), or all of them.
    ``info`` receives, for a level that selects, the cut key, the points above it, the ties at it and the ties taken."""
    n = keys.shape[0]
    if not 0 < nms_pre < n:
        return np.arange(n)
    order = np.lexsort((np.arange(n), -keys))[:nms_pre]
    if info is not None:
        cut = keys[order[-1]]
        above = int((keys > cut).sum())
        info.setdefault("cuts", []).append(dict(cut=float(cut), above=above, ties=int((keys == cut).sum()),
                                                taken=nms_pre - above))
    return np.sort(order)


def plan(level_sizes, nms_pre):
    k = [nms_pre if 0 < nms_pre < n else n for n in level_sizes]
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    return k, off[:-1], int(off[-1])


def dense(cls_scores, bbox_preds, centernesses, strides, img_shapes, scales=None, scale_factors=None, nms_pre=1000,
          info=None):
    """The dense rows in float64 -> dict: scores (B*K, C+1), boxes (B*K, 4), batch_idx i32, point_idx i64, and for the
    bounds cls (B*K, C) / ctr (B*K,) (the stored logits of every score), sx (B*K, 4) = s*x, dist (B*K, 4) = exp(s*x),
    centre (B*K, 4) = |x| / |y| of the point per box column, scale (B*K,); ``info['keys']``: per (image, level) the float64
    keys with the |a| + |c| of each (a = the class maximum)."""
    Bn, C = np.asarray(cls_scores[0]).shape[:2]
    L = len(cls_scores)
    s_lev = np.ones(L) if scales is None else np.asarray(scales, f32).astype(np.float64)
    scale = None
    if scale_factors is not None:
        s = np.asarray(scale_factors, f32).reshape(-1).astype(np.float64)
        scale = np.broadcast_to(s, (Bn,)) if s.shape[0] == 1 else s
    lv = [(rows(np.asarray(c, np.float64)), rows(np.asarray(r, np.float64)), rows(np.asarray(z, np.float64))[..., 0])
          for c, r, z in zip(cls_scores, bbox_preds, centernesses)]
    pts = [points([np.asarray(c).shape[2:]], [s]).astype(np.float64) for c, s in zip(cls_scores, strides)]
    out = {k: [] for k in ("cls", "ctr", "sx", "dist", "centre", "boxes", "batch_idx", "point_idx", "scale")}
    for b in range(Bn):
        ih, iw = int(img_shapes[b][0]), int(img_shapes[b][1])
        poff = 0
        for l, (x, r, z) in enumerate(lv):
            a = x[b].max(1)
            keys = sg(a) * sg(z[b])
            if info is not None:
                info.setdefault("keys", []).append((keys, np.abs(a) + np.abs(z[b])))
            keep = kept_points(keys, nms_pre, info)
            px, py = pts[l][keep, 0], pts[l][keep, 1]
            sx = s_lev[l] * r[b][keep]
            d = np.exp(sx)
            bx = np.stack([np.clip(px - d[:, 0], 0, iw - 1), np.clip(py - d[:, 1], 0, ih - 1),
                           np.clip(px + d[:, 2], 0, iw - 1), np.clip(py + d[:, 3], 0, ih - 1)], 1)
            out["cls"].append(x[b][keep])
            out["ctr"].append(z[b][keep])
            out["sx"].append(sx)
            out["dist"].append(d)
            out["centre"].append(np.stack([px, py, px, py], 1))
            out["boxes"].append(bx if scale is None else bx / scale[b])
            out["batch_idx"].append(np.full(keep.shape[0], b, np.int32))
            out["point_idx"].append(poff + keep.astype(np.int64))
            out["scale"].append(np.full(keep.shape[0], 1.0 if scale is None else scale[b]))
            poff += x.shape[1]
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["scores"] = np.concatenate([np.zeros((out["cls"].shape[0], 1)), sg(out["cls"]) * sg(out["ctr"])[:, None]], 1)
    return out


def select(dense_boxes, dense_scores, batch_idx, dense_point_idx, num_imgs, score_thr=0.05, nms_thr=0.5,
           max_per_img=100, stats=None):
    """tdn_multiclass_nms and the gather on given float32 dense tensors -> (dets, labels, point_idx, counts, row_idx)."""
    dets, labels, rws, counts = D.multiclass_nms(np.asarray(dense_boxes, f32), np.asarray(dense_scores, f32), batch_idx,
                                                 num_imgs, score_thr, nms_thr, max_per_img, stats)
    pidx = np.where(rws >= 0, np.asarray(dense_point_idx, np.int64)[np.maximum(rws, 0)], -1)
    return dets, labels, pidx, counts, rws


def detections(cls_scores, bbox_preds, centernesses, strides, img_shapes, scales=None, scale_factors=None,
               nms_pre=1000, score_thr=0.05, nms_thr=0.5, max_per_img=100, info=None, stats=None):
    """The whole spec on the CPU, the dense tensors rounded to float32 before the selection -> (dets, labels, point_idx,
    counts, dense_scores, dense_boxes, batch_idx, dense_point_idx, row_idx)."""
    d = dense(cls_scores, bbox_preds, centernesses, strides, img_shapes, scales, scale_factors, nms_pre, info)
    Bn = np.asarray(cls_scores[0]).shape[0]
    sc, bx = d["scores"].astype(f32), d["boxes"].astype(f32)
    dets, labels, pidx, counts, rws = select(bx, sc, d["batch_idx"], d["point_idx"], Bn, score_thr, nms_thr, max_per_img,
                                             stats)
    return dets, labels, pidx, counts, sc, bx, d["batch_idx"], d["point_idx"], rws
