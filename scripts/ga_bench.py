#!/usr/bin/env python
"""The Guided Anchoring operations at the GA-RPN shape — B = 2, 800 x 1344, strides 4..64, A = 9 approxs
per location, G in {8, 64} ground truths per image, bf16 channels_last head outputs — each replayed from a captured
graph, beside the same computation composed from torch operations along mmdetection v1's code path on the same GPU:

  ga_loc_target     the Python loop over the ground truths with its ``.item()`` reads and slice assignments (eager)
  ga_shape_target   the (9 Nloc) x G IoU matrix, its maximum over the approxs, MaxIoUAssigner's steps with the loop over
                    the ground truths, RandomSampler through ``nonzero`` and ``randperm`` (eager: it synchronises)
  guided_anchors    permute / reshape, delta2bbox and the sigmoid threshold (no synchronisation: replayed from a graph too)
  ga_loss           sigmoid focal loss of the location map and bounded_iou_loss on the ``nonzero`` rows, autograd (eager)
  ga_rpn_proposals  GARPNHead.get_bboxes: per image and level the mask select, sigmoid, top-k, delta2bbox, min-size filter
                    and NMS, then the per-image top-k (eager: boolean indexing synchronises).  There is no torch NMS
                    here, so the composition's NMS step is this library's own ``nms`` — as mmdetection calls its compiled
                    one — and only the steps around it are torch

Device events after warm-up; the graph of an op and its baseline alternate over ``--repeats`` windows and the spread is
printed.  Bytes: every input and every output of the op once, computed from the shapes.  One JSON object per line."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch_detection_amd as T  # noqa: E402
import ga_cases as K  # noqa: E402
from ghm_bench import graphed  # noqa: E402
from proposal_bench import time_events  # noqa: E402

SIZES = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
STRIDES = K.STRIDES
IMG = (800, 1344)
SCALE = 8
MEANS, STDS = (0.0, 0.0, 0.0, 0.0), (0.07, 0.07, 0.14, 0.14)
CLIP = abs(math.log(1e-6))


def inputs(B, G, seed=0):
    g = np.random.default_rng(seed)
    side = np.exp(g.uniform(np.log(16), np.log(600), (B, G, 2)))
    x1 = g.uniform(0, 1, (B, G)) * (IMG[1] - side[..., 0]).clip(1)
    y1 = g.uniform(0, 1, (B, G)) * (IMG[0] - side[..., 1]).clip(1)
    gt = np.stack([x1, y1, x1 + side[..., 0], y1 + side[..., 1]], -1).astype(np.float32)
    heads = []
    for ch in (1, 2):
        heads.append([torch.from_numpy(g.normal(0, 1.5, (B, ch, h, w)).astype(np.float32)).cuda().to(torch.bfloat16)
                      .contiguous(memory_format=torch.channels_last) for h, w in SIZES])
    return (torch.from_numpy(gt).cuda(), torch.full((B,), G, dtype=torch.int32, device="cuda"), heads[0], heads[1],
            torch.from_numpy(K.approxs_of(SIZES, 9)).cuda(), torch.from_numpy(K.squares_of(SIZES)).cuda(),
            torch.tensor([IMG] * B, dtype=torch.int32, device="cuda"))


# ---- the compositions ---------------------------------------------------------------------------------------------------------
def _region(box, ratio, size):
    x1 = torch.round((1 - ratio) * box[0] + ratio * box[2]).long().clamp(0, size[1] - 1)
    y1 = torch.round((1 - ratio) * box[1] + ratio * box[3]).long().clamp(0, size[0] - 1)
    x2 = torch.round(ratio * box[0] + (1 - ratio) * box[2]).long().clamp(0, size[1] - 1)
    y2 = torch.round(ratio * box[1] + (1 - ratio) * box[3]).long().clamp(0, size[0] - 1)
    return x1, y1, x2, y2


def eager_loc_target(gt, center_ratio=0.2, ignore_ratio=0.5):
    B, L = gt.shape[0], len(SIZES)
    r1, r2 = (1 - center_ratio) / 2, (1 - ignore_ratio) / 2
    tg = [torch.zeros(B, 1, h, w, device=gt.device) for h, w in SIZES]
    wt = [torch.full((B, 1, h, w), -1.0, device=gt.device) for h, w in SIZES]
    ig = [torch.zeros(B, 1, h, w, device=gt.device) for h, w in SIZES]
    for b in range(B):
        scale = torch.sqrt((gt[b, :, 2] - gt[b, :, 0] + 1) * (gt[b, :, 3] - gt[b, :, 1] + 1))
        lvls = torch.floor(torch.log2(scale) - math.log2(SCALE * STRIDES[0]) + 0.5).clamp(0, L - 1).long()
        for j in range(gt.shape[1]):
            l = lvls[j].item()
            box = gt[b, j] / STRIDES[l]
            ix1, iy1, ix2, iy2 = _region(box, r2, SIZES[l])
            cx1, cy1, cx2, cy2 = _region(box, r1, SIZES[l])
            tg[l][b, 0, cy1:cy2 + 1, cx1:cx2 + 1] = 1
            wt[l][b, 0, iy1:iy2 + 1, ix1:ix2 + 1] = 0
            wt[l][b, 0, cy1:cy2 + 1, cx1:cx2 + 1] = 1
            for d in (l - 1, l + 1):
                if 0 <= d < L:
                    x1, y1, x2, y2 = _region(gt[b, j] / STRIDES[d], r2, SIZES[d])
                    ig[d][b, 0, y1:y2 + 1, x1:x2 + 1] = 1
    for l in range(L):
        wt[l][(wt[l] < 0) & (ig[l] > 0)] = 0
        wt[l][wt[l] < 0] = 0.1
    return tg, wt


def _iou(a, b):
    lt, rb = torch.max(a[:, None, :2], b[None, :, :2]), torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    aa = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    ab = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    return inter / (aa[:, None] + ab[None] - inter)


def eager_shape_target(approxs, squares, gt, img_shapes, num=256):
    N, A, _ = approxs.shape
    flat = approxs.reshape(-1, 4)
    out = []
    for b in range(gt.shape[0]):
        h, w = img_shapes[b].tolist()
        inside = ((flat[:, 0] >= 0) & (flat[:, 1] >= 0) & (flat[:, 2] < w) & (flat[:, 3] < h)).view(N, A).any(1)
        ov = _iou(flat, gt[b]).view(N, A, -1).max(dim=1)[0]                  # the (9 Nloc) x G matrix
        ov = ov[inside]
        mx, am = ov.max(dim=1)
        assigned = ov.new_full((ov.shape[0],), -1, dtype=torch.long)
        assigned[(mx >= 0) & (mx < 0.3)] = 0
        assigned[mx >= 0.7] = am[mx >= 0.7] + 1
        gmax = ov.max(dim=0)[0]
        for j in range(gt.shape[1]):
            if gmax[j] >= 0.3:
                assigned[ov[:, j] == gmax[j]] = j + 1
        pos, neg = torch.nonzero(assigned > 0).flatten(), torch.nonzero(assigned == 0).flatten()
        pos = pos[torch.randperm(pos.numel(), device=pos.device)[:num // 2]]
        neg = neg[torch.randperm(neg.numel(), device=neg.device)[:num - pos.numel()]]
        idx = torch.nonzero(inside).flatten()
        an, gs, ws = (squares.new_zeros(N, 4) for _ in range(3))
        an[idx[pos]], gs[idx[pos]], ws[idx[pos]] = squares[idx[pos]], gt[b][assigned[pos] - 1], 1.0
        out.append((an, gs, ws))
    return out


def _delta2bbox(rois, d):
    dx, dy = d[:, 0] * STDS[0] + MEANS[0], d[:, 1] * STDS[1] + MEANS[1]      # scalars: nothing is copied from the host
    dw = (d[:, 2] * STDS[2] + MEANS[2]).clamp(-CLIP, CLIP)
    dh = (d[:, 3] * STDS[3] + MEANS[3]).clamp(-CLIP, CLIP)
    px, py = (rois[:, 0] + rois[:, 2]) * 0.5, (rois[:, 1] + rois[:, 3]) * 0.5
    pw, ph = rois[:, 2] - rois[:, 0] + 1, rois[:, 3] - rois[:, 1] + 1
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * dx, py + ph * dy
    return torch.stack([gx - gw * 0.5 + 0.5, gy - gh * 0.5 + 0.5, gx + gw * 0.5 - 0.5, gy + gh * 0.5 - 0.5], -1)


def torch_guided_anchors(shape, loc, squares, thr):
    B = shape[0].shape[0]
    s = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1, 2) for p in shape], 1).float()
    z = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1) for p in loc], 1).float()
    d = torch.cat([torch.zeros_like(s), s], 2)
    anchors = torch.stack([_delta2bbox(squares, d[b]) for b in range(B)])
    return anchors, z.sigmoid() >= thr


def eager_loss(loc, shape, lt, lw, an, gs, ws, loc_avg, avg, gamma=2.0, alpha=0.25, beta=0.2, eps=1e-3):
    B = lt.shape[0]
    z = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1) for p in loc], 1).float()
    s = torch.cat([p.permute(0, 2, 3, 1).reshape(B, -1, 2) for p in shape], 1).float()
    t = lt.float()
    p = z.sigmoid()
    pt = (1 - p) * t + p * (1 - t)
    fw = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    loss_loc = (torch.nn.functional.binary_cross_entropy_with_logits(z, t, reduction="none") * fw * lw).sum() / loc_avg
    inds = torch.nonzero(ws[..., 0].reshape(-1) > 0).flatten()               # the host synchronisation
    d = torch.cat([torch.zeros_like(s), s], 2).reshape(-1, 4)[inds]
    pred, tgt, w = _delta2bbox(an.reshape(-1, 4)[inds], d), gs.reshape(-1, 4)[inds], ws.reshape(-1, 4)[inds]
    pcx, pcy = (pred[:, 0] + pred[:, 2]) * 0.5, (pred[:, 1] + pred[:, 3]) * 0.5
    pw, ph = pred[:, 2] - pred[:, 0] + 1, pred[:, 3] - pred[:, 1] + 1
    tcx, tcy = (tgt[:, 0] + tgt[:, 2]) * 0.5, (tgt[:, 1] + tgt[:, 3]) * 0.5
    tw, th = tgt[:, 2] - tgt[:, 0] + 1, tgt[:, 3] - tgt[:, 1] + 1
    dx, dy = tcx - pcx, tcy - pcy
    comb = torch.stack([1 - torch.max((tw - 2 * dx.abs()) / (tw + 2 * dx.abs() + eps), torch.zeros_like(dx)),
                        1 - torch.max((th - 2 * dy.abs()) / (th + 2 * dy.abs() + eps), torch.zeros_like(dy)),
                        1 - torch.min(tw / (pw + eps), pw / (tw + eps)),
                        1 - torch.min(th / (ph + eps), ph / (th + eps))], -1)
    l = torch.where(comb < beta, 0.5 * comb * comb / beta, comb - 0.5 * beta)
    return torch.stack([loss_loc, (l * w).sum() / avg])


def _decode_clip(rois, d, shape, clip=abs(math.log(16 / 1000))):
    dw, dh = d[:, 2].clamp(-clip, clip), d[:, 3].clamp(-clip, clip)
    px, py = (rois[:, 0] + rois[:, 2]) * 0.5, (rois[:, 1] + rois[:, 3]) * 0.5
    pw, ph = rois[:, 2] - rois[:, 0] + 1, rois[:, 3] - rois[:, 1] + 1
    gw, gh = pw * dw.exp(), ph * dh.exp()
    gx, gy = px + pw * d[:, 0], py + ph * d[:, 1]
    return torch.stack([(gx - gw * 0.5 + 0.5).clamp(0, shape[1] - 1), (gy - gh * 0.5 + 0.5).clamp(0, shape[0] - 1),
                        (gx + gw * 0.5 - 0.5).clamp(0, shape[1] - 1), (gy + gh * 0.5 - 0.5).clamp(0, shape[0] - 1)], -1)


def eager_proposals(cls, reg, anchors, mask, nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7):
    out = []
    for b in range(anchors.shape[0]):
        found, n0 = [], 0
        for c, r in zip(cls, reg):
            n1 = n0 + c.shape[2] * c.shape[3]
            m = mask[b, n0:n1].bool()
            scores = c[b].permute(1, 2, 0).reshape(-1).float().sigmoid()[m]
            deltas = r[b].permute(1, 2, 0).reshape(-1, 4).float()[m]
            anc = anchors[b, n0:n1][m]
            n0 = n1
            if scores.numel() == 0:
                continue
            if 0 < nms_pre < scores.numel():
                scores, top = scores.topk(nms_pre)
                deltas, anc = deltas[top], anc[top]
            boxes = _decode_clip(anc, deltas, IMG)
            dets, _ = T.nms(torch.cat([boxes, scores[:, None]], 1), nms_thr)
            found.append(dets[:nms_post])
        dets = torch.cat(found)
        out.append(dets[dets[:, 4].topk(min(max_num, dets.shape[0]))[1]])
    return out


# ---- timing ---------------------------------------------------------------------------------------------------------------
def spread(v):
    return dict(min=round(min(v), 1), median=round(sorted(v)[len(v) // 2], 1), max=round(max(v), 1))


def record(op, G, ours, base, base_graphed, nbytes, args, extra=None):
    g_ours = graphed(ours)
    g_base = graphed(base) if base_graphed else None
    t_ours, t_base = [], []
    for _ in range(args.repeats):                            # alternating windows: other work shares the machine
        t_ours.append(time_events(g_ours.replay, args.iters))
        t_base.append(time_events(g_base.replay, args.iters) if g_base else time_events(base, args.base_iters))
    med = sorted(t_ours)[len(t_ours) // 2]
    mb = sorted(t_base)[len(t_base) // 2]
    rec = dict(op=op, shape="ga-rpn 800x1344 strides 4..64", B=2, A=9, G=G, nloc=K.nloc(SIZES),
               dtype="bf16 channels_last", iters=args.iters, repeats=args.repeats, graph_replay_us=spread(t_ours),
               torch_composition_us=spread(t_base), composition_is="graph replay" if g_base else "eager",
               composition_over_ours=round(mb / med, 1), bytes=int(nbytes), gbps_at_its_bytes=round(nbytes / med / 1e3, 1))
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--base-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the records to this .jsonl")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ga_bench.py measures on the GPU"
    B, N, A = 2, K.nloc(SIZES), 9
    for G in (8, 64):
        gt, cn, loc, shape, approxs, squares, shapes = inputs(B, G)
        lt, lw, lavg = T.ga_loc_target(SIZES, STRIDES, SCALE, gt, cn)
        st = T.ga_shape_target(approxs, squares, None, gt, cn, shapes)
        npos = int(st[3].sum())
        record("ga_loc_target", G, lambda: T.ga_loc_target(SIZES, STRIDES, SCALE, gt, cn), lambda: eager_loc_target(gt),
               False, B * N * 12 + B * G * 16, args, dict(launches=1))
        record("ga_shape_target", G, lambda: T.ga_shape_target(approxs, squares, None, gt, cn, shapes),
               lambda: eager_shape_target(approxs, squares, gt, shapes), False,
               N * A * 16 + N * 16 + B * G * 16 + B * N * (3 * 16 + 8), args, dict(launches=5, positives=npos))
        if G == 8:                                           # the ground truths play no part in the anchors
            record("guided_anchors", G, lambda: T.guided_anchors(shape, squares, loc, 0.01),
                   lambda: torch_guided_anchors(shape, loc, squares, 0.01), True,
                   B * N * (3 * 2 + 17) + N * 16, args, dict(launches=1))
            g = np.random.default_rng(1)
            reg = [torch.from_numpy(g.normal(0, 0.5, (B, 4, h, w)).astype(np.float32)).cuda().to(torch.bfloat16)
                   .contiguous(memory_format=torch.channels_last) for h, w in SIZES]
            anchors, mask = T.guided_anchors(shape, squares, loc, 0.4)
            pr = T.ga_rpn_proposals(loc, reg, anchors, mask, shapes)
            pe = eager_proposals(loc, reg, anchors, mask)
            # logits and deltas of the locations that are in, their anchors, the mask, the outputs
            inside = int(mask.sum())
            record("ga_rpn_proposals", G, lambda: T.ga_rpn_proposals(loc, reg, anchors, mask, shapes),
                   lambda: eager_proposals(loc, reg, anchors, mask), False,
                   B * N * (2 + 1) + inside * (8 + 16) + B * 2000 * 28, args,
                   dict(launches=4, nms_pre=2000, max_num=2000, locations_in=inside,
                        counts=pr[2].cpu().tolist(), counts_torch_composition=[int(p.shape[0]) for p in pe]))
        leaves = [t.detach().requires_grad_() for t in loc + shape]
        cot = torch.ones(2, device="cuda")
        avg = (st[3], st[4])
        total = float(st[3].sum() + st[4].sum())

        def ours():
            return torch.autograd.grad(T.ga_loss(leaves[:5], leaves[5:], lt, lw, st[0], st[1], st[2], lavg, avg), leaves,
                                       cot)

        def base():
            return torch.autograd.grad(eager_loss(leaves[:5], leaves[5:], lt, lw, st[0], st[1], st[2], lavg, total),
                                       leaves, cot)

        lo = T.ga_loss(leaves[:5], leaves[5:], lt, lw, st[0], st[1], st[2], lavg, avg).detach().cpu().tolist()
        le = eager_loss(leaves[:5], leaves[5:], lt, lw, st[0], st[1], st[2], lavg, total).detach().cpu().tolist()
        # heads read forward and backward, gradients written; the location targets and the row flag read twice
        record("ga_loss fwd+bwd", G, ours, base, False, 3 * B * N * 3 * 2 + 2 * B * N * (8 + 4 + 4), args,
               dict(launches=3, positives=npos, losses=lo, losses_torch_composition=le))


if __name__ == "__main__":
    main()
