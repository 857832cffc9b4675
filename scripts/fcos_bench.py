#!/usr/bin/env python
"""The FCOS operations at the FCOS shape (strides 8..128 at 800 x 1344: 22,400 points per image, C = 80, bf16
channels_last head outputs, 20 ground truths per image), B in {1, 2}: time per call of ``fcos_target``, of ``fcos_loss``
forward + backward and of ``fcos_detections`` (nms_pre 1000, score_thr 0.05, max_per_img 100) replayed from a captured
graph, and of the eager torch composition of the same arithmetic a user writes without them (targets: the (N, G)
distance tensors, masks, ``min`` over areas; loss: permute / reshape, focal from ``sigmoid``, IoU loss, BCE, autograd,
``.item()`` for the divisors; detections: per image and level sigmoid products, ``topk``, gather, decode, then a Python
loop over the 80 classes with one ``box.nms`` each).  Logits come from a fixed seed: a background prior of 0.01 with a
few hundred confident points per image.  Device events after warm-up; the median [min, max] of ``--repeats`` windows
of ``--iters`` calls each.  Prints one JSON object per batch size and appends it to profiles/fcos_bench.jsonl.

``--trace``: only issue eager calls (10 per batch size) for a ``rocprofv3 --kernel-trace --stats`` run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_detection_amd as T  # noqa: E402

C = 80
SHAPE = (800, 1344)
LEVELS = [((100, 168), 8), ((50, 84), 16), ((25, 42), 32), ((13, 21), 64), ((7, 11), 128)]
SIZES, STRIDES = [fs for fs, _ in LEVELS], [s for _, s in LEVELS]
RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, float("inf")))
CFG = dict(nms_pre=1000, score_thr=0.05, nms_thr=0.5, max_per_img=100)
G = 20


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    cl = lambda t: t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)   # noqa: E731
    cls, reg, ctr = [], [], []
    for (H, W), s in LEVELS:
        x = torch.randn(B, C, H, W, generator=g) * 1.2 - 4.6                # sigmoid(-4.6) = 0.01
        hot = torch.rand(B, C, H, W, generator=g) < 2e-4                    # confident points
        x[hot] += 7.0
        cls.append(cl(x))
        reg.append(cl(torch.randn(B, 4, H, W, generator=g) * 0.5 + float(np.log(2.0 * s))))
        ctr.append(cl(torch.randn(B, 1, H, W, generator=g)))
    return cls, reg, ctr, torch.tensor([SHAPE] * B, dtype=torch.int32).cuda()


def targets(B, seed=0):
    g = np.random.default_rng(seed)
    wh = g.uniform(30, 400, (B, G, 2))
    xy = g.uniform(0, 1, (B, G, 2)) * (np.asarray([SHAPE[1], SHAPE[0]]) - wh)
    gt = np.concatenate([xy, xy + wh], -1).astype(np.float32)
    return (torch.from_numpy(gt).cuda(), torch.from_numpy(g.integers(1, C + 1, (B, G))).cuda(),
            torch.full((B,), G, dtype=torch.int32).cuda())


# ---- the eager torch compositions ------------------------------------------------------------------------------------------
def eager_target(points, gt, gl, ranges):
    x, y, lev = points[:, 0], points[:, 1], points[:, 3].long()
    lo, hi = ranges[lev, 0][:, None], ranges[lev, 1][:, None]
    out = []
    for b in range(gt.shape[0]):
        d = torch.stack([x[:, None] - gt[b, :, 0], y[:, None] - gt[b, :, 1], gt[b, :, 2] - x[:, None],
                         gt[b, :, 3] - y[:, None]], -1)
        ok = (d.min(-1)[0] > 0) & (d.max(-1)[0] >= lo) & (d.max(-1)[0] <= hi)
        area = ((gt[b, :, 2] - gt[b, :, 0] + 1) * (gt[b, :, 3] - gt[b, :, 1] + 1))[None].expand_as(ok)
        best, j = torch.where(ok, area, torch.full_like(area, float("inf"))).min(1)
        hit = torch.isfinite(best)
        out.append((torch.where(hit, gl[b][j], torch.zeros_like(j)),
                    torch.where(hit[:, None], d[torch.arange(d.shape[0]), j], torch.zeros_like(d[:, 0]))))
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def eager_loss(cls, reg, ctr, labels, bt, gamma=2.0, alpha=0.25, eps=1e-6):
    B = labels.shape[0]
    flat = lambda ts: torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1, t.shape[1]) for t in ts], 1).float()  # noqa: E731
    x, r, z = flat(cls), flat(reg), flat(ctr)[..., 0]
    pos = labels > 0
    npos = int(pos.sum().item())
    onehot = labels[..., None] == torch.arange(1, C + 1, device=labels.device)
    p = x.sigmoid()
    ls, lns = torch.nn.functional.logsigmoid(x), torch.nn.functional.logsigmoid(-x)
    loss_cls = torch.where(onehot, -alpha * (1 - p) ** gamma * ls, -(1 - alpha) * p ** gamma * lns).sum() / (npos + B)
    d, t = r[pos].exp(), bt[pos]
    c = (torch.minimum(t[:, 0], t[:, 2]) / torch.maximum(t[:, 0], t[:, 2]) *
         torch.minimum(t[:, 1], t[:, 3]) / torch.maximum(t[:, 1], t[:, 3])).sqrt()
    area = lambda q: (q[:, 0] + q[:, 2] + 1) * (q[:, 1] + q[:, 3] + 1)   # noqa: E731
    inter = area(torch.minimum(d, t))
    iou = inter / (area(d) + area(t) - inter)
    loss_box = (c * -iou.clamp(min=eps).log()).sum() / c.sum()
    loss_ctr = torch.nn.functional.binary_cross_entropy_with_logits(z[pos], c, reduction="sum") / max(npos, 1)
    return torch.stack([loss_cls, loss_box, loss_ctr])


def eager_detections(cls, reg, ctr, points, shapes_host, nms_pre, score_thr, nms_thr, max_per_img):
    out = []
    for b, (ih, iw) in enumerate(shapes_host):
        boxes, scores = [], []
        for c, r, z, pt in zip(cls, reg, ctr, points):
            s = c[b].permute(1, 2, 0).reshape(-1, C).float().sigmoid() * z[b].reshape(-1, 1).float().sigmoid()
            d = r[b].permute(1, 2, 0).reshape(-1, 4).float().exp()
            if 0 < nms_pre < s.shape[0]:
                top = s.max(1)[0].topk(nms_pre)[1]
                s, d, pt = s[top], d[top], pt[top]
            boxes.append(torch.stack([(pt[:, 0] - d[:, 0]).clamp(0, iw - 1), (pt[:, 1] - d[:, 1]).clamp(0, ih - 1),
                                      (pt[:, 0] + d[:, 2]).clamp(0, iw - 1), (pt[:, 1] + d[:, 3]).clamp(0, ih - 1)], 1))
            scores.append(s)
        boxes, scores = torch.cat(boxes), torch.cat(scores)
        dets, labels = [], []
        for k in range(C):
            ok = scores[:, k] > score_thr
            if not bool(ok.any()):
                continue
            bx, s = boxes[ok].contiguous(), scores[ok, k].contiguous()
            _, keep = T.nms((bx, s), nms_thr)
            dets.append(torch.cat([bx[keep], s[keep, None]], 1))
            labels.append(torch.full((keep.numel(),), k, dtype=torch.int64, device=bx.device))
        if not dets:
            out.append((torch.zeros(0, 5, device=boxes.device), torch.zeros(0, dtype=torch.int64, device=boxes.device)))
            continue
        dets, labels = torch.cat(dets), torch.cat(labels)
        order = dets[:, 4].sort(descending=True, stable=True)[1][:max_per_img]
        out.append((dets[order], labels[order]))
    return out


def time_events(fn, iters, repeats):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    got = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) / iters * 1e3)
    return [round(statistics.median(got), 1), round(min(got), 1), round(max(got), 1)]


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcos_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for B in (1, 2):
        cls, reg, ctr, shapes = inputs(B)
        gt, gl, gc = targets(B)
        labels, bt, _, num_pos = T.fcos_target(SIZES, STRIDES, RANGES, gt, gl, gc)
        gvec = torch.ones(3, device="cuda")

        def loss_step():
            leaves = [t.detach().requires_grad_() for t in cls + reg + ctr]
            L = len(LEVELS)
            losses = T.fcos_loss(leaves[:L], leaves[L:2 * L], leaves[2 * L:], labels, bt)
            losses.backward(gvec)
            return losses.detach(), leaves[0].grad

        tgt = lambda: T.fcos_target(SIZES, STRIDES, RANGES, gt, gl, gc)                      # noqa: E731
        det = lambda: T.fcos_detections(cls, reg, ctr, STRIDES, shapes, **CFG)               # noqa: E731
        if args.trace:
            for _ in range(10):
                tgt()
                loss_step()
                det()
            torch.cuda.synchronize()
            continue
        points = T.fcos_points(SIZES, STRIDES)
        per_level = list(points.split([h * w for h, w in SIZES]))
        ranges_t = torch.tensor(RANGES, device="cuda")

        def eager_loss_step():
            leaves = [t.detach().requires_grad_() for t in cls + reg + ctr]
            L = len(LEVELS)
            losses = eager_loss(leaves[:L], leaves[L:2 * L], leaves[2 * L:], labels, bt)
            losses.backward(gvec)
            return losses.detach()

        g_t, _ = graphed(tgt)
        g_l, lout = graphed(loss_step)
        g_d, dout = graphed(det)
        sh = shapes.cpu().tolist()
        few = max(3, args.iters // 20)
        line = {
            "B": B, "points_per_image": int(points.shape[0]), "C": C, "dtype": "bf16", "layout": "channels_last",
            "gt_per_image": G, "num_pos": num_pos.cpu().tolist(), **CFG,
            "launches_detections": T.fcos_detections_plan(SIZES, B, C, CFG["nms_pre"])["launches"],
            "fcos_target_graph_replay_us": time_events(g_t.replay, args.iters, args.repeats),
            "fcos_loss_fwd_bwd_graph_replay_us": time_events(g_l.replay, args.iters, args.repeats),
            "fcos_detections_graph_replay_us": time_events(g_d.replay, args.iters, args.repeats),
            "eager_torch_target_us": time_events(lambda: eager_target(points, gt, gl, ranges_t), few, args.repeats),
            "eager_torch_loss_fwd_bwd_us": time_events(eager_loss_step, few, args.repeats),
            "eager_torch_detections_us": time_events(
                lambda: eager_detections(cls, reg, ctr, per_level, sh, **CFG), few, args.repeats),
            "losses": [round(v, 6) for v in lout[0].cpu().tolist()],
            "losses_eager_torch": [round(v, 6) for v in eager_loss_step().cpu().tolist()],
            "counts": dout[3].cpu().tolist(), "iters": args.iters, "repeats": args.repeats,
            "us_fields": "median, min, max of the windows"}
        lines.append(line)
        print(json.dumps(line))
    if args.trace:
        print(json.dumps({"trace": "10 calls of each function at B=1, 2"}))
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
