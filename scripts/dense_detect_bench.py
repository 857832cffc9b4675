#!/usr/bin/env python
"""Test-time detections of a single-stage head at the RetinaNet shape (strides 8..128 at 800 x 1344: 201,600 anchors per
image, A = 9, C = 80, bf16 channels_last head outputs, nms_pre 1000, score_thr 0.05, max_per_img 100), B in {1, 2}: time
per call of ``anchor_head_detections`` replayed from a captured graph, of the eager call, and of the eager torch
composition a user writes without it (per image and level: sigmoid, class maximum, ``topk``, gather, ``delta2bbox``; then
a Python loop over the 80 classes with a boolean index and one ``box.nms`` each, concat, sort, top-k — one ``.item()`` per
``box.nms``).  ``anchor_target_all`` on the same pyramid with 20 ground truths per image is timed beside it (graph
replay only: it replaces nothing a user would compose differently from ``anchor_target``).  Logits come from a fixed
seed: a background prior of 0.01 with a few hundred confident anchors per image.  Device events after warm-up; the
median of ``--repeats`` measurements of ``--iters`` calls each.  Prints one JSON object per batch size and appends it to
profiles/dense_detect_bench.jsonl.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_detection_amd as T  # noqa: E402

A, C = 9, 80
SHAPE = (800, 1344)
LEVELS = [((100, 168), 8), ((50, 84), 16), ((25, 42), 32), ((13, 21), 64), ((7, 11), 128)]
CFG = dict(nms_pre=1000, score_thr=0.05, nms_thr=0.5, max_per_img=100, target_stds=(0.1, 0.1, 0.2, 0.2))
G = 20


def pyramid():
    gens = [T.AnchorGenerator(s, [4 * 2 ** (i / 3) for i in range(3)], [0.5, 1.0, 2.0]) for _, s in LEVELS]
    return T.anchor_pyramid(gens, [fs for fs, _ in LEVELS], [s for _, s in LEVELS], "cuda")[0]


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    cls, reg = [], []
    for (H, W), _ in LEVELS:
        x = torch.randn(B, A * C, H, W, generator=g) * 1.2 - 4.6            # sigmoid(-4.6) = 0.01
        hot = torch.rand(B, A * C, H, W, generator=g) < 2e-5                # confident anchors, mostly on P3 / P4
        x[hot] += 7.0
        cls.append(x.bfloat16().cuda().contiguous(memory_format=torch.channels_last))
        reg.append((torch.randn(B, 4 * A, H, W, generator=g) * 0.5).bfloat16().cuda()
                   .contiguous(memory_format=torch.channels_last))
    return cls, reg, torch.tensor([SHAPE] * B, dtype=torch.int32).cuda()


def targets(B, seed=0):
    g = np.random.default_rng(seed)
    wh = g.uniform(30, 400, (B, G, 2))
    xy = g.uniform(0, 1, (B, G, 2)) * (np.asarray([SHAPE[1], SHAPE[0]]) - wh)
    gt = np.concatenate([xy, xy + wh], -1).astype(np.float32)
    return (torch.from_numpy(gt).cuda(), torch.from_numpy(g.integers(1, C + 1, (B, G))).cuda(),
            torch.full((B,), G, dtype=torch.int32).cuda())


def eager_baseline(cls, reg, anchors, shapes_host, nms_pre, score_thr, nms_thr, max_per_img, target_stds):
    out = []
    for b, shape in enumerate(shapes_host):
        boxes, scores = [], []
        for c, d, a in zip(cls, reg, anchors):
            s = c[b].permute(1, 2, 0).reshape(-1, C).float().sigmoid()
            dl = d[b].permute(1, 2, 0).reshape(-1, 4).float()
            if 0 < nms_pre < s.shape[0]:
                top = s.max(1)[0].topk(nms_pre)[1]
                s, dl, a = s[top], dl[top], a[top]
            boxes.append(T.delta2bbox(a.contiguous(), dl.contiguous(), (0, 0, 0, 0), target_stds, shape))
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
    return statistics.median(got), min(got), max(got)


def graphed(fn):
    fn()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_detect_bench.jsonl"))
    args = ap.parse_args()
    anchors = pyramid()
    all_anchors = torch.cat(anchors)
    if args.trace:
        for B in (1, 2):
            cls, reg, shapes = inputs(B)
            gt, gl, gc = targets(B)
            for _ in range(10):
                T.anchor_head_detections(cls, reg, anchors, shapes, **CFG)
                T.anchor_target_all(all_anchors, None, gt, gl, gc, shapes)
            torch.cuda.synchronize()
        print(json.dumps({"trace": "10 calls of each function at B=1, 2"}))
        return
    lines = []
    for B in (1, 2):
        cls, reg, shapes = inputs(B)
        gt, gl, gc = targets(B)
        det = lambda: T.anchor_head_detections(cls, reg, anchors, shapes, **CFG)   # noqa: E731
        tgt = lambda: T.anchor_target_all(all_anchors, None, gt, gl, gc, shapes)   # noqa: E731
        g, out = graphed(det)
        us_graph = time_events(g.replay, args.iters, args.repeats)
        us_call = time_events(det, args.iters, args.repeats)
        gt_graph, tout = graphed(tgt)
        us_tgt = time_events(gt_graph.replay, args.iters, args.repeats)
        sh = shapes.cpu().tolist()
        us_base = time_events(lambda: eager_baseline(cls, reg, anchors, sh, **CFG), max(3, args.iters // 20),
                              args.repeats)
        base = eager_baseline(cls, reg, anchors, sh, **CFG)
        counts = out[3].cpu().tolist()
        # torch's sigmoid and topk are not the spec's: a score within an ulp of a threshold or of a tie may differ
        same = all(counts[b] == base[b][0].shape[0] and torch.equal(out[1][b, :counts[b]], base[b][1])
                   for b in range(B))
        plan = T.anchor_head_detections_plan([fs for fs, _ in LEVELS], B, A, C, CFG["nms_pre"])
        lines.append({
            "B": B, "anchors_per_image": plan["anchors"], "A": A, "C": C, "dtype": "bf16", "layout": "channels_last",
            **{k: v for k, v in CFG.items() if k != "target_stds"}, "dense_rows": plan["rows"],
            "launches": plan["launches"], "key_workgroups": plan["key_workgroups"],
            "anchor_head_detections_graph_replay_us": round(us_graph[0], 1),
            "graph_replay_us_min_max": [round(us_graph[1], 1), round(us_graph[2], 1)],
            "anchor_head_detections_eager_call_us": round(us_call[0], 1),
            "eager_torch_baseline_us": round(us_base[0], 1),
            "eager_torch_baseline_us_min_max": [round(us_base[1], 1), round(us_base[2], 1)],
            "speedup_vs_eager_baseline": round(us_base[0] / us_graph[0], 1),
            "anchor_target_all_graph_replay_us": round(us_tgt[0], 1),
            "anchor_target_all_us_min_max": [round(us_tgt[1], 1), round(us_tgt[2], 1)], "gt_per_image": G,
            "num_pos": tout[4].cpu().tolist(), "iters": args.iters, "repeats": args.repeats,
            "labels_equal_to_eager_baseline": bool(same), "counts": counts})
        print(json.dumps(lines[-1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
