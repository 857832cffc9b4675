#!/usr/bin/env python
"""Test-time detections of the RoI box head at R = 1000 RoIs per image, C = 81, B in {1, 2, 4}, score_thr 0.05,
max_per_img 100, bf16 head outputs: time per call of ``bbox_head_detections`` replayed from a captured graph, of the
eager call, and of the eager torch composition a user writes without it (softmax, ``delta2bbox``, a Python loop over
the 80 classes with a boolean index and one ``box.nms`` each, concat, sort, top-k — one ``.item()`` per ``box.nms``).
Logits come from a fixed seed: a quarter of the rows are confident of one foreground class, the rest lean to the
background.  Device events after warm-up; the median of ``--repeats`` measurements of ``--iters`` calls each.  Prints
one JSON object per batch size and appends it to profiles/detect_bench.jsonl.

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

R_PER_IMG, C = 1000, 81
CFG = dict(score_thr=0.05, nms_thr=0.5, max_per_img=100)
SHAPE = (800, 1344)


def inputs(B, seed=0):
    g = np.random.default_rng(seed)
    R = B * R_PER_IMG
    centres = g.uniform(100, 1200, (40, 2)) * [1.0, 0.55]
    k = g.integers(0, 40, R)
    xy = centres[k] + g.normal(0, 24, (R, 2))
    wh = g.uniform(40, 260, (R, 2))
    img = np.repeat(np.arange(B), R_PER_IMG)[:, None]
    rois = np.concatenate([img, xy - wh / 2, xy + wh / 2], 1).astype(np.float32)
    x = g.normal(0, 1.0, (R, C))
    x[:, 0] += 4.0                                            # most rows lean to the background
    sure = g.random(R) < 0.25                                 # confident rows: one foreground class of the cluster's few
    x[sure, 1 + (k[sure] * 7 + g.integers(0, 3, sure.sum())) % (C - 1)] += 9.0
    d = g.normal(0, 0.5, (R, 4 * C))
    shapes = torch.tensor([SHAPE] * B, dtype=torch.int32).cuda()
    return (torch.from_numpy(rois).cuda(), torch.from_numpy(x).bfloat16().cuda(),
            torch.from_numpy(d).bfloat16().cuda(), shapes)


def eager_baseline(rois, cls, reg, shapes_host, score_thr, nms_thr, max_per_img):
    out = []
    scores = cls.float().softmax(1)
    for b, shape in enumerate(shapes_host):
        m = rois[:, 0] == b
        boxes = T.delta2bbox(rois[m, 1:].contiguous(), reg[m].float().contiguous(), (0, 0, 0, 0), (0.1, 0.1, 0.2, 0.2),
                             shape)
        sc = scores[m]
        dets, labels = [], []
        for c in range(1, C):
            ok = sc[:, c] > score_thr
            if not bool(ok.any()):
                continue
            bx, s = boxes[ok, 4 * c:4 * c + 4].contiguous(), sc[ok, c].contiguous()
            _, keep = T.nms((bx, s), nms_thr)
            dets.append(torch.cat([bx[keep], s[keep, None]], 1))
            labels.append(torch.full((keep.numel(),), c - 1, dtype=torch.int64, device=bx.device))
        if not dets:
            out.append((torch.zeros(0, 5, device=rois.device), torch.zeros(0, dtype=torch.int64, device=rois.device)))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bench.jsonl"))
    args = ap.parse_args()
    if args.trace:
        for B in (1, 2, 4):
            a = inputs(B)
            for _ in range(10):
                T.bbox_head_detections(*a, **CFG)
            torch.cuda.synchronize()
        print(json.dumps({"trace": "10 calls each at B=1, 2, 4"}))
        return
    lines = []
    for B in (1, 2, 4):
        a = inputs(B)
        T.bbox_head_detections(*a, **CFG)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed = T.bbox_head_detections(*a, **CFG)
        us_graph = time_events(g.replay, args.iters, args.repeats)
        us_call = time_events(lambda: T.bbox_head_detections(*a, **CFG), args.iters, args.repeats)
        sh = a[3].cpu().tolist()
        us_base = time_events(lambda: eager_baseline(*a[:3], sh, **CFG), max(3, args.iters // 20), args.repeats)
        base = eager_baseline(*a[:3], sh, **CFG)
        counts = graphed[3].cpu().tolist()
        # the eager softmax is torch's, not the spec's: a score within an ulp of a threshold or of a tie may differ
        same = all(counts[b] == base[b][0].shape[0] and
                   torch.equal(graphed[1][b, :counts[b]], base[b][1]) for b in range(B))
        lines.append({
            "B": B, "rois_per_image": R_PER_IMG, "C": C, **CFG, "dtype": "bf16",
            "bbox_head_detections_graph_replay_us": round(us_graph[0], 1),
            "graph_replay_us_min_max": [round(us_graph[1], 1), round(us_graph[2], 1)],
            "bbox_head_detections_eager_call_us": round(us_call[0], 1),
            "eager_torch_baseline_us": round(us_base[0], 1),
            "eager_torch_baseline_us_min_max": [round(us_base[1], 1), round(us_base[2], 1)],
            "speedup_vs_eager_baseline": round(us_base[0] / us_graph[0], 1),
            "iters": args.iters, "repeats": args.repeats,
            "labels_equal_to_eager_baseline": bool(same), "counts": counts})
        print(json.dumps(lines[-1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
