#!/usr/bin/env python
"""Training targets at the C4 pyramid (800x1344, A=3, five levels, 268,569 anchors per image), B=2: time per call of
``anchor_target`` (G = 8 and 100 ground truths per image) and of ``sample_rois`` (2 x 2000 proposals) replayed from a
captured graph, beside the eager composition a user would write without them (``bbox_overlaps`` per image, torch
reductions, ``randperm``, ``bbox2delta``).  Device events after warm-up.  Prints one JSON object per configuration.

``--trace``: only issue eager calls (10 of each configuration) for a ``rocprofv3 --kernel-trace --stats`` run that
counts launches per call and gives the per-kernel split."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_detection_amd as T  # noqa: E402
import target_cases as C  # noqa: E402
from proposal_bench import inputs, time_events  # noqa: E402

SHAPES = [(800, 1344), (704, 1216)]


def anchor_inputs(G):
    case = C.anchor_case(gt_counts=(G, G), shapes=SHAPES, seed=3)
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.items()}


def eager_anchor_target(anchors, valid_flags, gt_bboxes, gt_counts_host, shapes_host, num=256, pos_fraction=0.5):
    """The composition of today's ops: the (N, G) IoU matrix through HBM, nonzero / randperm with their host
    synchronisations, bbox2delta on the gathered rows."""
    out = []
    n = anchors.shape[0]
    for b, (h, w) in enumerate(shapes_host):
        gt = gt_bboxes[b, :gt_counts_host[b]].contiguous()
        inside = (valid_flags[b] != 0) & (anchors[:, 0] >= 0) & (anchors[:, 1] >= 0) & (anchors[:, 2] < w) & \
            (anchors[:, 3] < h)
        iou = T.bbox_overlaps(anchors, gt)
        iou = torch.where(inside[:, None], iou, torch.full_like(iou, -1.0))
        mx, am = iou.max(dim=1)
        assigned = torch.full((n,), -1, dtype=torch.int64, device=anchors.device)
        assigned[(mx >= 0) & (mx < 0.3)] = 0
        assigned[mx >= 0.7] = am[mx >= 0.7] + 1
        gmax = iou.max(dim=0)[0]
        hit = (iou == gmax[None, :]) & (gmax[None, :] >= 0.3)
        jj = torch.arange(1, gt.shape[0] + 1, device=anchors.device)[None, :]
        low = (hit * jj).max(dim=1)[0]
        assigned = torch.where(low > 0, low, assigned)
        pos, neg = torch.nonzero(assigned > 0).flatten(), torch.nonzero(assigned == 0).flatten()
        n_pos = min(pos.numel(), int(num * pos_fraction))
        pos = pos[torch.randperm(pos.numel(), device=pos.device)[:n_pos]]
        neg = neg[torch.randperm(neg.numel(), device=neg.device)[:num - n_pos]]
        labels = torch.zeros(n, dtype=torch.int64, device=anchors.device)
        weights = torch.zeros(n, device=anchors.device)
        targets = torch.zeros(n, 4, device=anchors.device)
        bw = torch.zeros(n, 4, device=anchors.device)
        labels[pos], weights[pos], weights[neg], bw[pos] = 1, 1.0, 1.0, 1.0
        if n_pos:
            targets[pos] = T.bbox2delta(anchors[pos].contiguous(), gt[assigned[pos] - 1].contiguous())
        out.append((labels, weights, targets, bw))
    return out


def eager_sample_rois(props, counts_host, gt_bboxes, gt_labels, gt_counts_host, num=512, pos_fraction=0.25):
    out = []
    for b in range(props.shape[0]):
        gt = gt_bboxes[b, :gt_counts_host[b]].contiguous()
        cand = torch.cat([gt, props[b, :counts_host[b], :4]]).contiguous()
        iou = T.bbox_overlaps(cand, gt)
        mx, am = iou.max(dim=1)
        assigned = torch.where(mx >= 0.5, am + 1, torch.zeros_like(am))
        pos, neg = torch.nonzero(assigned > 0).flatten(), torch.nonzero(assigned == 0).flatten()
        n_pos = min(pos.numel(), int(num * pos_fraction))
        pos = pos[torch.randperm(pos.numel(), device=pos.device)[:n_pos]].sort()[0]
        neg = neg[torch.randperm(neg.numel(), device=neg.device)[:num - n_pos]].sort()[0]
        sel = torch.cat([pos, neg])
        rois = torch.cat([torch.full((sel.numel(), 1), float(b), device=cand.device), cand[sel]], 1)
        labels = torch.cat([gt_labels[b][assigned[pos] - 1], torch.zeros_like(neg)])
        tg = T.bbox2delta(cand[pos].contiguous(), gt[assigned[pos] - 1].contiguous(), (0, 0, 0, 0),
                          (0.1, 0.1, 0.2, 0.2))
        out.append((rois, labels, tg))
    return out


def roi_inputs(G):
    cls, reg, anchors, shapes = inputs(2)
    props, _, counts = T.rpn_proposals(cls, reg, anchors, shapes, nms_pre=2000, nms_post=2000, max_num=2000)
    g = np.random.default_rng(1)
    p = props.cpu().numpy()
    gt = np.floor(p[:, g.integers(0, 1500, G), :4]) + g.integers(-6, 7, (2, G, 4)).astype(np.float32)
    gt[..., 2:] = np.maximum(gt[..., 2:], gt[..., :2] + 4)
    return (props, counts, torch.from_numpy(gt).cuda(), torch.from_numpy(g.integers(1, 81, (2, G))).cuda(),
            torch.full((2,), G, dtype=torch.int32).cuda())


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    for G in (8, 100):
        d = anchor_inputs(G)
        call = lambda: T.anchor_target(**d)  # noqa: E731
        if args.trace:
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            continue
        g, out = graph_of(call)
        us_graph = time_events(g.replay, args.iters)
        us_call = time_events(call, args.iters)
        sh, gc = d["img_shapes"].cpu().tolist(), d["gt_counts"].cpu().tolist()
        us_base = time_events(lambda: eager_anchor_target(d["anchors"], d["valid_flags"], d["gt_bboxes"], gc, sh),
                              max(5, args.iters // 20))
        base = eager_anchor_target(d["anchors"], d["valid_flags"], d["gt_bboxes"], gc, sh)
        print(json.dumps({
            "op": "anchor_target", "B": 2, "G": G, "anchors_per_image": d["anchors"].shape[0], "num": 256,
            "graph_replay_us": round(us_graph, 1), "eager_call_us": round(us_call, 1),
            "eager_composition_us": round(us_base, 1), "speedup_vs_eager_composition": round(us_base / us_graph, 1),
            "iou_matrix_bytes_per_image": d["anchors"].shape[0] * G * 4,
            "num_pos": out[4].cpu().tolist(), "num_neg": out[5].cpu().tolist(),
            "positives_equal_in_number_to_composition": [int(b[0].sum()) for b in base] == out[4].cpu().tolist()}))
    for G in (8, 100):
        r = roi_inputs(G)
        call = lambda: T.sample_rois(*r)  # noqa: E731
        if args.trace:
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            continue
        g, out = graph_of(call)
        us_graph = time_events(g.replay, args.iters)
        us_call = time_events(call, args.iters)
        ch, gc = r[1].cpu().tolist(), r[4].cpu().tolist()
        us_base = time_events(lambda: eager_sample_rois(r[0], ch, r[2], r[3], gc), max(5, args.iters // 20))
        print(json.dumps({
            "op": "sample_rois", "B": 2, "G": G, "proposals_per_image": ch, "num": 512,
            "graph_replay_us": round(us_graph, 1), "eager_call_us": round(us_call, 1),
            "eager_composition_us": round(us_base, 1), "speedup_vs_eager_composition": round(us_base / us_graph, 1),
            "num_pos": out[6].cpu().tolist(), "num_neg": out[7].cpu().tolist()}))
    if args.trace:
        print(json.dumps({"trace": "10 eager calls each: anchor_target G=8, G=100, sample_rois G=8, G=100"}))


if __name__ == "__main__":
    main()
