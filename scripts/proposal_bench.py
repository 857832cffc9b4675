#!/usr/bin/env python
"""RPN proposals at the C4 pyramid (800x1344, A=3, five levels, 268,569 anchors per image), bf16 channels_last head
outputs: time per call of ``rpn_proposals`` replayed from a captured graph, of an eager torch composition of the same
pipeline (torch.topk per level, torch decode, ``box.nms`` per (image, level), torch.topk merge) and of the CPU oracle
(tests/proposal_ref.py).  Device events after warm-up.  Prints one JSON object per configuration.

``--trace``: only issue eager calls (10 at B=2, 10 at B=4) for a ``rocprofv3 --kernel-trace --stats`` run that counts
launches per call."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_detection_amd as T  # noqa: E402

LEVELS = [((200, 336), 4), ((100, 168), 8), ((50, 84), 16), ((25, 42), 32), ((13, 21), 64)]
CONFIGS = {"train": dict(nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7),
           "test": dict(nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7)}


def inputs(B, seed=0):
    gens = [T.AnchorGenerator(st, [8], [0.5, 1.0, 2.0]) for _, st in LEVELS]
    anchors, _ = T.anchor_pyramid(gens, [fs for fs, _ in LEVELS], [st for _, st in LEVELS], "cuda")
    g = torch.Generator().manual_seed(seed)
    cls, reg = [], []
    for (h, w), _ in LEVELS:
        cls.append((torch.randn(B, 3, h, w, generator=g) * 2).bfloat16().cuda()
                   .contiguous(memory_format=torch.channels_last))
        reg.append((torch.randn(B, 12, h, w, generator=g) * 0.5).bfloat16().cuda()
                   .contiguous(memory_format=torch.channels_last))
    shapes = torch.tensor([(800, 1344)] * B, dtype=torch.int32).cuda()
    return cls, reg, anchors, shapes


def eager_baseline(cls, reg, anchors, shapes_host, nms_pre, nms_post, max_num, nms_thr):
    """What a user writes today: torch ops + one box.nms (five launches and a .item() each) per (image, level)."""
    B = cls[0].shape[0]
    out = []
    clip = abs(float(np.log(16 / 1000)))
    for b in range(B):
        h, w = shapes_host[b]
        scores, boxes, aidx = [], [], []
        off = 0
        for c, d, a in zip(cls, reg, anchors):
            logit = c[b].permute(1, 2, 0).reshape(-1).float()
            delta = d[b].permute(1, 2, 0).reshape(-1, 4).float()
            k = min(nms_pre, logit.numel())
            s, idx = logit.topk(k)
            r, dl = a[idx], delta[idx]
            px, py = (r[:, 0] + r[:, 2]) * 0.5, (r[:, 1] + r[:, 3]) * 0.5
            pw, ph = r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1
            gw, gh = pw * dl[:, 2].clamp(-clip, clip).exp(), ph * dl[:, 3].clamp(-clip, clip).exp()
            gx, gy = px + pw * dl[:, 0], py + ph * dl[:, 1]
            bx = torch.stack([(gx - gw * 0.5 + 0.5).clamp(0, w - 1), (gy - gh * 0.5 + 0.5).clamp(0, h - 1),
                              (gx + gw * 0.5 - 0.5).clamp(0, w - 1), (gy + gh * 0.5 - 0.5).clamp(0, h - 1)], 1)
            _, keep = T.nms((bx.contiguous(), s.contiguous()), nms_thr)
            keep = keep[:nms_post]
            scores.append(s[keep])
            boxes.append(bx[keep])
            aidx.append(idx[keep] + off)
            off += logit.numel()
        s, bx, ai = torch.cat(scores), torch.cat(boxes), torch.cat(aidx)
        top, sel = s.topk(min(max_num, s.numel()))
        out.append((torch.cat([bx[sel], top.sigmoid()[:, None]], 1), ai[sel]))
    return out


def time_events(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if args.trace:
        for B in (2, 4):
            cls, reg, anchors, shapes = inputs(B)
            for _ in range(10):
                T.rpn_proposals(cls, reg, anchors, shapes, **CONFIGS["train"])
            torch.cuda.synchronize()
        print(json.dumps({"trace": "10 calls at B=2, then 10 at B=4, train config"}))
        return
    import proposal_ref as R
    for B, name in ((2, "train"), (1, "test")):
        cfg = CONFIGS[name]
        cls, reg, anchors, shapes = inputs(B)
        T.rpn_proposals(cls, reg, anchors, shapes, **cfg)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            graphed = T.rpn_proposals(cls, reg, anchors, shapes, **cfg)
        us_graph = time_events(g.replay, args.iters)
        us_eager_call = time_events(lambda: T.rpn_proposals(cls, reg, anchors, shapes, **cfg), args.iters)
        sh = shapes.cpu().tolist()
        us_base = time_events(lambda: eager_baseline(cls, reg, anchors, sh, **cfg), max(5, args.iters // 20))
        # same candidates as the baseline?  (the baseline ranks by torch.topk, whose tie order is unspecified)
        base = eager_baseline(cls, reg, anchors, sh, **cfg)
        same_idx = all(torch.equal(base[b][1], graphed[1][b, :base[b][1].numel()]) for b in range(B))
        c_np, r_np = [c.float().cpu().numpy() for c in cls], [d.float().cpu().numpy() for d in reg]
        a_np = [a.cpu().numpy() for a in anchors]
        t0 = time.perf_counter()
        pr, ar, cr = R.rpn_proposals(c_np, r_np, a_np, sh, **cfg)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        print(json.dumps({
            "config": name, "B": B, **cfg, "dtype": "bf16", "layout": "channels_last",
            "anchors_per_image": sum(a.shape[0] for a in anchors),
            "rpn_proposals_graph_replay_us": round(us_graph, 1),
            "rpn_proposals_eager_call_us": round(us_eager_call, 1),
            "eager_torch_baseline_us": round(us_base, 1),
            "speedup_vs_eager_baseline": round(us_base / us_graph, 1),
            "cpu_oracle_ms": round(cpu_ms, 1),
            "anchor_idx_equal_to_oracle": bool(np.array_equal(graphed[1].cpu().numpy(), ar)),
            "anchor_idx_equal_to_eager_baseline": bool(same_idx),
            "counts": graphed[2].cpu().tolist()}))


if __name__ == "__main__":
    main()
