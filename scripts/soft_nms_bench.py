#!/usr/bin/env python
"""``multiclass_nms`` with greedy NMS against the three soft-NMS methods: time per call replayed from a
captured graph at 1000 rows per image, C = 81, B in {1, 2}, score_thr 0.05, max_num 100, class-specific boxes clustered
as detections are (40 centres per image, a quarter of the rows confident of one of the cluster's few classes), plus one
worst case: a single segment of 4096 mutually overlapping boxes (C = 2, every row a candidate), once with the configs
above (most candidates fall under min_score within a few rounds) and once with min_score = 0, where no candidate is
ever dropped and all 4096 rounds of the soft loop run.  Device events after warm-up; the median of ``--repeats``
measurements of ``--iters`` replays each.  Prints one JSON object per shape, with every soft method's ratio to the
greedy path of the same run, and appends it to profiles/soft_nms_bench.jsonl."""
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

N_PER_IMG, C = 1000, 81
THR, MAX_NUM = 0.05, 100
SOFT = {"linear": dict(type="soft_nms", method="linear", iou_thr=0.5, min_score=0.001),
        "gaussian": dict(type="soft_nms", method="gaussian", sigma=0.5, min_score=0.001),
        "naive": dict(type="soft_nms", method="naive", iou_thr=0.5, min_score=0.001)}


def inputs(B, seed=0):
    g = np.random.default_rng(seed)
    N = B * N_PER_IMG
    centres = g.uniform(100, 1200, (40, 2)) * [1.0, 0.55]
    k = g.integers(0, 40, N)
    xy = centres[k][:, None, :] + g.normal(0, 24, (N, C - 1, 2))
    wh = g.uniform(40, 260, (N, C - 1, 2))
    boxes = np.concatenate([xy - wh / 2, xy + wh / 2], -1).reshape(N, 4 * (C - 1)).astype(np.float32)
    x = g.normal(0, 1.0, (N, C))
    x[:, 0] += 4.0
    sure = g.random(N) < 0.25
    x[sure, 1 + (k[sure] * 7 + g.integers(0, 3, sure.sum())) % (C - 1)] += 9.0
    scores = torch.from_numpy(x).softmax(1).float()
    idx = torch.from_numpy(np.repeat(np.arange(B), N_PER_IMG).astype(np.int32))
    return torch.from_numpy(boxes).cuda(), scores.cuda(), idx.cuda(), B


def worst_case(seed=1):
    """4096 candidates of one class, every pair overlapping: 4096 rounds of the soft loop, all 1024 threads busy."""
    g = np.random.default_rng(seed)
    n = 4096
    xy = g.uniform(0, 20, (n, 2))
    boxes = np.concatenate([xy, xy + g.uniform(100, 140, (n, 2))], 1).astype(np.float32)
    scores = np.zeros((n, 2), np.float32)
    scores[:, 1] = g.uniform(0.1, 1.0, n)
    return torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), None, 1


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


def measure(args4, iters, repeats, soft=SOFT):
    out = {}
    for name, nms in [("hard", None)] + sorted(soft.items()):
        call = lambda: T.multiclass_nms(*args4, score_thr=THR, max_num=MAX_NUM, nms=nms)  # noqa: E731
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            res = call()
        us = time_events(g.replay, iters, repeats)
        out[name] = {"graph_replay_us": round(us[0], 1), "us_min_max": [round(us[1], 1), round(us[2], 1)],
                     "counts": res[3].cpu().tolist()}
    for name in soft:
        out[name]["ratio_to_hard"] = round(out[name]["graph_replay_us"] / out["hard"]["graph_replay_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_nms_bench.jsonl"))
    args = ap.parse_args()
    lines = []
    for B in (1, 2):
        lines.append({"case": "rows_1000_c81", "B": B, "rows_per_image": N_PER_IMG, "C": C, "score_thr": THR,
                      "max_num": MAX_NUM, "iters": args.iters, "repeats": args.repeats,
                      **measure(inputs(B), args.iters, args.repeats)})
        print(json.dumps(lines[-1]), flush=True)
    it = max(3, args.iters // 10)
    lines.append({"case": "one_segment_4096_overlapping", "B": 1, "rows_per_image": 4096, "C": 2, "score_thr": THR,
                  "max_num": MAX_NUM, "iters": it, "repeats": args.repeats, **measure(worst_case(), it, args.repeats)})
    print(json.dumps(lines[-1]), flush=True)
    every_round = {m: dict(cfg, min_score=0.0) for m, cfg in SOFT.items()}
    lines.append({"case": "one_segment_4096_overlapping_min_score_0", "B": 1, "rows_per_image": 4096, "C": 2,
                  "score_thr": THR, "max_num": MAX_NUM, "iters": it, "repeats": args.repeats,
                  **measure(worst_case(), it, args.repeats, every_round)})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
