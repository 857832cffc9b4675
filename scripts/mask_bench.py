#!/usr/bin/env python
"""The mask branch at the C4 shapes.  Training: B = 2, 2 x 128 mask RoIs (96 positives per image), M = 28, C = 81,
bf16 channels_last logits: ``mask_target`` and ``mask_head_loss`` forward + backward, replayed from a captured graph
and called eagerly, beside the composition a user writes without them (polygons rasterised on the host by
tests/mask_ref.py, a boolean-indexed ``binary_cross_entropy_with_logits`` with its host synchronisation, autograd).
Test: B = 1, 100 detections on an 800 x 1344 canvas: ``rois_from_detections`` + ``mask_head_masks`` (unpacked and
packed), beside a Python loop of one bilinear resize, threshold and paste per detection.  Inputs come from fixed seeds.
Device events after warm-up; the median of ``--repeats`` measurements of ``--iters`` calls each.  Prints one JSON object
per shape and appends it to profiles/mask_bench.jsonl.

``--trace``: only issue eager calls (10 per shape) for a ``rocprofv3 --kernel-trace --stats`` run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_detection_amd as T  # noqa: E402
import mask_ref as R  # noqa: E402

M, C = 28, 81
CANVAS = (800, 1344)


def star(cx, cy, rx, ry, n, g):
    ang = np.sort(g.uniform(0, 2 * np.pi, n))
    rad = g.uniform(0.6, 1.0, n)
    return np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang)], 1).astype(np.float32)


def train_inputs(B=2, per_img=128, pos=96, G=8, seed=0):
    g = np.random.default_rng(seed)
    polys, rois, inds, labels = [], [], [], []
    for b in range(B):
        wh = g.uniform(40, 400, (G, 2))
        c = g.uniform(0.2, 0.8, (G, 2)) * [CANVAS[1], CANVAS[0]]
        polys.append([[[float(v) for v in star(c[j, 0], c[j, 1], wh[j, 0] / 2, wh[j, 1] / 2, 30, g).reshape(-1)]
                       for _ in range(1 + j % 2)] for j in range(G)])
        k = g.integers(0, G, per_img)
        box = np.concatenate([c[k] - wh[k] / 2, c[k] + wh[k] / 2], 1) + g.normal(0, 6, (per_img, 4))
        rois.append(np.concatenate([np.full((per_img, 1), b), box], 1))
        inds.append(np.where(np.arange(per_img) < pos, k, -1))
        labels.append(g.integers(1, C, per_img))
    rois = torch.from_numpy(np.concatenate(rois).astype(np.float32)).cuda()
    inds = torch.from_numpy(np.concatenate(inds).astype(np.int32)).cuda()
    labels = torch.from_numpy(np.concatenate(labels).astype(np.int64)).cuda()
    packed = T.pack_polygons(polys, G)
    pred = torch.randn(B * per_img, C, M, M, generator=torch.Generator().manual_seed(seed)).mul(2).to(
        torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    return rois, inds, labels, packed, pred


def train_step(rois, inds, labels, polys_gpu, pred):
    targets, weights = T.mask_target(rois, inds, *polys_gpu, mask_size=M)
    loss = T.mask_head_loss(pred, targets, labels, weights)
    return loss, torch.autograd.grad(loss, [pred])[0]


def train_baseline(rois, inds, labels, polys_cpu, pred):
    """What a user writes without the kernels: the rasteriser on the host, then eager torch."""
    t, w = R.mask_target(rois.cpu().numpy(), inds.cpu().numpy(), *polys_cpu, M)
    t, w = torch.from_numpy(t).cuda(), torch.from_numpy(w).cuda()
    idx = (w > 0).nonzero()[:, 0]                                 # a host synchronisation
    loss = F.binary_cross_entropy_with_logits(pred[idx, labels[idx]].float(), t[idx].float())
    return loss, torch.autograd.grad(loss, [pred])[0]


def test_inputs(B=1, n=100, seed=0):
    g = np.random.default_rng(seed)
    wh = np.exp(g.uniform(np.log(24), np.log(500), (B, n, 2)))
    c = g.uniform(0.1, 0.9, (B, n, 2)) * [CANVAS[1], CANVAS[0]]
    dets = np.concatenate([c - wh / 2, c + wh / 2, g.random((B, n, 1))], 2).astype(np.float32)
    labels = torch.from_numpy(g.integers(0, C - 1, (B, n))).cuda()
    counts = torch.full((B,), n, dtype=torch.int32).cuda()
    pred = torch.randn(B * n, C, M, M, generator=torch.Generator().manual_seed(seed)).mul(2).to(
        torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    return torch.from_numpy(dets).cuda(), labels, counts, pred


def test_step(dets, labels, counts, pred, packed):
    rois = T.rois_from_detections(dets, counts)
    return rois, T.mask_head_masks(pred, dets, labels, counts, CANVAS, packed=packed)


def test_baseline(dets, labels, counts, pred):
    """mmdetection's get_seg_masks with torch on the device: one resize, threshold and paste per detection."""
    H, W = CANVAS
    out = torch.zeros(dets.shape[0] * dets.shape[1], H, W, dtype=torch.uint8, device=dets.device)
    boxes = dets.cpu().numpy()                                    # a host synchronisation
    cnt, lab = counts.cpu().tolist(), labels.cpu().numpy()
    for b in range(dets.shape[0]):
        for d in range(cnt[b]):
            x1, y1, x2, y2 = (int(v) for v in boxes[b, d, :4])
            w, h = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
            n = b * dets.shape[1] + d
            p = pred[n, lab[b, d] + 1].float().sigmoid()[None, None]
            m = F.interpolate(p, size=(h, w), mode="bilinear", align_corners=False)[0, 0] > 0.5
            xa, ya, xb, yb = max(x1, 0), max(y1, 0), min(x1 + w, W), min(y1 + h, H)
            if xa < xb and ya < yb:
                out[n, ya:yb, xa:xb] = m[ya - y1:yb - y1, xa - x1:xb - x1]
    return out


def time_events(fn, iters, repeats):
    for _ in range(3):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_bench.jsonl"))
    args = ap.parse_args()
    rois, inds, labels, packed_polys, pred = train_inputs()
    polys_gpu = [t.cuda() for t in packed_polys]
    polys_cpu = [t.numpy() for t in packed_polys]
    dets, dlabels, counts, dpred = test_inputs()
    if args.trace:
        for _ in range(10):
            train_step(rois, inds, labels, polys_gpu, pred)
            test_step(dets, dlabels, counts, dpred, False)
            test_step(dets, dlabels, counts, dpred, True)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "10 calls each of the training step and of both test steps"}))
        return
    lines = []
    g, out = graphed(lambda: train_step(rois, inds, labels, polys_gpu, pred))
    us_graph = time_events(g.replay, args.iters, args.repeats)
    us_call = time_events(lambda: train_step(rois, inds, labels, polys_gpu, pred), args.iters, args.repeats)
    us_base = time_events(lambda: train_baseline(rois, inds, labels, polys_cpu, pred), max(2, args.iters // 50),
                          args.repeats)
    base = train_baseline(rois, inds, labels, polys_cpu, pred)
    lines.append({
        "shape": "train", "B": 2, "rois": int(rois.shape[0]), "positives": int((inds >= 0).sum()), "M": M, "C": C,
        "dtype": "bf16 channels_last", "vertices": int(polys_cpu[0].shape[0]),
        "mask_target_loss_fwd_bwd_graph_replay_us": us_graph, "eager_call_us": us_call,
        "host_raster_eager_torch_baseline_us": us_base, "speedup_vs_baseline": round(us_base[0] / us_graph[0], 1),
        "loss": float(out[0].item()), "baseline_loss": float(base[0].item()),
        "iters": args.iters, "repeats": args.repeats})
    print(json.dumps(lines[-1]))
    ref = test_baseline(dets, dlabels, counts, dpred)
    us_base = time_events(lambda: test_baseline(dets, dlabels, counts, dpred), max(2, args.iters // 50), args.repeats)
    for packed in (False, True):
        g, out = graphed(lambda: test_step(dets, dlabels, counts, dpred, packed))
        us_graph = time_events(g.replay, args.iters, args.repeats)
        us_call = time_events(lambda: test_step(dets, dlabels, counts, dpred, packed), args.iters, args.repeats)
        line = {
            "shape": "test", "B": 1, "detections": int(dets.shape[1]), "canvas": list(CANVAS), "M": M, "C": C,
            "dtype": "bf16 channels_last", "packed": packed, "output_bytes": int(out[1].numel()),
            "rois_from_detections_mask_head_masks_graph_replay_us": us_graph, "eager_call_us": us_call,
            "eager_torch_loop_baseline_us": us_base, "speedup_vs_baseline": round(us_base[0] / us_graph[0], 1),
            "iters": args.iters, "repeats": args.repeats}
        if not packed:      # torch's resize is not the spec's arithmetic: pixels on a mask's rim may differ
            line["pixels_differing_from_baseline"] = int((out[1] != ref).sum())
            line["pixels_set"] = int(out[1].sum())
        lines.append(line)
        print(json.dumps(line))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
