#!/usr/bin/env python
"""Multi-level RoIAlign at the C4 pyramid (800x1344: P2..P5 = 200x336 .. 25x42, C = 256, bf16 channels_last):
time per call of ``roi_align`` (forward, and forward + backward) replayed from a captured graph, and of an eager
torch composition of the same spec (per-level gather of the four corners; its autograd backward is
``index_put_(accumulate=True)``).  Device events after warm-up.  Prints one JSON object per configuration and
writes them to profiles/roi_align_bench.jsonl (``--out``).

Configurations: train (B=2, 512 RoIs per image, 7x7, forward + backward), test (B=1, 1000 RoIs, 7x7, forward only),
mask (B=2, 128 RoIs per image, 14x14, forward + backward).  RoIs are drawn from a seed with a log-uniform scale mix
that puts rows on every level.

``--trace``: only issue eager calls (10 per configuration) for a ``rocprofv3 --kernel-trace --stats`` run
(summarised in profiles/roi_align_kernel_stats.csv)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_detection_amd as T  # noqa: E402

LEVELS = [((200, 336), 4), ((100, 168), 8), ((50, 84), 16), ((25, 42), 32)]
STRIDES = tuple(s for _, s in LEVELS)
CONFIGS = [("train", 2, 512, 7, True), ("test", 1, 1000, 7, False), ("mask", 2, 128, 14, True)]
C = 256


def inputs(B, per_img, seed=0):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, C, h, w, generator=g).bfloat16().cuda().contiguous(memory_format=torch.channels_last)
             for (h, w), _ in LEVELS]
    r = np.random.default_rng(seed)
    n = B * per_img
    side = np.exp(r.uniform(np.log(16), np.log(800), (n, 1))) * np.exp(r.uniform(-0.5, 0.5, (n, 2)))
    x1 = r.uniform(0, 1344 - side[:, 0].clip(max=1300))
    y1 = r.uniform(0, 800 - side[:, 1].clip(max=780))
    b = np.repeat(np.arange(B), per_img)
    rois = np.stack([b, x1, y1, x1 + side[:, 0], y1 + side[:, 1]], 1).astype(np.float32)
    return feats, torch.from_numpy(rois).cuda()


def eager_roi_align(feats, rois, S, sr=2, finest=56.0):
    """The spec in torch ops (sampling_ratio > 0): level map, then per level the samples' corners gathered from the
    NHWC features, weighted, summed and averaged.  One .nonzero() synchronisation per level."""
    R = rois.shape[0]
    x1, y1, x2, y2 = rois[:, 1], rois[:, 2], rois[:, 3], rois[:, 4]
    scale = torch.sqrt((x2 - x1 + 1) * (y2 - y1 + 1))
    lvl = torch.floor(torch.log2(scale / finest + 1e-6)).clamp(0, len(feats) - 1).long()
    out = feats[0].new_zeros(R, S, S, feats[0].shape[1])
    grid = (torch.arange(S, device=rois.device).float()[:, None] +
            (torch.arange(sr, device=rois.device).float()[None, :] + 0.5) / sr).reshape(-1)     # (S*sr,)
    for l, f in enumerate(feats):
        idx = (lvl == l).nonzero().squeeze(1)
        if idx.numel() == 0:
            continue
        x = f.permute(0, 2, 3, 1)                                        # NHWC view
        H, W = x.shape[1], x.shape[2]
        rr = rois[idx]
        sc = 1.0 / STRIDES[l]
        sw, sh = rr[:, 1] * sc, rr[:, 2] * sc
        bw = ((rr[:, 3] + 1) * sc - sw).clamp(min=0) / S
        bh = ((rr[:, 4] + 1) * sc - sh).clamp(min=0) / S

        def axis(s0, b, n):
            v = s0[:, None] + grid[None, :] * b[:, None]
            ok = (v >= -1) & (v <= n)
            v = v.clamp(min=0)
            lo = v.long().clamp(max=n - 1)
            hi = (lo + 1).clamp(max=n - 1)
            v = torch.where(lo >= n - 1, lo.float(), v)
            lw = v - lo
            return ok, lo, hi, lw, 1 - lw
        oky, yl, yh, ly, hy = axis(sh, bh, H)
        okx, xl, xh, lx, hx = axis(sw, bw, W)
        bi = rr[:, 0].long()[:, None, None]
        m = (oky[:, :, None] & okx[:, None, :]).float()

        def g(yy, xx):
            return x[bi, yy[:, :, None], xx[:, None, :]].float()         # (n, S*sr, S*sr, C)
        val = ((hy[:, :, None] * hx[:, None, :] * m)[..., None] * g(yl, xl) +
               (hy[:, :, None] * lx[:, None, :] * m)[..., None] * g(yl, xh) +
               (ly[:, :, None] * hx[:, None, :] * m)[..., None] * g(yh, xl) +
               (ly[:, :, None] * lx[:, None, :] * m)[..., None] * g(yh, xh))
        n = idx.numel()
        val = val.reshape(n, S, sr, S, sr, -1).mean((2, 4))
        out = out.index_put((idx,), val.to(out.dtype))
    return out.permute(0, 3, 1, 2)


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


def graphed(fn):
    """Capture fn on the stream it warmed up on (as GraphedStep does); fn must not leave an autograd graph alive."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_align_bench.jsonl"))
    args = ap.parse_args()
    if args.trace:
        for name, B, per_img, S, bwd in CONFIGS:
            feats, rois = inputs(B, per_img)
            leaves = [f.detach().requires_grad_(bwd) for f in feats]
            for _ in range(10):
                out = T.roi_align(leaves, rois, S, STRIDES, 2)
                if bwd:
                    torch.autograd.grad(out, leaves, torch.ones_like(out))
            torch.cuda.synchronize()
        print(json.dumps({"trace": "10 eager calls per configuration: " + ", ".join(c[0] for c in CONFIGS)}))
        return
    lines = []
    for name, B, per_img, S, bwd in CONFIGS:
        feats, rois = inputs(B, per_img)
        R = rois.shape[0]
        levels = torch.bincount(T.map_roi_levels(rois, 4), minlength=4).tolist()
        dout = torch.randn(R, C, S, S, generator=torch.Generator().manual_seed(1)).bfloat16().cuda()
        leaves = [f.detach().requires_grad_(True) for f in feats]

        def fwd():
            return T.roi_align(feats, rois, S, STRIDES, 2)

        def fwd_bwd():
            out = T.roi_align(leaves, rois, S, STRIDES, 2)
            return torch.autograd.grad(out, leaves, dout)

        def eager_fwd():
            return eager_roi_align(feats, rois, S)

        def eager_fwd_bwd():
            out = eager_roi_align(leaves, rois, S)
            return torch.autograd.grad(out, leaves, dout)

        rec = {"config": name, "B": B, "rois": R, "out_size": S, "sampling_ratio": 2, "C": C, "dtype": "bf16",
               "layout": "channels_last", "rois_per_level": levels}
        rec["fwd_graph_replay_us"] = round(time_events(graphed(fwd).replay, args.iters), 1)
        rec["fwd_eager_call_us"] = round(time_events(fwd, args.iters), 1)
        rec["eager_torch_fwd_us"] = round(time_events(eager_fwd, max(5, args.iters // 10)), 1)
        rec["speedup_fwd_vs_eager_torch"] = round(rec["eager_torch_fwd_us"] / rec["fwd_graph_replay_us"], 1)
        ours, base = fwd().float(), eager_fwd().float()
        rec["max_abs_diff_vs_eager_torch_fwd"] = float((ours - base).abs().max())
        if bwd:
            rec["fwd_bwd_graph_replay_us"] = round(time_events(graphed(fwd_bwd).replay, args.iters), 1)
            rec["bwd_only_us_est"] = round(rec["fwd_bwd_graph_replay_us"] - rec["fwd_graph_replay_us"], 1)
            rec["eager_torch_fwd_bwd_us"] = round(time_events(eager_fwd_bwd, max(5, args.iters // 10)), 1)
            rec["speedup_fwd_bwd_vs_eager_torch"] = round(rec["eager_torch_fwd_bwd_us"] /
                                                          rec["fwd_bwd_graph_replay_us"], 1)
        torch.cuda.synchronize()
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
