#!/usr/bin/env python
"""Forward + backward of the fused losses replayed from a captured graph, beside the eager torch composition a user
would write without them (permute / reshape of every level, ``F.binary_cross_entropy_with_logits`` or a sigmoid focal
loss, ``F.smooth_l1_loss``, ``F.cross_entropy`` on expanded targets, autograd), on the same GPU.  Three shapes:

  rpn        C4 pyramid (800x1344, five levels), B = 2, A = 3, C = 1, bf16 channels_last
  retinanet  strides 8..128 at 800x1344, B = 2, A = 9, C = 80, focal, bf16 channels_last
  roi_head   R = 1024, C = 81, class-specific boxes, fp32

Device events after warm-up.  Prints one JSON object per shape with the bytes the call has to move when every tensor
is touched once per pass (head outputs read forward and backward, gradients written, targets read twice; the RoI
head's box columns are only written) and what that is in
GB/s at the measured time."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch_detection_amd as T  # noqa: E402
from proposal_bench import time_events  # noqa: E402

C4 = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
RETINA = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def dense_inputs(levels, B, A, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = sum(h * w for h, w in levels) * A
    mk = lambda ch, h, w, s: (torch.randn(B, ch, h, w, generator=g) * s).to(torch.bfloat16).cuda().contiguous(  # noqa: E731
        memory_format=torch.channels_last).requires_grad_(True)
    cls = [mk(A * C, h, w, 2.0) for h, w in levels]
    reg = [mk(4 * A, h, w, 0.5) for h, w in levels]
    r = np.random.default_rng(seed)
    labels = np.where(r.random((B, N)) < 0.002, r.integers(1, C + 1, (B, N)), 0).astype(np.int64)
    lw = (r.random((B, N)) < (1.0 if C > 1 else 0.002)).astype(np.float32)      # RPN: 256-ish sampled; dense: all
    lw[labels > 0] = 1
    bt = r.normal(0, 0.5, (B, N, 4)).astype(np.float32)
    bw = np.repeat((labels > 0)[..., None], 4, -1).astype(np.float32)
    tg = [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    num_pos = torch.from_numpy((labels > 0).sum(1).astype(np.int32)).cuda()
    return cls, reg, tg, num_pos


def eager_dense(cls, reg, tg, num_pos, C, gamma, alpha=0.25, beta=1.0 / 9.0):
    labels, lw, bt, bw = tg
    B = labels.shape[0]
    x = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1, C) for c in cls], 1).float()
    r = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1, 4) for c in reg], 1).float()
    onehot = (labels[..., None] == torch.arange(1, C + 1, device=labels.device)).float()
    l = F.binary_cross_entropy_with_logits(x, onehot, reduction="none")
    if gamma is not None:
        p = torch.sigmoid(x)
        pt = (1 - p) * onehot + p * (1 - onehot)
        l = l * (alpha * onehot + (1 - alpha) * (1 - onehot)) * pt.pow(gamma)
    avg = float(max(int(num_pos.sum().item()), 1))                              # the host synchronisation
    return torch.stack([(l * lw[..., None]).sum() / avg,
                        (F.smooth_l1_loss(r, bt, beta=beta, reduction="none") * bw).sum() / avg])


def roi_inputs(R, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    cls = (torch.randn(R, C, generator=g) * 2).cuda().requires_grad_(True)
    reg = (torch.randn(R, 4 * C, generator=g) * 0.5).cuda().requires_grad_(True)
    r = np.random.default_rng(seed)
    labels = np.where(r.random(R) < 0.25, r.integers(1, C, R), 0).astype(np.int64)
    lw = (r.random(R) < 0.9).astype(np.float32)
    bt = r.normal(0, 0.5, (R, 4)).astype(np.float32)
    bw = np.repeat(((labels > 0) & (lw > 0))[:, None], 4, -1).astype(np.float32)
    return cls, reg, [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]


def eager_roi(cls, reg, tg):
    labels, lw, bt, bw = tg
    R, C = cls.shape
    avg = float(max(int((lw > 0).sum().item()), 1))
    lc = (F.cross_entropy(cls, labels, reduction="none") * lw).sum() / avg
    tgt = torch.zeros(R, C, 4, device=cls.device)
    wgt = torch.zeros(R, C, 4, device=cls.device)
    idx = labels[:, None, None].expand(R, 1, 4)
    tgt.scatter_(1, idx, bt[:, None])
    wgt.scatter_(1, idx, bw[:, None])
    lr = (F.smooth_l1_loss(reg, tgt.view(R, 4 * C), beta=1.0, reduction="none") * wgt.view(R, 4 * C)).sum() / avg
    return torch.stack([lc, lr])


def measure(name, fn_fused, fn_eager, leaves, floor_bytes, iters, extra):
    cot = torch.ones(2, device="cuda")

    def fused():
        return torch.autograd.grad(fn_fused(), leaves, cot)

    def eager():
        return torch.autograd.grad(fn_eager(), leaves, cot)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fused()
    us_graph = time_events(g.replay, iters)
    us_call = time_events(fused, iters)
    us_eager = time_events(eager, max(5, iters // 10))
    lf, le = fn_fused().detach().cpu().tolist(), fn_eager().detach().cpu().tolist()
    print(json.dumps(dict(extra, op=name, graph_replay_us=round(us_graph, 1), eager_call_us=round(us_call, 1),
                          eager_composition_us=round(us_eager, 1),
                          speedup_vs_eager_composition=round(us_eager / us_graph, 1),
                          floor_bytes=int(floor_bytes), gbps_at_floor_bytes=round(floor_bytes / us_graph / 1e3, 1),
                          losses=lf, losses_eager_composition=le)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    for name, levels, A, C, gamma in (("rpn", C4, 3, 1, None), ("retinanet", RETINA, 9, 80, 2.0)):
        cls, reg, tg, num_pos = dense_inputs(levels, 2, A, C)
        head = sum(t.numel() * 2 for t in cls + reg)
        targets = sum(t.numel() * t.element_size() for t in tg)
        measure(name,
                lambda: T.anchor_head_loss(cls, reg, *tg, avg_factor=num_pos, num_classes=C, gamma=gamma),
                lambda: eager_dense(cls, reg, tg, num_pos, C, gamma), cls + reg, 3 * head + 2 * targets, args.iters,
                dict(B=2, A=A, C=C, dtype="bf16 channels_last", head_elements=head // 2,
                     anchors_per_image=tg[0].shape[1]))
    cls, reg, tg = roi_inputs(1024, 81)
    head = (cls.numel() + reg.numel()) * 4
    measure("roi_head", lambda: T.bbox_head_loss(cls, reg, *tg), lambda: eager_roi(cls, reg, tg), [cls, reg],
            3 * cls.numel() * 4 + reg.numel() * 4 + 2 * sum(t.numel() * t.element_size() for t in tg), args.iters,
            dict(R=1024, C=81, dtype="fp32", head_elements=head // 4))


if __name__ == "__main__":
    main()
