#!/usr/bin/env python
"""Forward + backward of the gradient-harmonised losses (``ghm_head_loss``) replayed from a captured graph
at the RetinaNet shape of ``loss_bench.py`` (strides 8..128 at 800x1344, B = 2, A = 9, C = 80, bf16 channels_last), beside

  (a) the focal ``anchor_head_loss`` of the same tree on the same tensors, also replayed from a graph, and
  (b) an eager torch composition that follows mmdetection's GHMC / GHMR: per level, a Python loop over the bins with one
      ``.item()`` per bin, expanded (N, C) targets, autograd.

Device events after warm-up; (a) and the GHM graph alternate over ``--repeats`` windows of ``--iters`` replays each and
the spread is printed.  Bytes: the each-tensor-once floor of a loss (head outputs read forward and backward, gradients
written, targets read twice) and what GHM has to move (the forward reads heads and targets twice: once to count, once
for the loss).  One JSON object per line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch_detection_amd as T  # noqa: E402
from loss_bench import RETINA, dense_inputs  # noqa: E402
from proposal_bench import time_events  # noqa: E402

BINS_C, BINS_R, MMT_C, MMT_R, MU = 30, 10, 0.75, 0.7, 0.02


def _weights(g, valid, bins, last_edge, mmt, acc):
    edges = torch.arange(bins + 1, device=g.device, dtype=torch.float32) / bins
    edges[-1] = last_edge
    weights = torch.zeros_like(g)
    tot = max(valid.float().sum().item(), 1.0)
    n = 0
    for i in range(bins):
        inds = (g >= edges[i]) & (g < edges[i + 1]) & valid
        num_in_bin = inds.sum().item()                      # the host synchronisation, once per bin and level
        if num_in_bin > 0:
            acc[i] = mmt * acc[i] + (1 - mmt) * num_in_bin
            weights[inds] = tot / acc[i]
            n += 1
    if n > 0:
        weights = weights / n
    return weights, tot


def eager_ghm(cls, reg, tg, C, acc_c, acc_r):
    labels, lw, bt, bw = tg
    B = labels.shape[0]
    total, n0 = 0, 0
    for c, r in zip(cls, reg):
        x = c.permute(0, 2, 3, 1).reshape(B, -1, C).float()
        d = r.permute(0, 2, 3, 1).reshape(B, -1, 4).float()
        n1 = n0 + x.shape[1]
        onehot = (labels[:, n0:n1, None] == torch.arange(1, C + 1, device=labels.device)).float()
        valid = (lw[:, n0:n1, None] > 0).expand_as(x)
        g = (x.sigmoid().detach() - onehot).abs()
        w, tot = _weights(g, valid, BINS_C, 1 + 1e-6, MMT_C, acc_c)
        lc = F.binary_cross_entropy_with_logits(x, onehot, w, reduction="sum") / tot
        diff = d - bt[:, n0:n1]
        l = torch.sqrt(diff * diff + MU * MU) - MU
        g = (diff / torch.sqrt(MU * MU + diff * diff)).abs().detach()
        w, tot = _weights(g, bw[:, n0:n1] > 0, BINS_R, 1e3, MMT_R, acc_r)
        total = total + torch.stack([lc, (l * w).sum() / tot])
        n0 = n1
    return total


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ghm_bench.py measures on the GPU"
    A, C = 9, 80
    cls, reg, tg, num_pos = dense_inputs(RETINA, 2, A, C)
    leaves = cls + reg
    cot = torch.ones(2, device="cuda")
    acc = [torch.zeros(BINS_C, device="cuda"), torch.zeros(BINS_R, device="cuda")]

    def ghm():
        return torch.autograd.grad(T.ghm_head_loss(cls, reg, *tg, acc[0], acc[1], C, BINS_C, BINS_R, MMT_C, MMT_R, MU),
                                   leaves, cot)

    def focal():
        return torch.autograd.grad(T.anchor_head_loss(cls, reg, *tg, avg_factor=num_pos, num_classes=C, gamma=2.0),
                                   leaves, cot)

    acc_e = [torch.zeros(BINS_C, device="cuda"), torch.zeros(BINS_R, device="cuda")]

    def eager():
        return torch.autograd.grad(eager_ghm(cls, reg, tg, C, *acc_e), leaves, cot)

    g_ghm, g_focal = graphed(ghm), graphed(focal)
    t_ghm, t_focal = [], []
    for _ in range(args.repeats):                            # alternating windows: other work shares the machine
        t_focal.append(time_events(g_focal.replay, args.iters))
        t_ghm.append(time_events(g_ghm.replay, args.iters))
    us_call = time_events(ghm, args.iters)
    us_eager = time_events(eager, 3)
    head = sum(t.numel() * 2 for t in leaves)
    targets = sum(t.numel() * t.element_size() for t in tg)
    floor, moved = 3 * head + 2 * targets, 4 * head + 3 * targets
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    spread = lambda v: dict(min=round(min(v), 1), median=round(med(v), 1), max=round(max(v), 1))  # noqa: E731
    acc[0].zero_(), acc[1].zero_(), acc_e[0].zero_(), acc_e[1].zero_()
    lf = T.ghm_head_loss(cls, reg, *tg, acc[0], acc[1], C, BINS_C, BINS_R, MMT_C, MMT_R, MU).detach().cpu().tolist()
    le = eager_ghm(cls, reg, tg, C, *acc_e).detach().cpu().tolist()
    print(json.dumps(dict(op="ghm_head_loss fwd+bwd", shape="retinanet 800x1344", B=2, A=A, C=C,
                          dtype="bf16 channels_last", head_elements=head // 2, anchors_per_image=tg[0].shape[1],
                          bins=[BINS_C, BINS_R], momentum=[MMT_C, MMT_R], iters=args.iters, repeats=args.repeats,
                          ghm_graph_replay_us=spread(t_ghm), focal_graph_replay_us=spread(t_focal),
                          ghm_over_focal=round(med(t_ghm) / med(t_focal), 2), ghm_eager_call_us=round(us_call, 1),
                          eager_mmdet_composition_us=round(us_eager, 1),
                          speedup_vs_eager_composition=round(us_eager / med(t_ghm), 1),
                          floor_bytes=int(floor), ghm_bytes=int(moved),
                          ghm_gbps_at_its_bytes=round(moved / med(t_ghm) / 1e3, 1),
                          focal_gbps_at_floor_bytes=round(floor / med(t_focal) / 1e3, 1),
                          losses=lf, losses_eager_composition=le)), flush=True)


if __name__ == "__main__":
    main()
