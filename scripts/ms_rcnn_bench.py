#!/usr/bin/env python
"""Mask Scoring R-CNN pieces, time per call replayed from a captured graph (device events after warm-up;
the median of ``--repeats`` measurements of ``--iters`` replays each), at R = 256 rows, C = 81 classes, S = 14 (28 x 28
logits), 256 channels, bf16, and an 800 x 1344 canvas with 30-vertex instances:

  stem    ``mask_iou_stem``: its own launches one by one (the addend; the two backward launches), the whole layer forward
          and forward + backward, and the same layer composed from torch ops (sigmoid, max_pool2d, cat, conv2d, relu,
          autograd) on the same GPU
  target  ``mask_iou_target`` (one launch) and a torch composition that is GIVEN the whole-image ground-truth bitmaps
          (which this project never forms): slice sums by an integral image, threshold, products and sums
  loss    ``mask_iou_loss`` forward + backward and ``mask_scores`` against their torch compositions
  head    ``MaskIoUHead`` (mmdetection's default sizes) forward + backward against the same module in torch

Every step runs in a child process of its own under ``timeout``; the first step that fails ends the run.  Prints one JSON
object per measurement and appends them to profiles/ms_rcnn_bench.jsonl."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"stem": 240, "target": 180, "loss": 120, "head": 300}      # seconds each child may take
R, C, S, CH = 256, 81, 14, 256
CANVAS = (800, 1344)


def time_events(fn, iters, repeats):
    import torch
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
    return [round(statistics.median(got), 2), round(min(got), 2), round(max(got), 2)]


def graphed(fn):
    """fn captured once (after one eager call on a side stream) -> its replay."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def pair(row, key, ours, theirs, args):
    """Times ``ours`` and ``theirs`` by graph replay (``theirs`` eagerly if it cannot be captured) into ``row``."""
    import torch
    g0, _ = graphed(ours)
    t0 = time_events(g0.replay, args.iters, args.repeats)
    row[key + "_graph_replay_us"] = t0
    try:
        g1, _ = graphed(theirs)
        t1 = time_events(g1.replay, args.iters, args.repeats)
        row["torch_" + key + "_graph_replay_us"] = t1
    except Exception as e:
        torch.cuda.synchronize()
        t1 = time_events(theirs, args.iters, args.repeats)
        row["torch_" + key + "_eager_us"] = t1
        row["torch_" + key + "_note"] = "not capturable: %s" % type(e).__name__
    row["ratio_torch_over_ours_" + key] = round(t1[0] / t0[0], 3)


def _logits(gen):
    import torch
    x = 2 * torch.randn(R, C, 2 * S, 2 * S, generator=gen)
    return x.cuda().bfloat16().contiguous(memory_format=torch.channels_last)


def step_stem(T, args):
    import torch
    import torch.nn.functional as F
    from torch_detection_amd import mask_iou_ops as P
    gen = torch.Generator().manual_seed(0)
    cl = torch.channels_last
    feats = torch.randn(R, CH, S, S, generator=gen).cuda().bfloat16().contiguous(memory_format=cl).requires_grad_(True)
    pred = _logits(gen).requires_grad_(True)
    labels = torch.randint(1, C, (R,), generator=gen).cuda()
    conv = torch.nn.Conv2d(CH + 1, CH, 3, padding=1).cuda()
    w, b = conv.weight, conv.bias
    gy = torch.randn(R, CH, S, S, generator=gen).cuda().bfloat16().contiguous(memory_format=cl)
    base = {"R": R, "C": C, "S": S, "Cf": CH, "Cout": CH, "dtype": "bf16", "us_are": "median, min, max",
            "iters": args.iters, "repeats": args.repeats}
    out = []
    a, Pm, idx = P.mask_iou_stem_fwd(pred.detach(), labels, w.detach(), 0, torch.bfloat16)
    gz = gy.permute(0, 2, 3, 1)
    g, _ = graphed(lambda: P.mask_iou_stem_fwd(pred.detach(), labels, w.detach(), 0, torch.bfloat16))
    out.append(dict(base, op="mask_iou_stem_fwd (1 launch)", graph_replay_us=time_events(g.replay, args.iters, args.repeats)))
    g, _ = graphed(lambda: P.mask_iou_stem_bwd(gz, Pm, idx, pred.detach(), labels, w.detach(), 0))
    out.append(dict(base, op="mask_iou_stem_bwd (2 launches)",
                    graph_replay_us=time_events(g.replay, args.iters, args.repeats)))
    tconv = torch.nn.Conv2d(CH + 1, CH, 3, padding=1).cuda().bfloat16().to(memory_format=cl)
    rows = torch.arange(R, device="cuda")

    def torch_layer():
        p = F.max_pool2d(torch.sigmoid(pred[rows, labels])[:, None], 2, 2)
        return F.relu(tconv(torch.cat([feats, p], 1)))

    def fwd():
        with torch.no_grad():
            return T.mask_iou_stem(feats, pred, labels, w, b)

    def t_fwd():
        with torch.no_grad():
            return torch_layer()

    row = dict(base, op="mask_iou_stem")
    pair(row, "forward", fwd, t_fwd, args)
    pair(row, "forward_backward", lambda: torch.autograd.grad(T.mask_iou_stem(feats, pred, labels, w, b),
                                                              [feats, pred, w, b], gy),
         lambda: torch.autograd.grad(torch_layer(), [feats, pred] + list(tconv.parameters()), gy), args)
    out.append(row)
    return out


def _instances(G, nv, seed):
    """B = 2 images of G star-shaped instances of ``nv`` vertices on the canvas, as pack_polygons takes them."""
    import numpy as np
    g = np.random.default_rng(seed)
    h, w = CANVAS
    polys, boxes = [], []
    for b in range(2):
        inst, bx = [], []
        for _ in range(G):
            rx, ry = g.uniform(40, 300), g.uniform(40, 250)
            cx, cy = g.uniform(rx, w - rx), g.uniform(ry, h - ry)
            ang = np.sort(g.uniform(0, 2 * np.pi, nv))
            rad = g.uniform(0.6, 1.0, nv)
            p = np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang)], 1).astype(np.float32)
            inst.append([[float(v) for v in p.reshape(-1)]])
            bx.append([p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()])
        polys.append(inst)
        boxes.append(bx)
    return polys, np.array(boxes, np.float32)


def step_target(T, args):
    import numpy as np
    import torch
    gen = torch.Generator().manual_seed(1)
    G, M = 16, 2 * S
    polys, boxes = _instances(G, 30, 3)
    pg = [t.cuda() for t in T.pack_polygons(polys, G)]
    g = np.random.default_rng(4)
    img = g.integers(0, 2, R)
    inds = g.integers(0, G, R)
    rois = np.concatenate([img[:, None].astype(np.float32), boxes[img, inds] + g.normal(0, 12, (R, 4)).astype(np.float32)], 1)
    rois_d = torch.from_numpy(rois.astype(np.float32)).cuda()
    inds_d = torch.from_numpy(inds.astype(np.int32)).cuda()
    labels = torch.randint(1, C, (R,), generator=gen).cuda()
    pred = _logits(gen)
    targets, _ = T.mask_target(rois_d, inds_d, *pg, mask_size=M)
    shapes = torch.tensor([CANVAS, CANVAS], dtype=torch.int32).cuda()
    # what the torch composition is GIVEN: the instances' bitmaps on the canvas and their integral images
    import ms_rcnn_ref as ref
    xy, po, gpo = (t.cpu().numpy() for t in pg)
    import mask_ref
    maps = np.stack([np.stack([ref.instance_bitmap(mask_ref.instance_polys(xy, po, gpo, b, j), *CANVAS)
                               for j in range(G)]) for b in range(2)])
    integral = torch.from_numpy(np.pad(maps.cumsum(2).cumsum(3), ((0, 0), (0, 0), (1, 0), (1, 0))).astype(np.float32)).cuda()
    full = torch.from_numpy(maps.sum((2, 3)).astype(np.float32)).cuda()
    bi, gi = torch.from_numpy(img).cuda(), torch.from_numpy(inds).cuda()
    rows = torch.arange(R, device="cuda")
    h, w = CANVAS

    def theirs():
        box = rois_d[:, 1:].long()
        x1, y1 = box[:, 0].clamp(0, w), box[:, 1].clamp(0, h)
        x2, y2 = (box[:, 2] + 1).clamp(0, w), (box[:, 3] + 1).clamp(0, h)
        x2, y2 = torch.maximum(x2, x1), torch.maximum(y2, y1)
        I = integral[bi, gi]
        inside = I[rows, y2, x2] - I[rows, y1, x2] - I[rows, y2, x1] + I[rows, y1, x1]
        ratio = inside / (full[bi, gi] + 1e-7)
        mp = (pred[rows, labels].float() > 0.0).float()
        mt = targets.float()
        ov = (mp * mt).sum((-1, -2))
        return ov / (mp.sum((-1, -2)) + mt.sum((-1, -2)) / (ratio + 1e-7) - ov)

    ours = lambda: T.mask_iou_target(rois_d, inds_d, *pg, pred, labels, targets, shapes, thr=0.0)
    a, c = ours().cpu().numpy(), torch.nan_to_num(theirs()).cpu().numpy()
    row = {"op": "mask_iou_target (1 launch)", "R": R, "C": C, "M": M, "canvas": CANVAS, "instances_per_image": G,
           "vertices": 30, "dtype": "bf16", "positive_rows": int((a > 0).sum()),
           "max_abs_difference_from_the_bitmap_composition": float(np.abs(a - c).max()),
           "torch_is_given": "the instances' canvas bitmaps as integral images (%d MB)" % (integral.numel() * 4 >> 20),
           "us_are": "median, min, max", "iters": args.iters, "repeats": args.repeats}
    pair(row, "call", ours, theirs, args)
    return [row]


def step_loss(T, args):
    import torch
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(2)
    pred = torch.randn(R, C, generator=gen).cuda().requires_grad_(True)
    labels = torch.randint(1, C, (R,), generator=gen).cuda()
    targets = torch.where(torch.rand(R, generator=gen) < 0.6, torch.rand(R, generator=gen), torch.zeros(R)).cuda()
    rows = torch.arange(R, device="cuda")
    base = {"R": R, "C": C, "us_are": "median, min, max", "iters": args.iters, "repeats": args.repeats}

    def theirs():
        live = (targets > 0).float()
        d = (pred[rows, labels] - targets) * live
        loss = 0.5 * (d * d).sum() / live.sum().clamp(min=1)
        return (loss,) + torch.autograd.grad(loss, [pred])

    def ours():
        loss = T.mask_iou_loss(pred, labels, targets)
        return (loss,) + torch.autograd.grad(loss, [pred])

    row = dict(base, op="mask_iou_loss forward + backward (3 launches)", dtype="f32")
    pair(row, "forward_backward", ours, theirs, args)
    Bn, N = 2, 100
    ip = torch.randn(Bn * N, C, generator=gen).cuda()
    dets = torch.rand(Bn, N, 5, generator=gen).cuda()
    lab = torch.randint(0, C - 1, (Bn, N), generator=gen).cuda()
    counts = torch.tensor([100, 63], dtype=torch.int32).cuda()
    ar = torch.arange(N, device="cuda")
    row2 = dict(base, op="mask_scores (1 launch)", B=Bn, max_num=N)
    pair(row2, "call", lambda: T.mask_scores(ip, dets, lab, counts),
         lambda: ip.view(Bn, N, C).gather(2, (lab + 1)[..., None])[..., 0] * dets[..., 4] * (ar[None] < counts[:, None]), args)
    return [row, row2]


def step_head(T, args):
    import copy
    import torch
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(3)
    cl = torch.channels_last
    head = T.MaskIoUHead().cuda()
    feats = torch.randn(R, CH, S, S, generator=gen).cuda().bfloat16().contiguous(memory_format=cl).requires_grad_(True)
    pred = _logits(gen).requires_grad_(True)
    labels = torch.randint(1, C, (R,), generator=gen).cuda()
    gout = torch.randn(R, C, generator=gen).cuda()
    params = list(head.parameters())
    convs = copy.deepcopy(head.convs).bfloat16().to(memory_format=cl)
    fcs, last = copy.deepcopy(head.fcs).bfloat16(), copy.deepcopy(head.fc_mask_iou).bfloat16()
    tparams = list(convs.parameters()) + list(fcs.parameters()) + list(last.parameters())
    rows = torch.arange(R, device="cuda")

    def torch_head():
        x = torch.cat([feats, F.max_pool2d(torch.sigmoid(pred[rows, labels])[:, None], 2, 2)], 1)
        for conv in convs:
            x = F.relu(conv(x))
        x = x.reshape(R, -1)
        for fc in fcs:
            x = F.relu(fc(x))
        return last(x).float()

    row = {"op": "MaskIoUHead", "R": R, "C": C, "S": S, "channels": CH, "fc_out_channels": 1024, "dtype": "bf16",
           "us_are": "median, min, max", "iters": args.iters, "repeats": args.repeats}

    def fwd():
        with torch.no_grad():
            return head(feats, pred, labels)

    def t_fwd():
        with torch.no_grad():
            return torch_head()

    pair(row, "forward", fwd, t_fwd, args)
    pair(row, "forward_backward", lambda: torch.autograd.grad(head(feats, pred, labels), [feats, pred] + params, gout),
         lambda: torch.autograd.grad(torch_head(), [feats, pred] + tparams, gout), args)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_rcnn_bench.jsonl"))
    args = ap.parse_args()
    steps = {"stem": step_stem, "target": step_target, "loss": step_loss, "head": step_head}
    if args.step:                                   # a child: one step on the GPU, its JSON lines on stdout
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))          # the target step builds its bitmaps with the CPU oracle
        import torch_detection_amd as T
        for ln in steps[args.step](T, args):
            print("JSON " + json.dumps(ln), flush=True)
        return 0
    lines = []
    for name in ("stem", "target", "loss", "head"):
        cmd = ["timeout", "-k", "10", str(STEPS[name]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--iters", str(args.iters), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        for ln in p.stdout.splitlines():
            if ln.startswith("JSON "):
                lines.append(json.loads(ln[5:]))
                print(ln[5:], flush=True)
        if p.returncode != 0:
            print("step %s ended with status %d: stopping" % (name, p.returncode), file=sys.stderr)
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
