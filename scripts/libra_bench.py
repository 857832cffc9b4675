#!/usr/bin/env python
"""Libra R-CNN pieces, time per call replayed from a captured graph (device events after warm-up; the
median of ``--repeats`` measurements of ``--iters`` replays each):

  bfp    the BFP neck at the benchmark pyramid (B = 2, C = 256, bf16, levels 200x336, 100x168, 50x84, 25x42, 13x21,
         refine_level 2) with refine_type None and 'conv': forward, and forward + backward; for refine_type None also the
         four launches one by one with the bytes each moves when every tensor is touched once, the bytes/s that gives,
         and the same computation composed from torch ops (adaptive_max_pool2d, interpolate, autograd) on the same GPU
  sample ``sample_rois`` with the random and the IoU-balanced negative sampler at 2 x 2000 proposals, 40 ground truths per
         image, num = 512
  loss   ``bbox_head_loss`` with smooth L1 and with balanced L1 at R = 1024, C = 81, bf16, forward + backward

Every step runs in a child process of its own under ``timeout``; the first step that fails ends the run.  Prints one JSON
object per measurement and writes them to profiles/libra_bench.jsonl (a run replaces the file)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"bfp": 300, "sample": 120, "loss": 120}             # seconds each child may take
SIZES = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
B, C, REFINE = 2, 256, 2


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


def step_bfp(T, args):
    import torch
    import torch.nn.functional as F
    from torch_detection_amd import libra_ops as P
    gen = torch.Generator().manual_seed(0)
    cl = torch.channels_last
    xs = [torch.randn(B, C, h, w, generator=gen).cuda().bfloat16().contiguous(memory_format=cl) for h, w in SIZES]
    gs = [torch.randn(B, C, h, w, generator=gen).cuda().bfloat16().contiguous(memory_format=cl) for h, w in SIZES]
    px = [h * w for h, w in SIZES]
    level = [B * n * C * 2 for n in px]                     # bytes of one map of each level
    pyramid, bsf_bytes = sum(level), level[REFINE]
    iters = max(5, args.iters // 4)
    out = []
    # the four launches, each tensor touched once
    bsf = P.bfp_gather_fwd(xs, REFINE)
    dref = P.bfp_scatter_bwd(gs, bsf, REFINE)
    launches = {
        "gather_fwd": (lambda: P.bfp_gather_fwd(xs, REFINE), pyramid + bsf_bytes),
        "scatter_fwd": (lambda: P.bfp_scatter_fwd(xs, bsf, REFINE), 2 * pyramid + bsf_bytes),
        "scatter_bwd": (lambda: P.bfp_scatter_bwd(gs, bsf, REFINE), pyramid + 2 * bsf_bytes),
        "gather_bwd": (lambda: P.bfp_gather_bwd(xs, gs, dref, REFINE), 3 * pyramid + bsf_bytes),
    }
    for name, (fn, moved) in launches.items():
        g, _ = graphed(fn)
        t = time_events(g.replay, iters, args.repeats)
        out.append({"op": "bfp_" + name, "B": B, "C": C, "sizes": SIZES, "refine_level": REFINE, "dtype": "bf16",
                    "graph_replay_us": t, "bytes_each_tensor_once": moved,
                    "GB_per_s_each_tensor_once": round(moved / t[0] / 1e3, 1), "us_are": "median, min, max",
                    "iters": iters, "repeats": args.repeats})

    # the module, and the torch composition of the same computation
    def torch_bfp(feats, conv=None):
        size = feats[REFINE].shape[2:]
        parts = [F.adaptive_max_pool2d(x, output_size=size) if l < REFINE else F.interpolate(x, size=size, mode="nearest")
                 for l, x in enumerate(feats)]
        bsf_ = sum(parts) / len(parts)
        if conv is not None:
            bsf_ = F.relu(conv(bsf_))
        return [(F.interpolate(bsf_, size=x.shape[2:], mode="nearest") if l < REFINE else
                 F.adaptive_max_pool2d(bsf_, output_size=x.shape[2:])) + x for l, x in enumerate(feats)]

    for refine_type in (None, "conv"):
        neck = T.BFP(C, len(SIZES), REFINE, refine_type).cuda()
        neck.init_weights()
        conv = None
        if refine_type == "conv":
            conv = torch.nn.Conv2d(C, C, 3, padding=1).cuda().bfloat16().to(memory_format=cl)
        leaves = [x.detach().clone().requires_grad_(True) for x in xs]
        params = list(neck.parameters())
        tparams = list(conv.parameters()) if conv is not None else []

        def fwd():
            with torch.no_grad():
                return neck(leaves)

        def fwd_bwd():
            return torch.autograd.grad(neck(leaves), leaves + params, gs)

        def t_fwd():
            with torch.no_grad():
                return torch_bfp(leaves, conv)

        def t_fwd_bwd():
            return torch.autograd.grad(torch_bfp(leaves, conv), leaves + tparams, gs)

        row = {"op": "BFP", "B": B, "C": C, "sizes": SIZES, "refine_level": REFINE, "refine_type": refine_type,
               "dtype": "bf16", "us_are": "median, min, max", "iters": iters, "repeats": args.repeats}
        for key, ours, theirs in (("forward", fwd, t_fwd), ("forward_backward", fwd_bwd, t_fwd_bwd)):
            g0, _ = graphed(ours)
            t0 = time_events(g0.replay, iters, args.repeats)
            row[key + "_graph_replay_us"] = t0
            try:
                g1, _ = graphed(theirs)
                t1 = time_events(g1.replay, iters, args.repeats)
                row["torch_" + key + "_graph_replay_us"] = t1
            except Exception as e:                          # a torch op that cannot be captured: time it eagerly
                torch.cuda.synchronize()
                t1 = time_events(theirs, iters, args.repeats)
                row["torch_" + key + "_eager_us"] = t1
                row["torch_" + key + "_note"] = "not capturable: %s" % type(e).__name__
            row["ratio_torch_over_ours_" + key] = round(t1[0] / t0[0], 3)
        if refine_type is None:
            fwd_bytes = launches["gather_fwd"][1] + launches["scatter_fwd"][1]
            all_bytes = sum(v[1] for v in launches.values())
            row["forward_bytes_each_tensor_once"] = fwd_bytes
            row["forward_GB_per_s_each_tensor_once"] = round(fwd_bytes / row["forward_graph_replay_us"][0] / 1e3, 1)
            row["forward_backward_bytes_each_tensor_once"] = all_bytes
            row["forward_backward_GB_per_s_each_tensor_once"] = round(
                all_bytes / row["forward_backward_graph_replay_us"][0] / 1e3, 1)
        out.append(row)
    return out


def step_sample(T, args):
    import numpy as np
    import torch
    g = np.random.default_rng(0)
    Bn, P, G = 2, 2000, 40
    xy = g.uniform(0, 1000, (Bn, G, 2))
    gt = np.concatenate([xy, xy + g.uniform(40, 300, (Bn, G, 2))], 2).astype(np.float32)
    src = gt[np.arange(Bn)[:, None], g.integers(0, G, (Bn, P))]
    size = np.tile(src[..., 2:] - src[..., :2], 2)
    box = src + g.normal(0, 1, (Bn, P, 4)) * size * g.choice([0.02, 0.1, 0.25, 0.5, 2.0], (Bn, P, 1))
    box[..., 2:] = np.maximum(box[..., 2:], box[..., :2] + 2)
    props = torch.from_numpy(np.concatenate([box, g.random((Bn, P, 1))], 2).astype(np.float32)).cuda()
    counts = torch.full((Bn,), P, dtype=torch.int32).cuda()
    gtd = torch.from_numpy(gt).cuda()
    labels = torch.from_numpy(g.integers(1, 81, (Bn, G))).cuda()
    gcnt = torch.full((Bn,), G, dtype=torch.int32).cuda()
    row = {"op": "sample_rois", "B": Bn, "proposals_per_image": P, "gt_per_image": G, "num": 512, "us_are": "median, min, max",
           "iters": args.iters, "repeats": args.repeats}
    for name, kw in (("random", {}), ("iou_balanced", dict(neg_sampler="iou_balanced")),
                     ("iou_balanced_floor", dict(neg_sampler="iou_balanced", floor_thr=0.1, floor_fraction=0.25))):
        gr, keep = graphed(lambda: T.sample_rois(props, counts, gtd, labels, gcnt, seed=3, **kw))
        row[name + "_graph_replay_us"] = time_events(gr.replay, args.iters, args.repeats)
        row[name + "_num_pos_neg"] = [keep[6].cpu().tolist(), keep[7].cpu().tolist()]
    row["ratio_iou_balanced_over_random"] = round(row["iou_balanced_graph_replay_us"][0] /
                                                  row["random_graph_replay_us"][0], 3)
    row["ratio_iou_balanced_floor_over_random"] = round(row["iou_balanced_floor_graph_replay_us"][0] /
                                                        row["random_graph_replay_us"][0], 3)
    return [row]


def step_loss(T, args):
    import numpy as np
    import torch
    R, Cn = 1024, 81
    g = np.random.default_rng(0)
    cls = torch.from_numpy(g.normal(0, 2, (R, Cn)).astype(np.float32)).cuda().bfloat16().requires_grad_(True)
    reg = torch.from_numpy(g.normal(0, 0.5, (R, 4 * Cn)).astype(np.float32)).cuda().bfloat16().requires_grad_(True)
    labels = torch.from_numpy(np.where(g.random(R) < 0.25, g.integers(1, Cn, R), 0).astype(np.int64)).cuda()
    lw = torch.ones(R, device="cuda")
    bt = torch.from_numpy(g.normal(0, 0.5, (R, 4)).astype(np.float32)).cuda()
    bw = (labels > 0).float()[:, None].repeat(1, 4).contiguous()
    gt = torch.ones(2, device="cuda")
    row = {"op": "bbox_head_loss", "R": R, "C": Cn, "dtype": "bf16", "us_are": "median, min, max", "iters": args.iters,
           "repeats": args.repeats}
    for name, kw in (("smooth_l1", {}), ("balanced_l1", dict(reg_loss="balanced_l1"))):
        def step():
            losses = T.bbox_head_loss(cls, reg, labels, lw, bt, bw, **kw)
            return (losses,) + torch.autograd.grad(losses, [cls, reg], gt)
        gr, keep = graphed(step)
        row[name + "_forward_backward_graph_replay_us"] = time_events(gr.replay, args.iters, args.repeats)
        row[name + "_losses"] = [round(float(v), 5) for v in keep[0].detach().cpu()]
    row["ratio_balanced_over_smooth"] = round(row["balanced_l1_forward_backward_graph_replay_us"][0] /
                                              row["smooth_l1_forward_backward_graph_replay_us"][0], 3)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "libra_bench.jsonl"))
    args = ap.parse_args()
    if args.step:                                   # a child: one step on the GPU, its JSON lines on stdout
        sys.path.insert(0, ROOT)
        import torch_detection_amd as T
        for ln in {"bfp": step_bfp, "sample": step_sample, "loss": step_loss}[args.step](T, args):
            print("JSON " + json.dumps(ln), flush=True)
        return 0
    lines = []
    for name in ("bfp", "sample", "loss"):
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
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
