#!/usr/bin/env python
"""Cascade R-CNN pieces, time per call replayed from a captured graph (device events after warm-up; the
median of ``--repeats`` measurements of ``--iters`` replays each):

  refine   ``refine_bboxes`` row-aligned (labels given, and the arg-max of bf16 logits) and compacted (P = 512, ground
           truths dropped) at R = 1024 rows of one image and of two images (2 x 512), C = 81, class-specific (R, 4C)
           and class-agnostic (R, 4) bf16 deltas
  detect   ``cascade_detections`` with S = 1 and S = 3 stages and ``bbox_head_detections`` (the baseline) on the same
           rows, C = 81, bf16, max_per_img 100
  head     ``CascadeRoIHead`` (3 stages, 256 channels, fc 1024, class-agnostic, num = 512) at B = 2 on a four-level
           pyramid of a 256 x 384 image, 1000 proposals per image: ``forward_train`` (forward only, replayed),
           ``simple_test`` (replayed), and the eager forward + backward

Every step runs in a child process of its own under ``timeout``; the first step that fails ends the run.  Prints one JSON
object per measurement and appends them to profiles/cascade_bench.jsonl."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"refine": 240, "detect": 240, "head": 420}           # seconds each child may take
C = 81
SHAPE = (800, 1344)


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


def rows(B, per_img, seed=0):
    import numpy as np
    import torch
    g = np.random.default_rng(seed)
    R = B * per_img
    centres = g.uniform(100, 1200, (40, 2)) * [1.0, 0.55]
    k = g.integers(0, 40, R)
    xy = centres[k] + g.normal(0, 24, (R, 2))
    wh = g.uniform(40, 260, (R, 2))
    img = np.repeat(np.arange(B), per_img)[:, None]
    rois = np.concatenate([img, xy - wh / 2, xy + wh / 2], 1).astype(np.float32)
    x = [g.normal(0, 1.0, (R, C)) for _ in range(3)]
    sure = g.random(R) < 0.25
    for xs in x:
        xs[:, 0] += 4.0
        xs[sure, 1 + (k[sure] * 7) % (C - 1)] += 9.0
    d = g.normal(0, 0.5, (R, 4 * C))
    labels = g.integers(0, C, R)
    gt = rois[:B * 8, 1:].reshape(B, 8, 4).copy()
    gi = np.full((R,), -1, np.int32)
    gi[::16] = 0
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(rois=cuda(rois), cls=[cuda(v).bfloat16() for v in x], reg=cuda(d).bfloat16(),
                reg4=cuda(d[:, 4:8]).bfloat16(), labels=cuda(labels), gt=cuda(gt), gi=cuda(gi),
                shapes=torch.tensor([SHAPE] * B, dtype=torch.int32).cuda())


def step_refine(T, args):
    out = []
    for B, per in ((1, 1024), (2, 512)):
        a = rows(B, per)
        for name, reg in (("class_specific", a["reg"]), ("class_agnostic", a["reg4"])):
            g0, _ = graphed(lambda: T.refine_bboxes(a["rois"], reg, a["shapes"], labels=a["labels"]))
            g1, _ = graphed(lambda: T.refine_bboxes(a["rois"], reg, a["shapes"], cls_score=a["cls"][0]))
            g2, k2 = graphed(lambda: T.refine_bboxes(a["rois"], reg, a["shapes"], labels=a["labels"],
                                                     pos_assigned_gt_inds=a["gi"], gt_bboxes=a["gt"], max_per_img=512))
            moved = a["rois"].numel() * 4 * 2 + a["cls"][0].numel() * 2 + B * per * 8
            out.append({"op": "refine_bboxes", "B": B, "R": B * per, "C": C, "deltas": name, "dtype": "bf16",
                        "row_aligned_labels_graph_replay_us": time_events(g0.replay, args.iters, args.repeats),
                        "row_aligned_argmax_graph_replay_us": time_events(g1.replay, args.iters, args.repeats),
                        "compacted_labels_P512_graph_replay_us": time_events(g2.replay, args.iters, args.repeats),
                        "row_aligned_bytes_touched": moved, "counts": k2[1].cpu().tolist(),
                        "us_are": "median, min, max", "iters": args.iters, "repeats": args.repeats})
    return out


def step_detect(T, args):
    out = []
    cfg = dict(score_thr=0.05, nms_thr=0.5, max_per_img=100)
    for B, per in ((1, 1024), (2, 512)):
        a = rows(B, per)
        base, kb = graphed(lambda: T.bbox_head_detections(a["rois"], a["cls"][0], a["reg"], a["shapes"], **cfg))
        s1, k1 = graphed(lambda: T.cascade_detections(a["rois"], a["cls"][:1], a["reg"], a["shapes"], **cfg))
        s3, k3 = graphed(lambda: T.cascade_detections(a["rois"], a["cls"], a["reg"], a["shapes"], **cfg))
        tb = time_events(base.replay, args.iters, args.repeats)
        t1 = time_events(s1.replay, args.iters, args.repeats)
        t3 = time_events(s3.replay, args.iters, args.repeats)
        out.append({"op": "cascade_detections", "B": B, "R": B * per, "C": C, **cfg, "dtype": "bf16",
                    "bbox_head_detections_graph_replay_us": tb, "cascade_S1_graph_replay_us": t1,
                    "cascade_S3_graph_replay_us": t3, "ratio_S3_over_bbox_head_detections": round(t3[0] / tb[0], 3),
                    "ratio_S1_over_bbox_head_detections": round(t1[0] / tb[0], 3),
                    "S1_equals_bbox_head_detections": all(bool((x == y).all()) for x, y in zip(kb, k1)),
                    "counts_S3": k3[3].cpu().tolist(), "us_are": "median, min, max", "iters": args.iters,
                    "repeats": args.repeats})
    return out


def step_head(T, args):
    import torch
    torch.manual_seed(0)
    B, P = 2, 1000
    H, W = 256, 384
    head = T.CascadeRoIHead().cuda()
    with torch.no_grad():                           # an untrained fc_cls scores every class 1 / 81: nothing to select
        for h in head.bbox_head:
            h.fc_cls.weight.mul_(100)
            h.fc_reg.weight.mul_(100)
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(B, 256, H // s, W // s, generator=g).cuda().bfloat16()
             .contiguous(memory_format=torch.channels_last) for s in (4, 8, 16, 32)]
    gxy = torch.rand(B, 8, 2, generator=g) * torch.tensor([W - 120.0, H - 120.0])
    gt = torch.cat([gxy, gxy + torch.rand(B, 8, 2, generator=g) * 100 + 16], -1).contiguous().cuda()
    gt_labels = torch.randint(1, C, (B, 8), generator=g).cuda()
    gt_counts = torch.full((B,), 8, dtype=torch.int32).cuda()
    jit = gt.cpu()[:, torch.arange(P) % 8] + torch.randn(B, P, 4, generator=g) * torch.linspace(1, 24, P).view(1, P, 1)
    props = torch.cat([jit, torch.rand(B, P, 1, generator=g)], -1).contiguous().cuda()
    counts = torch.full((B,), P, dtype=torch.int32).cuda()
    ish = torch.tensor([(H, W)] * B, dtype=torch.int32).cuda()

    def train():
        return head.forward_train(feats, props, counts, gt, gt_labels, gt_counts, ish, seed=3)

    def train_bwd():
        head.zero_grad(set_to_none=True)
        sum(train().values()).backward()

    def test():
        return head.simple_test(feats, props, counts, ish)

    gtr, ktr = graphed(train)
    gte, kte = graphed(test)
    return [{"op": "CascadeRoIHead", "B": B, "channels": 256, "fc_out_channels": 1024, "stages": 3, "num": 512,
             "proposals_per_image": P, "pyramid": [[H // s, W // s] for s in (4, 8, 16, 32)], "dtype": "bf16",
             "forward_train_graph_replay_us": time_events(gtr.replay, max(5, args.iters // 10), args.repeats),
             "simple_test_graph_replay_us": time_events(gte.replay, max(5, args.iters // 10), args.repeats),
             "forward_train_plus_backward_eager_us": time_events(train_bwd, max(3, args.iters // 20), args.repeats),
             "losses": {k: round(float(v.detach()), 4) for k, v in ktr.items()}, "test_counts": kte[3].cpu().tolist(),
             "us_are": "median, min, max", "iters": args.iters, "repeats": args.repeats}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_bench.jsonl"))
    args = ap.parse_args()
    if args.step:                                   # a child: one step on the GPU, its JSON lines on stdout
        sys.path.insert(0, ROOT)
        import torch_detection_amd as T
        for ln in {"refine": step_refine, "detect": step_detect, "head": step_head}[args.step](T, args):
            print("JSON " + json.dumps(ln), flush=True)
        return 0
    lines = []
    for name in ("refine", "detect", "head"):
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
