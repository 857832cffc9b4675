#!/usr/bin/env python
"""The fused SGD step on ResNet-50-FPN's real parameter set with a gradient reducer attached (the gradients are views of
its flat buffer), in two weight layouts — ``as_built``: the layers' channels_last 3x3 weights, which is the reducer's
gradient layout; ``contiguous``: OIHW weights, against which the reducer's [O][kh][kw][I] views are permuted (the
transposed path) — beside the update a user writes without it ON THE SAME TENSORS: ``clip_grad_norm_(params, 35)`` +
``torch.optim.SGD(foreach=True).step()``.  Both are timed as a captured graph
replay (device time, no host in the way) and as eager calls; launches are counted from a recorded launch plan (ours)
and from the profiler's kernel list (torch).  The gradients are seeded and small (norm < 35), so neither side's clip
changes them and repeated steps keep the parameters in range.  Device events after warm-up; the median of ``--repeats``
measurements of ``--iters`` calls each.  Prints one JSON object per configuration and appends it to
profiles/optim_bench.jsonl.  The bytes model: 20 B per element for the update, 4 B for the norm, over
the 6.29 TB/s a float4 copy reaches on this GPU."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_detection_amd as T  # noqa: E402
from torch_detection_amd import _lib, dp  # noqa: E402

COPY_RATE = 6.29e12
MAX_NORM = 35.0


def model(weights):
    rb = T.ResNet(50).cuda().train()
    rb.init_weights()
    rf = T.FPN([256, 512, 1024, 2048], 256, 5).cuda()
    rf.init_weights()
    if weights == "contiguous":
        for p in list(rb.parameters()) + list(rf.parameters()):
            p.data = p.data.contiguous()
    red = dp.attach_reducer([rf, rb])
    params = [p for p in list(rb.parameters()) + list(rf.parameters()) if p.grad is not None]
    red.flat.copy_(torch.randn(red.flat.numel(), generator=torch.Generator().manual_seed(0)).mul_(1e-3))
    return rb, rf, red, params


def groups(params):
    """mmdetection's norm_decay_mult = 0: weights decay, norm scales and shifts do not."""
    return [dict(params=[p for p in params if p.dim() == 4], weight_decay=1e-4),
            dict(params=[p for p in params if p.dim() != 4], weight_decay=0.0)]


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
        fn()
    return g


def plan_launches(fn):
    """Launches of the library that one call of ``fn`` makes (tdn_plan_*)."""
    lib = _lib.load()
    _lib.check(lib.tdn_plan_begin(), "tdn_plan_begin")
    try:
        fn()
    finally:
        plan = lib.tdn_plan_end()
    out = (ctypes.c_int32 * 3)()
    lib.tdn_plan_stats(plan, out)
    lib.tdn_plan_free(plan)
    torch.cuda.synchronize()
    return int(out[0])


def profiled_kernels(fn):
    """Kernels one call of ``fn`` launches, from the profiler; None when this build of torch records no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) == torch.autograd.DeviceType.CUDA)
        return n or None
    except Exception:  # noqa: BLE001 - a figure we may have to report as not measured
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.jsonl"))
    args = ap.parse_args()
    for weights, name, kw in (("as_built", "momentum_clip", dict()),
                              ("as_built", "nesterov_clip_dynamic_scale", dict(nesterov=True)),
                              ("contiguous", "momentum_clip", dict())):
        rb, rf, red, params = model(weights)
        numel = sum(p.numel() for p in params)
        permuted = sum(p.numel() for p in params if p.grad.stride() != p.stride())
        floor_us = (20 * numel + 4 * numel) / COPY_RATE * 1e6
        opt = T.SGD(groups(params), lr=0.02, momentum=0.9, max_norm=MAX_NORM,
                    loss_scale="dynamic" if kw else None, init_scale=1.0, **kw)
        opt.step()
        torch.cuda.synchronize()
        launches = plan_launches(opt.step)
        g = graphed(opt.step)
        us_graph = time_events(g.replay, args.iters, args.repeats)
        us_call = time_events(opt.step, args.iters, args.repeats)
        taken, skipped = int(opt.steps_taken.item()), int(opt.steps_skipped.item())
        paths = opt._plan.paths
        base = torch.optim.SGD(groups(params), lr=0.02, momentum=0.9, foreach=True, **kw)

        def base_step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            base.step()

        base_kernels = profiled_kernels(base_step)
        us_base_call = time_events(base_step, max(2, args.iters // 10), args.repeats)
        try:
            us_base_graph = time_events(graphed(base_step).replay, max(2, args.iters // 10), args.repeats)
        except Exception as e:  # noqa: BLE001 - the baseline may refuse capture; the eager figure stands alone then
            torch.cuda.synchronize()
            us_base_graph = None
            print("baseline not capturable: %s" % e, file=sys.stderr)
        best_base = us_base_graph[0] if us_base_graph else us_base_call[0]
        line = {
            "config": name, "weights": weights, "model": "ResNet-50-FPN, reducer attached", "parameters": len(params),
            "elements": numel,
            "elements_with_permuted_gradient": permuted,
            "items_linear_transposed_general": [paths.count(k) for k in (0, 1, 2)],
            "update_chunks": opt._plan.update_chunks, "norm_chunks": opt._plan.norm_chunks,
            "fused_graph_replay_us": us_graph, "fused_eager_call_us": us_call, "fused_launches": launches,
            "steps_taken": taken, "steps_skipped": skipped,
            "torch_foreach_clip_graph_replay_us": us_base_graph, "torch_foreach_clip_eager_call_us": us_base_call,
            "torch_kernels": base_kernels,
            "bytes_model_MB": [round(20 * numel / 1e6, 1), round(4 * numel / 1e6, 1)], "bytes_floor_us": round(floor_us, 1),
            "ratio_to_baseline": round(us_graph[0] / best_base, 3), "ratio_to_bytes_floor": round(us_graph[0] / floor_us, 2),
            "iters": args.iters, "repeats": args.repeats}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        del opt, base, g, rb, rf, red, params


if __name__ == "__main__":
    main()
