#!/usr/bin/env python
"""The 2x2 stride-2 transposed convolution of the mask head (csrc/deconv.hip) at the head's own shapes,
beside three yardsticks that are never the code under test, all on the same tensors:

  (a) ``composed``: what the kernels avoid — ``linear_fwd`` into a scratch (M, 4 Cout) buffer plus a pixel-shuffle copy
      into the NHWC map (the copy is torch's, one strided ``copy_``);
  (b) ``torch``: ``F.conv_transpose2d`` on the GPU (channels_last, same dtype) and the two halves of its backward
      (the stride-2 ``conv2d`` that is its input gradient; ``conv2d_weight`` + the bias sum);
  (c) ``share_of_copy_rate``: the bytes each launch has to move (operands read once, results written once) over its
      time, as a fraction of the 6.29 TB/s float4 copy rate DESIGN.md §4h records.

It also times the whole ``FCNMaskHead`` forward (+ backward at the training shapes) beside the same layers in torch.

Method (scripts/linear_bench.py): every arm is captured as a graph of ``--inner`` calls and replayed; device events after
warm-up; the arms of one product are alternated inside each of ``--repeats`` windows; median, min and max are reported.
Every (dtype, R) step runs in a child process of its own under its own time limit; the first step that fails or times
out ends the run.  Prints one JSON object per measurement and appends it to ``--out``."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
PEAK = 2.5e15
H = W = 14
CIN = COUT = 256
STEPS = [(128, True), (256, True), (100, False), (200, False)]


def graphed(fn, inner):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


def measure(arms, inner, iters, repeats):
    """arms: {name: callable}.  -> {name: [median, min, max] microseconds per call, or an error string}."""
    graphs, out = {}, {}
    for name, fn in arms.items():
        try:
            graphs[name] = graphed(fn, inner)
        except Exception as e:  # noqa: BLE001 - an arm that cannot run here is reported, not hidden
            torch.cuda.synchronize()
            out[name] = "not measured: %s" % str(e).split("\n")[0][:160]
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    got = {name: [] for name in graphs}
    for _ in range(repeats):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            got[name].append(e0.elapsed_time(e1) / (iters * inner) * 1e3)
    for name, v in got.items():
        out[name] = [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)]
    return out


def emit(line, path):
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(line) + "\n")


def per(v, us):
    return None if not isinstance(us, list) else v / (us[0] * 1e-6)


def products(R, dtype, train):
    """{product: (flop, bytes, {arm: fn})} of the deconv at R RoIs."""
    from torch_detection_amd import deconv_ops as D, linear_ops as L
    gen = torch.Generator().manual_seed(R)
    M = R * H * W
    x = torch.randn(R, H, W, CIN, generator=gen).cuda().to(dtype).permute(0, 3, 1, 2)
    w = (torch.randn(CIN, COUT, 2, 2, generator=gen) / CIN ** 0.5).cuda()
    b = torch.randn(COUT, generator=gen).cuda()
    g = torch.randn(R, 2 * H, 2 * W, COUT, generator=gen).cuda().to(dtype).permute(0, 3, 1, 2)
    w_fwd, w_dgrad = D.pack_deconv_weight(w, True, dtype)
    dw, db = torch.empty(CIN, COUT, 2, 2, device="cuda"), torch.empty(COUT, device="cuda")
    w16, b16 = w.to(dtype), b.to(dtype)
    x2 = x.permute(0, 2, 3, 1).reshape(M, CIN)
    b4 = b.repeat(4)
    ybuf = torch.empty(R, 2 * H, 2 * W, COUT, dtype=dtype, device="cuda")

    def composed():
        s = L.linear_fwd(x2, w_fwd, 4 * COUT, b4, True, False, 1)       # splits=1: this file's own kernel, unsplit
        ybuf.view(R, H, 2, W, 2, COUT).copy_(s.view(R, H, W, 2, 2, COUT).permute(0, 1, 3, 2, 4, 5))
        return ybuf

    flop = 2.0 * M * CIN * 4 * COUT
    nx, ny, nw = 2 * M * CIN, 2 * 4 * M * COUT, 2 * 4 * COUT * CIN
    prods = {"fwd": (flop, nx + nw + ny, {"deconv": lambda: D.deconv2x2_fwd(x, w_fwd, b, True),
                                          "composed": composed,
                                          "torch": lambda: F.relu(F.conv_transpose2d(x, w16, b16, stride=2))})}
    if train:
        # what autograd runs for the layer: its input gradient is the stride-2 conv2d with the same weight, its weight
        # gradient that conv's weight gradient with the roles of input and cotangent swapped, plus the bias sum
        prods["dgrad"] = (flop, ny + nw + nx, {
            "deconv": lambda: D.deconv2x2_dgrad(g, w_dgrad),
            "torch": lambda: F.conv2d(g, w16, None, stride=2)})
        prods["wgrad"] = (flop, nx + ny + 4 * 4 * COUT * CIN, {
            "deconv": lambda: D.deconv2x2_wgrad(x, g, dw=dw, dbias=db),
            "torch": lambda: (torch.nn.grad.conv2d_weight(g, (CIN, COUT, 2, 2), x, stride=2), g.sum((0, 2, 3)))})
    return prods


def head_arms(R, dtype, train):
    import torch_detection_amd as T
    from torch_detection_amd import functional
    gen = torch.Generator().manual_seed(R)
    x = torch.randn(R, CIN, H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
    gz = torch.randn(R, 81, 2 * H, 2 * W, generator=gen).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
    torch.manual_seed(0)
    head = T.FCNMaskHead().cuda()
    functional.REPACK_IN_CAPTURE = False     # time the layers: the fp32 -> 16-bit repack of a captured step is not part of either arm
    convs = [torch.nn.Conv2d(CIN, CIN, 3, padding=1) for _ in range(4)]
    ref = torch.nn.ModuleList(convs + [torch.nn.ConvTranspose2d(CIN, COUT, 2, stride=2), torch.nn.Conv2d(COUT, 81, 1)])
    ref = ref.cuda().to(dtype).to(memory_format=torch.channels_last)

    def ref_fwd(xi):
        h = xi
        for c in ref[:5]:
            h = F.relu(c(h))
        return ref[5](h)

    def ours():
        if not train:
            with torch.no_grad():
                return head(x)
        xi = x.detach().requires_grad_(True)
        head(xi).backward(gz)

    def theirs():
        if not train:
            with torch.no_grad():
                return ref_fwd(x)
        xi = x.detach().requires_grad_(True)
        ref_fwd(xi).backward(gz)

    M = R * H * W
    flop = 2.0 * M * (4 * 9 * CIN * CIN + CIN * 4 * COUT + 4 * COUT * 81) * (3 if train else 1)
    return flop, {"head": ours, "torch": theirs}


def run_step(R, dtype, train, args):
    from torch_detection_amd import deconv_ops as D
    dn = str(dtype).replace("torch.", "")
    for prod, (flop, nbytes, arms) in products(R, dtype, train).items():
        us = measure(arms, args.inner, args.iters, args.repeats)
        pl = D.deconv2x2_plan({"fwd": 0, "dgrad": 1, "wgrad": 2}[prod], R, H, W, CIN, COUT)
        emit({"layer": "upsample", "product": prod, "dtype": dn, "R": R, "M": R * H * W, "Cin": CIN, "Cout": COUT,
              "us_median_min_max": us, "gflop": round(flop / 1e9, 2), "mbytes": round(nbytes / 1e6, 2),
              "tflops": {k: (round(per(flop, v) / 1e12, 1) if isinstance(v, list) else None) for k, v in us.items()},
              "share_of_copy_rate": {k: (round(per(nbytes, v) / COPY_RATE, 3) if isinstance(v, list) else None)
                                     for k, v in us.items()},
              "tiles": pl.tiles, "slices": pl.slices, "workgroups": pl.workgroups, "launches": pl.launches,
              "inner": args.inner, "iters": args.iters, "repeats": args.repeats}, args.out)
    flop, arms = head_arms(R, dtype, train)
    us = measure(arms, 1, args.iters, args.repeats)
    emit({"layer": "FCNMaskHead", "product": "fwd+bwd" if train else "fwd", "dtype": dn, "R": R,
          "us_median_min_max": us, "gflop": round(flop / 1e9, 2),
          "tflops": {k: (round(per(flop, v) / 1e12, 1) if isinstance(v, list) else None) for k, v in us.items()},
          "inner": 1, "iters": args.iters, "repeats": args.repeats}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds granted to each (dtype, R) step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deconv_bench.jsonl"))
    ap.add_argument("--step", default=None, help="internal: 'dtype,R,train' — run this one step in this process")
    args = ap.parse_args()
    if args.step:
        dn, R, train = args.step.split(",")
        run_step(int(R), getattr(torch, dn), train == "1", args)
        return 0
    for dn in ("bfloat16", "float16"):
        for R, train in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s,%d,%d" % (dn, R, train), "--inner",
                   str(args.inner), "--iters", str(args.iters), "--repeats", str(args.repeats), "--out", args.out]
            try:
                rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print("step %s R=%d ended with status %d: stopping" % (dn, R, rc), file=sys.stderr)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
