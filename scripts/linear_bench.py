#!/usr/bin/env python
"""The fully connected layers of the box head (csrc/linear.hip) beside two arms that are never the code
under test: (a) the same product through the conv entry points as a 1x1 conv with N = 1, H = M, W = 1 — what the parent
commit offers, for the layers whose O is a multiple of 64 (``linear_own_unsplit`` beside it is this file's kernel forced
to stay unsplit and unrouted, ``splits=1``); (b) torch (hipBLASLt): ``F.linear`` forward and the two
matmuls its autograd backward runs (``g @ w`` and ``g.T @ x``), same dtype, on the GPU.

Method (scripts/optim_bench.py): every arm is captured as a graph of ``--inner`` calls and replayed; device events
after warm-up; the arms of one product are alternated inside each of ``--repeats`` windows; the median over the windows
and the spread (min, max) of each arm are reported.  FLOP = 2 M K O per product; the share is of the 2.5 PFLOP/s dense
bf16 MFMA peak.  Prints one JSON object per measurement and appends it to ``--out``."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_detection_amd as T  # noqa: E402
from torch_detection_amd import linear_ops as L, ops  # noqa: E402

PEAK = 2.5e15
LAYERS = [("fc6", 1024, 12544, 256), ("fc7", 1024, 1024, None), ("fc_cls", 81, 1024, None), ("fc_reg", 324, 1024, None)]


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


def tf(flop, us):
    return None if not isinstance(us, list) else round(flop / (us[0] * 1e-6) / 1e12, 1)


def layer_arms(name, O, K, C, M, dtype, train):
    """The products of one layer: {product: (flop, {arm: fn})}."""
    gen = torch.Generator().manual_seed(O + K + M)
    x = torch.randn(M, K, generator=gen).cuda().to(dtype)
    w = (torch.randn(O, K, generator=gen) / K ** 0.5).cuda()
    b = torch.randn(O, generator=gen).cuda()
    g = torch.randn(M, O, generator=gen).cuda().to(dtype)
    w_fwd, w_dgrad = L.pack_linear_weight(w, C, True, dtype)
    dw, db = torch.empty(O, K, device="cuda"), torch.empty(O, device="cuda")
    w16, b16 = w.to(dtype), b.to(dtype)
    relu = name.startswith("fc") and not name.startswith("fc_")
    flop = 2.0 * M * K * O
    prods = {"fwd": (flop, {"linear": lambda: L.linear_fwd(x, w_fwd, O, b, relu),
                            "torch": lambda: F.linear(x, w16, b16)})}
    if train:
        prods["dgrad"] = (flop, {"linear": lambda: L.linear_dgrad(g, w_dgrad, x if relu else None),
                                 "torch": lambda: g @ w16})
        prods["wgrad"] = (flop, {"linear": lambda: L.linear_wgrad(x, g, C, dw=dw, dbias=db),
                                 "torch": lambda: g.t() @ x})
        if C is not None:
            prods["wgrad"][1]["linear_C_eq_K"] = lambda: L.linear_wgrad(x, g, None, dw=dw, dbias=db)
    if O % 64 == 0:
        x4, g4 = x.view(1, M, 1, K), g.view(1, M, 1, O)
        cw_fwd, cw_dgrad = ops.pack_conv_weight(w.view(O, K, 1, 1), None, True, dtype)
        cdw = torch.empty(O, 1, 1, K, device="cuda")
        prods["fwd"][1]["conv1x1"] = lambda: ops.conv2d_fwd(x4, cw_fwd, 1, 1, 0, shift=b, relu=relu)
        # splits=1 keeps the product in csrc/linear.hip's own kernel, unsplit, whatever the library would choose
        prods["fwd"][1]["linear_own_unsplit"] = lambda: L.linear_fwd(x, w_fwd, O, b, relu, False, 1)
        if train:
            prods["dgrad"][1]["linear_own_unsplit"] = lambda: L.linear_dgrad(g, w_dgrad, x if relu else None, 1)
        if train:
            prods["dgrad"][1]["conv1x1"] = lambda: ops.conv2d_dgrad(g4, cw_dgrad, (M, 1), 1, 1, 0,
                                                                    mask_src=x4 if relu else None)
            prods["wgrad"][1]["conv1x1"] = lambda: ops.conv2d_wgrad(x4, g4, cw_fwd, 1, 1, 0, dw=cdw, dbeta=db)
    return prods


def head_arms(M, dtype, train):
    gen = torch.Generator().manual_seed(M)
    x = torch.randn(M, 256, 7, 7, generator=gen).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
    gc = torch.randn(M, 81, generator=gen).cuda().to(dtype)
    gr = torch.randn(M, 324, generator=gen).cuda().to(dtype)
    torch.manual_seed(0)
    head = T.BBoxHead().cuda()
    from torch_detection_amd import functional
    functional.REPACK_IN_CAPTURE = False     # time the products: the fp32 -> 16-bit repack of a captured step is not part of either arm
    ref = torch.nn.ModuleList([torch.nn.Linear(12544, 1024), torch.nn.Linear(1024, 1024), torch.nn.Linear(1024, 81),
                               torch.nn.Linear(1024, 324)]).cuda().to(dtype)
    xr = x.contiguous().view(M, -1)

    def ours():
        if not train:
            with torch.no_grad():
                return head(x)
        xi = x.detach().requires_grad_(True)
        cls, reg = head(xi)
        torch.autograd.backward([cls, reg], [gc, gr])

    def theirs():
        if not train:
            with torch.no_grad():
                h = F.relu(ref[1](F.relu(ref[0](xr))))
                return ref[2](h), ref[3](h)
        xi = xr.detach().requires_grad_(True)
        h = F.relu(ref[1](F.relu(ref[0](xi))))
        torch.autograd.backward([ref[2](h), ref[3](h)], [gc, gr])

    flop = 2.0 * M * (12544 * 1024 + 1024 * 1024 + 405 * 1024) * (3 if train else 1)
    return flop, {"linear": ours, "torch": theirs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_bench.jsonl"))
    args = ap.parse_args()
    for dtype in (torch.bfloat16, torch.float16):
        dn = str(dtype).replace("torch.", "")
        for M, train in ((1024, True), (2048, True), (2000, False)):
            for name, O, K, C in LAYERS:
                for prod, (flop, arms) in layer_arms(name, O, K, C, M, dtype, train).items():
                    us = measure(arms, args.inner, args.iters, args.repeats)
                    pl = L.linear_plan({"fwd": 0, "dgrad": 1, "wgrad": 2}[prod], M, O, K)
                    emit({"layer": name, "product": prod, "dtype": dn, "M": M, "O": O, "K": K, "C": C,
                          "us_median_min_max": us, "gflop": round(flop / 1e9, 2),
                          "tflops": {k: tf(flop, v) for k, v in us.items()},
                          "share_of_bf16_peak": {k: (round(flop / (v[0] * 1e-6) / PEAK, 3) if isinstance(v, list) else None)
                                                 for k, v in us.items()},
                          "routed_to_conv": bool(pl.conv), "tiles": pl.tiles, "slices": pl.slices, "workgroups": pl.workgroups, "launches": pl.launches,
                          "inner": args.inner, "iters": args.iters, "repeats": args.repeats}, args.out)
            flop, arms = head_arms(M, dtype, train)
            us = measure(arms, 1, args.iters, args.repeats)
            emit({"layer": "head", "product": "fwd+bwd" if train else "fwd", "dtype": dn, "M": M,
                  "us_median_min_max": us, "gflop": round(flop / 1e9, 2), "tflops": {k: tf(flop, v) for k, v in us.items()},
                  "inner": 1, "iters": args.iters, "repeats": args.repeats}, args.out)


if __name__ == "__main__":
    main()
