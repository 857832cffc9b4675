#!/usr/bin/env python
"""The RPN head's pyramid-wide predictors (csrc/dense_head.hip) at the workload pyramid — B = 2, levels
200x336, 100x168, 50x84, 25x42, 13x21, C = 256, A = 3 — each product timed three ways on the same tensors:

  (a) ``pred``: the one launch (weight gradient: two) of this kernel family over all five levels;
  (b) ``composed``: the same product built from the ``linear_*`` kernels level by level, with everything that route
      needs: forward — ``linear_fwd`` into a stacked (M, 15) buffer and the two slicing copies; input gradient — the
      stacking copy of the two cotangents, ``linear_dgrad`` (its pad launch inside) and the ReLU mask as
      ``add_relu_mask``; weight gradient — the stacking copy and ``linear_wgrad`` chained with beta = 1 over the levels.
      ``composed_fused_mask`` is the input gradient with the mask folded into ``linear_dgrad`` (``mask_src``) instead;
  (c) ``torch``: ``F.conv2d`` per level and predictor (forward), matmuls on the row matrices (gradients).

``share_of_copy_rate``: the bytes the product has to move (operands read once, results written once) over its time, as a
fraction of the 6.29 TB/s float4 copy rate.  It also times the whole ``RPNHead``, forward and forward + backward, beside
the same layers in torch.

Method (scripts/deconv_bench.py): every arm is captured as a graph of ``--inner`` calls and replayed; device events after
warm-up; the arms of one product are alternated inside each of ``--repeats`` windows; median, min and max are reported.
Every dtype runs in a child process of its own under its own time limit; the first that fails or times out ends the
run.  Prints one JSON object per measurement and appends it to ``--out``."""
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
B, C, A = 2, 256, 3
SIZES = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
CL = torch.channels_last


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


def products(dtype):
    """{product: (bytes, {arm: fn})} of the predictors over the workload pyramid."""
    from torch_detection_amd import dense_ops as D, linear_ops as L, ops
    gen = torch.Generator().manual_seed(1)
    O = 5 * A
    hs = [torch.randn(B, H, W, C, generator=gen).clamp_(min=0).cuda().to(dtype).permute(0, 3, 1, 2) for H, W in SIZES]
    gc = [torch.randn(B, H, W, A, generator=gen).cuda().to(dtype).permute(0, 3, 1, 2) for H, W in SIZES]
    gr = [torch.randn(B, H, W, 4 * A, generator=gen).cuda().to(dtype).permute(0, 3, 1, 2) for H, W in SIZES]
    wc = (torch.randn(A, C, 1, 1, generator=gen) / C ** 0.5).cuda()
    wr = (torch.randn(4 * A, C, 1, 1, generator=gen) / C ** 0.5).cuda()
    bc, br = torch.randn(A, generator=gen).cuda(), torch.randn(4 * A, generator=gen).cuda()
    w_fwd, w_dgrad = D.pack_pred_weight(wc, wr, True, dtype)
    ws = torch.cat([wc.view(A, C), wr.view(4 * A, C)])
    bs = torch.cat([bc, br])
    l_fwd, l_dgrad = L.pack_linear_weight(ws, None, True, dtype)
    h2 = [h.permute(0, 2, 3, 1).reshape(-1, C) for h in hs]
    h4 = [h.permute(0, 2, 3, 1) for h in hs]
    gc2 = [g.permute(0, 2, 3, 1).reshape(-1, A) for g in gc]
    gr2 = [g.permute(0, 2, 3, 1).reshape(-1, 4 * A) for g in gr]
    wc16, wr16, bc16, br16 = wc.to(dtype), wr.to(dtype), bc.to(dtype), br.to(dtype)
    wc2, wr2 = wc16.view(A, C), wr16.view(4 * A, C)
    dw, db = torch.empty(O, C, device="cuda"), torch.empty(O, device="cuda")

    def composed_fwd():
        out = []
        for x in h2:
            y = L.linear_fwd(x, l_fwd, O, bs)
            out.append((y[:, :A].contiguous(), y[:, A:].contiguous()))
        return out

    def composed_dgrad(fused):
        out = []
        for x, x4, a, b in zip(h2, h4, gc2, gr2):
            g = torch.cat([a, b], 1)
            if fused:
                out.append(L.linear_dgrad(g, l_dgrad, mask_src=x))
            else:
                dx = L.linear_dgrad(g, l_dgrad)
                out.append(ops.add_relu_mask(dx.view(x4.shape), None, x4))
        return out

    def composed_wgrad():
        for l, (x, a, b) in enumerate(zip(h2, gc2, gr2)):
            L.linear_wgrad(x, torch.cat([a, b], 1), dw=dw, dbias=db, beta=1.0 if l else 0.0)
        return dw[:A], db[:A], dw[A:], db[A:]

    def torch_wgrad():
        dc = dr = sc = sr = None
        for x, a, b in zip(h2, gc2, gr2):
            tc, tr, uc, ur = a.T @ x, b.T @ x, a.sum(0), b.sum(0)
            dc, dr = (tc, tr) if dc is None else (dc + tc, dr + tr)
            sc, sr = (uc, ur) if sc is None else (sc + uc, sr + ur)
        return dc, dr, sc, sr

    rows = sum(B * H * W for H, W in SIZES)
    nw = 2 * O * C
    slab = D.pred_plan(D.WGRAD, [B * H * W for H, W in SIZES], C, A).workspace_bytes
    return rows, {
        "fwd": (rows * (2 * C + 2 * O) + nw, {
            "pred": lambda: D.pred_fwd(hs, w_fwd, bc, br),
            "composed": composed_fwd,
            "torch": lambda: [(F.conv2d(h, wc16, bc16), F.conv2d(h, wr16, br16)) for h in hs]}),
        "dgrad": (rows * (4 * C + 2 * O) + nw, {
            "pred": lambda: D.pred_dgrad(gc, gr, w_dgrad, hs),
            "composed": lambda: composed_dgrad(False),
            "composed_fused_mask": lambda: composed_dgrad(True),
            "torch": lambda: [(a @ wc2 + b @ wr2) * (x > 0) for x, a, b in zip(h2, gc2, gr2)]}),
        "wgrad": (rows * (2 * C + 2 * O) + 2 * slab + 4 * O * C, {
            "pred": lambda: D.pred_wgrad(hs, gc, gr),
            "composed": composed_wgrad,
            "torch": torch_wgrad}),
    }


def head_arms(dtype, train):
    import torch_detection_amd as T
    from torch_detection_amd import functional
    gen = torch.Generator().manual_seed(2)
    xs = [torch.randn(B, C, H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=CL) for H, W in SIZES]
    gc = [torch.randn(B, A, H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=CL) for H, W in SIZES]
    gr = [torch.randn(B, 4 * A, H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=CL) for H, W in SIZES]
    torch.manual_seed(0)
    head = T.RPNHead(C, C).cuda()
    functional.REPACK_IN_CAPTURE = False     # time the layers: the fp32 -> 16-bit repack of a captured step is not part of either arm
    ref = torch.nn.ModuleList([torch.nn.Conv2d(C, C, 3, padding=1), torch.nn.Conv2d(C, A, 1), torch.nn.Conv2d(C, 4 * A, 1)])
    ref = ref.cuda().to(dtype).to(memory_format=CL)

    def ref_fwd(feats):
        hs = [F.relu(ref[0](x)) for x in feats]
        return [ref[1](h) for h in hs] + [ref[2](h) for h in hs]

    def ours():
        if not train:
            with torch.no_grad():
                return head(xs)
        feats = [x.detach().requires_grad_(True) for x in xs]
        cls, reg = head(feats)
        torch.autograd.backward(cls + reg, gc + gr)

    def theirs():
        if not train:
            with torch.no_grad():
                return ref_fwd(xs)
        feats = [x.detach().requires_grad_(True) for x in xs]
        torch.autograd.backward(ref_fwd(feats), gc + gr)

    return {"head": ours, "torch": theirs}


def run_step(dtype, args):
    from torch_detection_amd import dense_ops as D
    dn = str(dtype).replace("torch.", "")
    rows, prods = products(dtype)
    level_rows = [B * H * W for H, W in SIZES]
    for prod, (nbytes, arms) in prods.items():
        us = measure(arms, args.inner, args.iters, args.repeats)
        pl = D.pred_plan({"fwd": 0, "dgrad": 1, "wgrad": 2}[prod], level_rows, C, A)
        faster = None
        if isinstance(us.get("pred"), list) and isinstance(us.get("composed"), list):
            faster = us["pred"][2] < us["composed"][1]          # the slowest repeat below the composed form's fastest
        emit({"layer": "rpn predictors", "product": prod, "dtype": dn, "B": B, "levels": SIZES, "rows": rows, "C": C,
              "A": A, "us_median_min_max": us, "mbytes": round(nbytes / 1e6, 2),
              "share_of_copy_rate": {k: (round(nbytes / (v[0] * 1e-6) / COPY_RATE, 3) if isinstance(v, list) else None)
                                     for k, v in us.items()},
              "pred_slowest_below_composed_fastest": faster,
              "workgroups": pl.workgroups, "slices": pl.slices, "launches": pl.launches,
              "inner": args.inner, "iters": args.iters, "repeats": args.repeats}, args.out)
    for train in (False, True):
        us = measure(head_arms(dtype, train), 1, args.iters, args.repeats)
        emit({"layer": "RPNHead", "product": "fwd+bwd" if train else "fwd", "dtype": dn, "B": B, "levels": SIZES,
              "C": C, "A": A, "us_median_min_max": us, "inner": 1, "iters": args.iters, "repeats": args.repeats},
             args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds granted to each dtype")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_head_bench.jsonl"))
    ap.add_argument("--step", default=None, help="internal: the dtype to run in this process")
    args = ap.parse_args()
    if args.step:
        run_step(getattr(torch, args.step), args)
        return 0
    for dn in ("bfloat16", "float16"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", dn, "--inner", str(args.inner), "--iters",
               str(args.iters), "--repeats", str(args.repeats), "--out", args.out]
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("step %s ended with status %d: stopping" % (dn, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
