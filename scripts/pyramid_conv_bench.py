#!/usr/bin/env python
"""The shared-weight 3x3 conv over a pyramid (csrc/pyramid_conv.hip) at RetinaNet's workload pyramid —
B = 2, levels 100x168, 50x84, 25x42, 13x21, 7x11 (44 800 pixels), Cin = 256 — for the three Cout classes of the head
(tower 256, cls 720, reg 36), each product timed on the same tensors as

  (a) ``pyramid``: the one launch (weight gradient: two) of this kernel family over all five levels;
  (b) ``composed``: the same product from the existing conv units level by level — exactly what ``RetinaHead`` runs on its
      composed route (``heads._Layer``): for a predictor the weight zero padded to the next multiple of 64 and the slicing
      copy per level (forward), the pad copy per cotangent (input gradient; the weight gradient arm reuses that copy, as
      the backward pass does, so it is NOT charged for it), the weight gradients on one shared ``WgradQueue`` and the fp32
      level sum;
  (c) ``split``: ``RetinaHead``'s split route — the levels of at least ``heads.SPLIT_PIXELS`` pixels (here levels 0 and 1)
      as in (b), the three tail levels in one launch of (a) — forward and input gradient only;
  (d) ``torch``: ``F.conv2d`` / ``conv2d_input`` / ``conv2d_weight`` per level on 16-bit channels_last tensors.

It also times the whole ``RetinaHead`` (80 classes, 9 anchors), forward and forward + backward, on its default route, on
the all-composed and the all-pyramid route, beside the same layers in torch.

Method (scripts/dense_head_bench.py): every arm is captured as a graph of ``--inner`` calls and replayed; device events
after warm-up; the arms of one product are alternated inside each of ``--repeats`` windows; median, min and max are
reported.  Every dtype runs in a child process of its own under its own time limit; the first that fails or times out
ends the run.  Prints one JSON object per measurement and appends it to ``--out``."""
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

B, C, NUM_CLASSES = 2, 256, 81
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
CL = torch.channels_last
PRODUCTS = ("fwd", "dgrad", "wgrad")
PEAK_FLOPS, COPY_RATE = 2.5e15, 6.29e12


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


def routes_of(route):
    return {k: {p: route for p in PRODUCTS} for k in ("tower", "cls", "reg")}


def make_head(route=None):
    import torch_detection_amd as T
    torch.manual_seed(0)
    head = T.RetinaHead(NUM_CLASSES, C).cuda()
    if route is not None:
        head._routes = routes_of(route)
    return head


def products(dtype):
    """{(class, product): (Cout, {arm: fn})} over the workload pyramid."""
    from torch_detection_amd import functional as HF
    gen = torch.Generator().manual_seed(1)
    mk = lambda ch, relu=False: [
        (torch.randn(B, H, W, ch, generator=gen).clamp_(min=0) if relu else torch.randn(B, H, W, ch, generator=gen))
        .cuda().to(dtype).permute(0, 3, 1, 2) for H, W in SIZES]
    xs = mk(C, True)                                       # a ReLU's output: the input and the mask source
    hp, hc, hs = make_head("pyramid"), make_head("composed"), make_head("split")
    with torch.no_grad():
        for p, q, r in zip(hp.parameters(), hc.parameters(), hs.parameters()):
            if p.dim() == 4:
                p.mul_(4.0)                                # outputs and gradients of ordinary size
            q.copy_(p)
            r.copy_(p)
    chains = [h._chains(dtype) for h in (hp, hc, hs)]
    layers = {"tower": [c[0][1] for c in chains], "cls": [c[0][-1] for c in chains], "reg": [c[1][-1] for c in chains]}
    dev = xs[0].device
    out = {}
    for kind, (lp, lc, ls) in layers.items():
        Cout = lp.Cout
        gs = mk(Cout)
        w16 = lp.weight.detach().to(dtype).contiguous(memory_format=CL)
        b16 = lp.bias.detach().to(dtype)
        relu = lp.relu

        def wgrad_of(layer, xs=xs, gs=gs):
            wq = HF.WgradQueue(dev)
            t = layer.wgrad(xs, gs, wq)
            wq.flush()
            HF.join_side_stream(dev)
            return t()

        def dgrad_padded(layer, gs=gs):
            layer._pads.clear()                            # the pad copy of the cotangents belongs to this product
            return layer.dgrad(gs, mask_src=xs)

        def torch_fwd(w16=w16, b16=b16, relu=relu):
            ys = [F.conv2d(x, w16, b16, 1, 1) for x in xs]
            return [F.relu(y) for y in ys] if relu else ys

        def torch_dgrad(w16=w16, gs=gs):
            return [torch.nn.grad.conv2d_input(x.shape, w16, g, 1, 1) * (x > 0) for x, g in zip(xs, gs)]

        def torch_wgrad(w16=w16, gs=gs):
            dw = db = None
            for x, g in zip(xs, gs):
                tw, tb = torch.nn.grad.conv2d_weight(x, w16.shape, g, 1, 1), g.sum((0, 2, 3))
                dw, db = (tw, tb) if dw is None else (dw + tw, db + tb)
            return dw, db

        def wgrad_composed(lc=lc, wgrad_of=wgrad_of, state={}):
            if not state:                                  # the first (eager) call pads the cotangents once; the
                lc._pads.clear()                           # captured calls reuse that copy, as the backward pass does
                state["padded"] = True
            return wgrad_of(lc)

        out[(kind, "fwd")] = (Cout, {
            "pyramid": lambda lp=lp: lp.fwd(xs),
            "composed": lambda lc=lc: lc.fwd(xs),
            "split": lambda ls=ls: ls.fwd(xs),
            "torch": torch_fwd})
        out[(kind, "dgrad")] = (Cout, {
            "pyramid": lambda lp=lp, gs=gs: lp.dgrad(gs, mask_src=xs),
            "composed": lambda lc=lc, f=dgrad_padded: f(lc),
            "split": lambda ls=ls, f=dgrad_padded: f(ls),
            "torch": torch_dgrad})
        out[(kind, "wgrad")] = (Cout, {
            "pyramid": lambda lp=lp, wgrad_of=wgrad_of: wgrad_of(lp),
            "composed": wgrad_composed,
            "torch": torch_wgrad})
    return out


def head_arms(dtype, train):
    from torch_detection_amd import functional
    gen = torch.Generator().manual_seed(2)
    A = 9
    xs = [torch.randn(B, C, H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=CL) for H, W in SIZES]
    gc = [torch.randn(B, A * (NUM_CLASSES - 1), H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=CL)
          for H, W in SIZES]
    gr = [torch.randn(B, 4 * A, H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=CL) for H, W in SIZES]
    heads = {"head": make_head(), "head_composed": make_head("composed"), "head_pyramid": make_head("pyramid")}
    functional.REPACK_IN_CAPTURE = False     # time the layers: the fp32 -> 16-bit repack of a captured step is not part of any arm
    conv = lambda i, o: torch.nn.Conv2d(i, o, 3, padding=1)
    ref = torch.nn.ModuleList([conv(C, C) for _ in range(8)] + [conv(C, A * (NUM_CLASSES - 1)), conv(C, 4 * A)])
    ref = ref.cuda().to(dtype).to(memory_format=CL)

    def ref_fwd(feats):
        cls, reg = [], []
        for x in feats:
            c = r = x
            for i in range(4):
                c, r = F.relu(ref[i](c)), F.relu(ref[4 + i](r))
            cls.append(ref[8](c))
            reg.append(ref[9](r))
        return cls + reg

    def ours(head):
        def run():
            if not train:
                with torch.no_grad():
                    return head(xs)
            feats = [x.detach().requires_grad_(True) for x in xs]
            cls, reg = head(feats)
            torch.autograd.backward(cls + reg, gc + gr)
        return run

    def theirs():
        if not train:
            with torch.no_grad():
                return ref_fwd(xs)
        feats = [x.detach().requires_grad_(True) for x in xs]
        torch.autograd.backward(ref_fwd(feats), gc + gr)

    arms = {k: ours(h) for k, h in heads.items()}
    arms["torch"] = theirs
    return arms


def run_step(dtype, args):
    from torch_detection_amd import heads
    from torch_detection_amd import pyramid_ops as P
    dn = str(dtype).replace("torch.", "")
    pixels = sum(B * H * W for H, W in SIZES)
    for (kind, prod), (Cout, arms) in products(dtype).items():
        us = measure(arms, args.inner, args.iters, args.repeats)
        pl = P.pyramid_conv_plan(PRODUCTS.index(prod), B, SIZES, C, Cout)
        flops = 2.0 * pixels * 9 * C * Cout
        nbytes = pixels * 2 * (C + Cout) + 2 * 9 * C * Cout + (pixels * 2 * C if prod == "dgrad" else 0) + \
            (2 * pl.slab_bytes + 4 * 9 * C * Cout if prod == "wgrad" else 0)
        stays = split_below = None
        if isinstance(us.get("pyramid"), list) and isinstance(us.get("composed"), list):
            stays = us["pyramid"][2] < us["composed"][1]        # the slowest repeat below the composed form's fastest
        if isinstance(us.get("split"), list) and isinstance(us.get("composed"), list) and isinstance(us.get("pyramid"), list):
            split_below = us["split"][2] < min(us["composed"][1], us["pyramid"][1])
        emit({"layer": kind, "product": prod, "dtype": dn, "B": B, "levels": SIZES, "pixels": pixels, "Cin": C,
              "Cout": Cout, "us_median_min_max": us, "gflop": round(flops / 1e9, 2), "mbytes": round(nbytes / 1e6, 2),
              "roofline_us": round(max(flops / PEAK_FLOPS, nbytes / COPY_RATE) * 1e6, 1),
              "tflops": {k: (round(flops / (v[0] * 1e-6) / 1e12, 1) if isinstance(v, list) else None)
                         for k, v in us.items()},
              "pyramid_slowest_below_composed_fastest": stays, "split_slowest_below_both_fastest": split_below,
              "default_route": heads.RETINA_ROUTES[kind][prod],
              "workgroups": pl.workgroups, "slices": pl.slices, "launches": pl.launches, "slab_mbytes":
              round(pl.slab_bytes / 1e6, 2), "inner": args.inner, "iters": args.iters, "repeats": args.repeats}, args.out)
    for train in (False, True):
        us = measure(head_arms(dtype, train), 1, args.iters, args.repeats)
        emit({"layer": "RetinaHead", "product": "fwd+bwd" if train else "fwd", "dtype": dn, "B": B, "levels": SIZES,
              "Cin": C, "num_classes": NUM_CLASSES, "default_routes": heads.RETINA_ROUTES, "us_median_min_max": us,
              "inner": 1, "iters": args.iters, "repeats": args.repeats}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds granted to each dtype")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_conv_bench.jsonl"))
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
