#!/usr/bin/env python
"""GroupNorm (+ ReLU) with shared affine parameters over a pyramid (csrc/pyramid_gn.hip) at the FCOS
workload pyramid — B = 2, levels 100x168, 50x84, 25x42, 13x21, 7x11 (44 800 pixels), C = 256, 32 groups — forward and
backward, each timed on the same tensors as

  (a) ``pyramid``: the three launches of this kernel family over all five levels;
  (b) ``composed``: exactly what ``FCOSHead`` runs on its composed route (``heads._GnLayer``): ``ops.gn_fwd`` per level;
      ``ops.act_mask`` + ``ops.gn_bwd`` per level, dgamma / dbeta accumulated in level order;
  (c) ``torch``: ``F.group_norm`` + ``F.relu`` per level on 16-bit channels_last tensors, and its autograd.

The three predictor products whose Cout §4m did not time (``fcos_cls`` 80, ``fcos_reg`` 4, ``fcos_centerness`` 1) are
timed as in scripts/pyramid_conv_bench.py: ``pyramid`` / ``composed`` / ``split`` (forward and input gradient),
``pyramid`` / ``composed`` (weight gradient).  Then the whole ``FCOSHead`` (80 classes), forward and forward + backward:
its default routes, all composed, and the same layers in torch.

Method (scripts/pyramid_conv_bench.py): every arm is captured as a graph of ``--inner`` calls and replayed; device events
after warm-up; the arms of one product are alternated inside each of ``--repeats`` windows; median, min and max are
reported.  Every dtype runs in a child process of its own under its own time limit; the first that fails or times out
ends the run.  Prints one JSON object per measurement and appends it to ``--out``."""
import argparse
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from pyramid_conv_bench import CL, COPY_RATE, PEAK_FLOPS, SIZES, B, C, emit, measure  # noqa: E402

NUM_CLASSES, GROUPS = 81, 32
PRODUCTS = ("fwd", "dgrad", "wgrad")
PRED_KINDS = ("cls", "reg", "ctr")


def routes_of(route):
    from torch_detection_amd import heads
    r = {k: {p: route for p in PRODUCTS} for k in ("tower",) + PRED_KINDS}
    if route == heads.SPLIT:
        for k in r:
            r[k]["wgrad"] = heads.COMPOSED
    gn = heads.PYRAMID if route == heads.PYRAMID else heads.COMPOSED
    r["gn"] = {"fwd": gn, "bwd": gn}
    return r


def make_head(route=None):
    import torch_detection_amd as T
    torch.manual_seed(0)
    head = T.FCOSHead(NUM_CLASSES, C).cuda()
    if route is not None:
        head._routes = routes_of(route)
    return head


def maps(gen, ch, dtype, relu=False):
    return [(torch.randn(B, H, W, ch, generator=gen).clamp_(min=0) if relu else torch.randn(B, H, W, ch, generator=gen))
            .cuda().to(dtype).permute(0, 3, 1, 2) for H, W in SIZES]


def gn_products(dtype):
    """{product: {arm: fn}} of one tower layer's GroupNorm + ReLU over the workload pyramid."""
    from torch_detection_amd import heads
    gen = torch.Generator().manual_seed(3)
    zs, gs = maps(gen, C, dtype), maps(gen, C, dtype)
    norm = torch.nn.GroupNorm(GROUPS, C).cuda()
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.5, 0.5)
    holder = lambda r: type("H", (), {"_routes": {"gn": {"fwd": r, "bwd": r}}})()
    lp, lc = heads._GnLayer(holder(heads.PYRAMID), norm, False), heads._GnLayer(holder(heads.COMPOSED), norm, False)
    yp, sp = lp.fwd(zs)
    yc, sc = lc.fwd(zs)
    w16, b16 = norm.weight.detach().to(dtype), norm.bias.detach().to(dtype)
    saved = []

    def torch_fwd():
        with torch.no_grad():
            return [F.relu(F.group_norm(z, GROUPS, w16, b16, norm.eps)) for z in zs]

    def torch_bwd():
        # The two backward functions autograd runs for relu and group_norm, called directly on the current stream (the
        # autograd engine itself would run them on the stream of a forward made outside the capture), on what autograd
        # saves: F.group_norm hands native_group_norm an NCHW-contiguous copy of a channels_last input on this device, and
        # the cotangent is made contiguous in the same way.
        with torch.no_grad():
            if not saved:                                  # the first (eager) call: the forward's saved tensors
                for z in zs:
                    zc = z.contiguous()
                    pre, mean, rstd = torch.native_group_norm(zc, w16, b16, B, C, z.shape[2] * z.shape[3], GROUPS, norm.eps)
                    saved.append((zc, torch.relu(pre), mean, rstd))
            dzs, dw, db = [], None, None
            for g, (zc, y, mean, rstd) in zip(gs, saved):
                gm = torch.ops.aten.threshold_backward(g, y, 0).contiguous()
                dz, tw, tb = torch.ops.aten.native_group_norm_backward(gm, zc, mean, rstd, w16, B, C, zc.shape[2] * zc.shape[3],
                                                                       GROUPS, [True, True, True])
                dzs.append(dz)
                dw, db = (tw, tb) if dw is None else (dw + tw, db + tb)
            return dzs, dw, db

    return {"fwd": {"pyramid": lambda: lp.fwd(zs), "composed": lambda: lc.fwd(zs), "torch": torch_fwd},
            "bwd": {"pyramid": lambda: lp.bwd(gs, yp, zs, sp), "composed": lambda: lc.bwd(gs, yc, zs, sc),
                    "torch": torch_bwd}}


def pred_products(dtype):
    """{(kind, product): (Cout, {arm: fn})}: the three predictors over the workload pyramid."""
    from torch_detection_amd import functional as HF
    gen = torch.Generator().manual_seed(1)
    xs = maps(gen, C, dtype, True)
    hp, hc, hs = make_head("pyramid"), make_head("composed"), make_head("split")
    with torch.no_grad():
        for p, q, r in zip(hp.parameters(), hc.parameters(), hs.parameters()):
            if p.dim() == 4:
                p.mul_(4.0)
            q.copy_(p)
            r.copy_(p)
    preds = [h._chains(dtype)[1] for h in (hp, hc, hs)]
    dev = xs[0].device
    out = {}
    for i, kind in enumerate(PRED_KINDS):
        lp, lc, ls = (p[i] for p in preds)
        Cout = lp.Cout
        gs = maps(gen, Cout, dtype)

        def wgrad_of(layer, gs=gs):
            wq = HF.WgradQueue(dev)
            t = layer.wgrad(xs, gs, wq)
            wq.flush()
            HF.join_side_stream(dev)
            return t()

        def dgrad_padded(layer, gs=gs):
            layer._pads.clear()                            # the pad copy of the cotangents belongs to this product
            return layer.dgrad(gs)                         # unmasked: a GroupNorm layer lies below

        def wgrad_composed(lc=lc, wgrad_of=wgrad_of, state={}):
            if not state:                                  # the first (eager) call pads the cotangents once; the
                lc._pads.clear()                           # captured calls reuse that copy, as the backward pass does
                state["padded"] = True
            return wgrad_of(lc)

        out[(kind, "fwd")] = (Cout, {"pyramid": lambda lp=lp: lp.fwd(xs), "composed": lambda lc=lc: lc.fwd(xs),
                                     "split": lambda ls=ls: ls.fwd(xs)})
        out[(kind, "dgrad")] = (Cout, {"pyramid": lambda lp=lp, gs=gs: lp.dgrad(gs),
                                       "composed": lambda lc=lc, f=dgrad_padded: f(lc),
                                       "split": lambda ls=ls, f=dgrad_padded: f(ls)})
        out[(kind, "wgrad")] = (Cout, {"pyramid": lambda lp=lp, f=wgrad_of: f(lp), "composed": wgrad_composed})
    return out


def head_arms(dtype, train):
    from torch_detection_amd import functional
    gen = torch.Generator().manual_seed(2)
    mk = lambda ch: [torch.randn(B, ch, H, W, generator=gen).cuda().to(dtype).contiguous(memory_format=CL)
                     for H, W in SIZES]
    xs, gc, gr, gt = mk(C), mk(NUM_CLASSES - 1), mk(4), mk(1)
    heads = {"head": make_head(), "head_composed": make_head("composed")}
    functional.REPACK_IN_CAPTURE = False     # time the layers: the fp32 -> 16-bit repack of a captured step is not part of any arm
    conv = lambda i, o, bias: torch.nn.Conv2d(i, o, 3, padding=1, bias=bias)
    ref = torch.nn.ModuleList([conv(C, C, False) for _ in range(8)] + [torch.nn.GroupNorm(GROUPS, C) for _ in range(8)] +
                              [conv(C, NUM_CLASSES - 1, True), conv(C, 4, True), conv(C, 1, True)])
    ref = ref.cuda().to(dtype).to(memory_format=CL)

    def ref_fwd(feats):
        cls, reg, ctr = [], [], []
        for x in feats:
            c = r = x
            for i in range(4):
                c, r = F.relu(ref[8 + i](ref[i](c))), F.relu(ref[12 + i](ref[4 + i](r)))
            cls.append(ref[16](c))
            reg.append(ref[17](r))
            ctr.append(ref[18](c))
        return cls + reg + ctr

    def ours(head):
        def run():
            if not train:
                with torch.no_grad():
                    return head(xs)
            feats = [x.detach().requires_grad_(True) for x in xs]
            cls, reg, ctr = head(feats)
            torch.autograd.backward(cls + reg + ctr, gc + gr + gt)
        return run

    def theirs():
        if not train:
            with torch.no_grad():
                return ref_fwd(xs)
        feats = [x.detach().requires_grad_(True) for x in xs]
        torch.autograd.backward(ref_fwd(feats), gc + gr + gt)

    arms = {k: ours(h) for k, h in heads.items()}
    arms["torch"] = theirs
    return arms


def run_step(dtype, args):
    from torch_detection_amd import heads
    from torch_detection_amd import pyramid_ops as P
    dn = str(dtype).replace("torch.", "")
    pixels = sum(B * H * W for H, W in SIZES)
    common = {"dtype": dn, "B": B, "levels": SIZES, "pixels": pixels, "inner": args.inner, "iters": args.iters,
              "repeats": args.repeats}
    for prod, arms in gn_products(dtype).items():
        us = measure(arms, args.inner, args.iters, args.repeats)
        pl = P.pyramid_gn_plan(P.GN_FWD if prod == "fwd" else P.GN_BWD, B, SIZES, C, GROUPS)
        # forward: z read twice, y written; backward: g, y, z read twice, dz written — 16-bit maps
        nbytes = pixels * C * 2 * (3 if prod == "fwd" else 7)
        stays = None
        if isinstance(us.get("pyramid"), list) and isinstance(us.get("composed"), list):
            stays = us["pyramid"][2] < us["composed"][1]        # the slowest repeat below the composed form's fastest
        line = {"layer": "gn", "product": prod, "C": C, "groups": GROUPS, "us_median_min_max": us,
                "mbytes": round(nbytes / 1e6, 2), "byte_bound_us": round(nbytes / COPY_RATE * 1e6, 1),
                "pyramid_fraction_of_copy_rate": (round(nbytes / COPY_RATE * 1e6 / us["pyramid"][0], 3)
                                                  if isinstance(us.get("pyramid"), list) else None),
                "pyramid_slowest_below_composed_fastest": stays,
                "default_route": heads.FCOS_ROUTES["gn"]["fwd" if prod == "fwd" else "bwd"],
                "launches": {"pyramid": pl.launches, "composed": len(SIZES) * (3 if prod == "fwd" else 4)},
                "workgroups": list(pl.workgroups), "chunks": pl.chunks, "workspace_bytes": pl.workspace_bytes}
        line.update(common)
        emit(line, args.out)
    for (kind, prod), (Cout, arms) in pred_products(dtype).items():
        us = measure(arms, args.inner, args.iters, args.repeats)
        pl = P.pyramid_conv_plan(PRODUCTS.index(prod), B, SIZES, C, Cout)
        flops = 2.0 * pixels * 9 * C * Cout
        nbytes = pixels * 2 * (C + Cout) + 2 * 9 * C * Cout + (2 * pl.slab_bytes + 4 * 9 * C * Cout if prod == "wgrad" else 0)
        ok = lambda k: isinstance(us.get(k), list)
        stays = us["pyramid"][2] < us["composed"][1] if ok("pyramid") and ok("composed") else None
        split_below = (us["split"][2] < min(us["composed"][1], us["pyramid"][1])
                       if ok("split") and ok("composed") and ok("pyramid") else None)
        line = {"layer": kind, "product": prod, "Cin": C, "Cout": Cout, "us_median_min_max": us,
                "gflop": round(flops / 1e9, 2), "mbytes": round(nbytes / 1e6, 2),
                "roofline_us": round(max(flops / PEAK_FLOPS, nbytes / COPY_RATE) * 1e6, 1),
                "pyramid_slowest_below_composed_fastest": stays, "split_slowest_below_both_fastest": split_below,
                "default_route": heads.FCOS_ROUTES[kind][prod], "workgroups": pl.workgroups, "launches": pl.launches}
        line.update(common)
        emit(line, args.out)
    for train in (False, True):
        us = measure(head_arms(dtype, train), 1, args.iters, args.repeats)
        line = {"layer": "FCOSHead", "product": "fwd+bwd" if train else "fwd", "Cin": C, "num_classes": NUM_CLASSES,
                "default_routes": heads.FCOS_ROUTES, "us_median_min_max": us}
        line.update(common)
        line["inner"] = 1
        emit(line, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds granted to each dtype")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_gn_bench.jsonl"))
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
