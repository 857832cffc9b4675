#!/usr/bin/env python
"""sha256 of every output tensor of the pyramid-wide kernels that share csrc/pyramid_core.h (csrc/dense_head.hip,
csrc/pyramid_conv.hip, csrc/pyramid_gn.hip, csrc/bfp.hip) on seeded inputs built on the CPU: one JSON line {"lib": ...,
"cases": n, "digests": {case: sha256}}.  Run it once per build, each in a fresh process — TDN_LIB=<another build in the
package directory> chooses the build, as for scripts/gemm128_digest.py — and compare the lines: two builds compute the same
bits iff every digest is equal.

The pyramids are those of tests/test_gpu_dense_head.py, tests/test_gpu_pyramid_conv.py and tests/test_gpu_pyramid_gn.py,
"long" (three 128-row steps per weight-gradient slice) and "empty" included; a digest covers one output over all levels.
Predictors: pack, forward, dgrad, wgrad.  3x3 conv: pack, forward with bias and ReLU / without, dgrad with mask and addend /
plain, wgrad.  GroupNorm: forward and backward, with ReLU and (once) without.  BFP: gather and scatter, forward and
backward, at every refine level, C = 64.  Both dtypes."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch_detection_amd import _lib, dense_ops as D, libra_ops as L, pyramid_ops as P  # noqa: E402

BF, FP = torch.bfloat16, torch.float16
NAME = {BF: "bf16", FP: "fp16"}
PYRAMIDS = {
    "four": (2, [(9, 8), (5, 4), (3, 2), (1, 1)]),
    "one": (1, [(1, 1)]),
    "thin": (1, [(1, 7), (7, 1), (2, 2)]),
    "eight": (1, [(5, 5), (1, 1), (3, 3), (1, 1), (2, 2), (1, 1), (1, 2), (1, 1)]),
    "tile": (2, [(1, 127), (8, 16), (3, 43)]),
    "empty": (0, [(4, 4), (2, 2)]),
    "long": (2, [(82, 100), (3, 2)]),
}
GN_PYRAMIDS = {
    "four": PYRAMIDS["four"],
    "chunks": (1, [(37, 41), (3, 2)]),
    "hole": (2, [(5, 4), (0, 4), (3, 2)]),
    "single": (1, [(6, 10)]),
    "long": PYRAMIDS["long"],
}
BFP_PYRAMIDS = {"four": PYRAMIDS["four"], "up": (1, [(3, 2), (5, 4), (9, 8)])}
# (pyramid, A, C), (pyramid, Cout, Cin), (pyramid, C, groups, ReLU settings)
PRED = [("four", 3, 64), ("four", 12, 64), ("long", 3, 64), ("long", 12, 64), ("eight", 9, 256), ("tile", 3, 64),
        ("one", 12, 64), ("empty", 3, 64)]
CONV = [("four", 9, 64), ("four", 65, 64), ("long", 9, 64), ("long", 65, 64), ("eight", 36, 256), ("tile", 65, 64),
        ("thin", 9, 64), ("empty", 36, 64)]
GN = [("four", 64, 32, (True, False)), ("chunks", 256, 32, (True,)), ("hole", 64, 32, (True,)), ("single", 64, 32, (True,)),
      ("long", 256, 32, (True,))]
gen = torch.Generator().manual_seed(355)
digests = {}


def put(tag, **tensors):
    for name, ts in tensors.items():
        h = hashlib.sha256()
        for t in ts if isinstance(ts, (list, tuple)) else [ts]:
            h.update(t.detach().contiguous().reshape(-1).cpu().view(torch.uint8).numpy().tobytes())
        digests["%s %s" % (tag, name)] = h.hexdigest()


def maps(B, sizes, ch, dt, zeros=False):
    """Per level a logical (B, ch, H, W) tensor in channels_last memory, a quarter of it exact zeros when asked."""
    out = []
    for H, W in sizes:
        t = torch.randn(B, H, W, ch, generator=gen)
        if zeros:
            t[torch.rand(t.shape, generator=gen) < 0.25] = 0
        out.append(t.to(dt).cuda().permute(0, 3, 1, 2))
    return out


def pred(name, A, C, dt):
    B, sizes = PYRAMIDS[name]
    tag = "pred %s A%d C%d %s" % (name, A, C, NAME[dt])
    hs, gc, gr = maps(B, sizes, C, dt, True), maps(B, sizes, A, dt), maps(B, sizes, 4 * A, dt)
    wc, wr = (torch.randn(A, C, generator=gen) / C ** 0.5).cuda(), (torch.randn(4 * A, C, generator=gen) / C ** 0.5).cuda()
    bc, br = torch.randn(A, generator=gen).cuda(), torch.randn(4 * A, generator=gen).cuda()
    w_fwd, w_dgrad = D.pack_pred_weight(wc, wr, True, dt)
    cls, reg = D.pred_fwd(hs, w_fwd, bc, br)
    dwc, dbc, dwr, dbr = D.pred_wgrad(hs, gc, gr)
    put(tag, w_fwd=w_fwd, w_dgrad=w_dgrad, cls=cls, reg=reg, dh=D.pred_dgrad(gc, gr, w_dgrad, hs), dw_cls=dwc, dbias_cls=dbc,
        dw_reg=dwr, dbias_reg=dbr)


def conv(name, Cout, Cin, dt):
    B, sizes = PYRAMIDS[name]
    tag = "conv %s O%d C%d %s" % (name, Cout, Cin, NAME[dt])
    xs, gs = maps(B, sizes, Cin, dt, True), maps(B, sizes, Cout, dt)
    ms, ad = maps(B, sizes, Cin, dt, True), maps(B, sizes, Cin, dt)
    w = (torch.randn(Cout, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5).cuda()
    b = torch.randn(Cout, generator=gen).cuda()
    w_fwd, w_dgrad = P.pack_pyramid_weight(w, True, dt)
    dw, db = P.pyramid_conv_wgrad(xs, gs)
    put(tag, w_fwd=w_fwd, w_dgrad=w_dgrad, y_relu=P.pyramid_conv_fwd(xs, w_fwd, b, Cout, True),
        y_plain=P.pyramid_conv_fwd(xs, w_fwd, None, Cout), dx_masked=P.pyramid_conv_dgrad(gs, w_dgrad, ms, ad),
        dx_plain=P.pyramid_conv_dgrad(gs, w_dgrad), dw=dw, dbias=db)


def gn(name, C, G, relus, dt):
    B, sizes = GN_PYRAMIDS[name]
    tag = "gn %s C%d G%d %s" % (name, C, G, NAME[dt])
    zs, gs = maps(B, sizes, C, dt), maps(B, sizes, C, dt)
    gamma, beta = (1 + 0.5 * torch.randn(C, generator=gen)).cuda(), torch.randn(C, generator=gen).cuda()
    for relu in relus:
        ys, stats = P.pyramid_gn_fwd(zs, gamma, beta, G, 1e-5, relu)
        dzs, dgamma, dbeta = P.pyramid_gn_bwd(gs, ys, zs, stats, gamma, G, relu)
        put("%s relu%d" % (tag, relu), y=ys, stats=stats, dz=dzs, dgamma=dgamma, dbeta=dbeta)


def bfp(name, dt):
    B, sizes = BFP_PYRAMIDS[name]
    C = 64
    xs, gs = maps(B, sizes, C, dt), maps(B, sizes, C, dt)
    for r in range(len(sizes)):
        tag = "bfp %s refine%d %s" % (name, r, NAME[dt])
        bsf = L.bfp_gather_fwd(xs, r)
        dbsf = L.bfp_scatter_bwd(gs, bsf, r)
        put(tag, bsf=bsf, out=L.bfp_scatter_fwd(xs, bsf, r), dbsf=dbsf, dx=L.bfp_gather_bwd(xs, gs, dbsf, r))


for dt in (BF, FP):
    for case in PRED:
        pred(*case, dt)
    for case in CONV:
        conv(*case, dt)
    for case in GN:
        gn(*case, dt)
    for name in BFP_PYRAMIDS:
        bfp(name, dt)
torch.cuda.synchronize()
print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "cases": len(digests), "digests": digests}))
