#!/usr/bin/env python
"""sha256 of every output tensor of the normalisation kernels (csrc/gn.hip, csrc/pyramid_gn.hip) on seeded inputs built
on the CPU: one JSON line {"lib": ..., "digests": {case: sha256}}.  Run it once per build, each in a fresh process —
TDN_LIB=<another build in the package directory> chooses the build, as for scripts/norm_bench.py — and compare the
lines: two builds compute the same bits iff every digest is equal.

Cases: gn_fwd / gn_bwd on GEOM_CASES and CASES of tests/test_gpu_gn.py; bn_train_fwd / bn_train_bwd with running
statistics on BN_GEOM_CASES and BN_CASES; the options at OPT_SHAPE (addend SAME and UP2X, relu 0 / 1 / 2, accumulate
0 and 1); pyramid_gn_fwd / pyramid_gn_bwd on every PYRAMIDS x CG of tests/test_gpu_pyramid_gn.py in both dtypes."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import test_gpu_gn as GN  # noqa: E402
import test_gpu_pyramid_gn as PG  # noqa: E402
from torch_detection_amd import _lib, ops, pyramid_ops  # noqa: E402

BF, FP = torch.bfloat16, torch.float16
NAME = {BF: "bf16", FP: "fp16"}
gen = torch.Generator().manual_seed(20)
digests = {}


def rnd(shape, dt, scale=1.5, shift=0.3):
    """NHWC device tensor of dt; sample n is shifted by n % 8 so that neighbouring samples do not share statistics"""
    t = torch.randn(*shape, generator=gen) * scale + shift + (torch.arange(shape[0]) % 8).view(-1, 1, 1, 1)
    return t.to(dt).cuda()


def vec(C, lo, hi):
    return (torch.rand(C, generator=gen) * (hi - lo) + lo).cuda()


def put(tag, names, tensors):
    for name, t in zip(names, tensors):
        flat = t.detach().contiguous().reshape(-1).cpu()
        digests["%s %s" % (tag, name)] = hashlib.sha256(flat.view(torch.uint8).numpy().tobytes()).hexdigest()


def gn(N, C, H, W, G, dt, addend=None, relu=False, mode=ops.ADD_SAME, acc=False, tag=""):
    tag = "gn N%d C%d %dx%d G%d %s%s" % (N, C, H, W, G, NAME[dt], tag)
    z, g, gamma, beta = rnd((N, H, W, C), dt), rnd((N, H, W, C), dt, 1.0, 0.0), vec(C, 0.5, 1.5), vec(C, -0.5, 0.5)
    y, stats = ops.gn_fwd(z, gamma, beta, G, 1e-5, addend, relu, mode)
    dg, db = (vec(C, -30, 30), vec(C, -30, 30)) if acc else (None, None)
    bwd = ops.gn_bwd(g, z, stats, gamma, G, dg, db, acc)
    put(tag, ("y", "stats", "dz", "dgamma", "dbeta"), (y, stats) + tuple(bwd))


def bn(N, C, H, W, dt, addend=None, relu=False, mode=ops.ADD_SAME, acc=False, tag=""):
    tag = "bn N%d C%d %dx%d %s%s" % (N, C, H, W, NAME[dt], tag)
    z, g, gamma, beta = rnd((N, H, W, C), dt), rnd((N, H, W, C), dt, 1.0, 0.0), vec(C, 0.5, 1.5), vec(C, -0.5, 0.5)
    rm, rv = vec(C, -1, 1), vec(C, 0.5, 2)
    y, stats = ops.bn_train_fwd(z, gamma, beta, rm, rv, 0.1, 1e-5, addend, relu, mode)
    dg, db = (vec(C, -30, 30), vec(C, -30, 30)) if acc else (None, None)
    put(tag, ("y", "stats", "running_mean", "running_var", "dz", "dgamma", "dbeta"),
        (y, stats, rm, rv) + tuple(ops.bn_train_bwd(g, z, stats, gamma, dg, db, acc)))


for N, C, H, W, G, dt in GN.GEOM_CASES:
    gn(N, C, H, W, G, dt)
for N, C, H, W in GN.CASES:
    for dt in (BF, FP):
        gn(N, C, H, W, 32, dt)
for N, C, H, W, dt in GN.BN_GEOM_CASES:
    bn(N, C, H, W, dt)
for N, C, H, W in GN.BN_CASES:
    for dt in (BF, FP):
        bn(N, C, H, W, dt)
N, C, H, W = GN.OPT_SHAPE
for dt in (BF, FP):
    for fn, extra in ((gn, (32,)), (bn, ())):
        for relu in (0, 1, 2):
            fn(N, C, H, W, *extra, dt, rnd((N, H, W, C), dt), relu, ops.ADD_SAME, tag=" same relu%d" % relu)
        fn(N, C, H, W, *extra, dt, rnd((N, H // 2, W // 2, C), dt), 1, ops.ADD_UP2X, tag=" up2x relu1")
        fn(N, C, H, W, *extra, dt, None, 0, ops.ADD_SAME, True, tag=" acc")
for name, (B, sizes) in PG.PYRAMIDS.items():
    for C, G in PG.CG:
        for dt in (BF, FP):
            for relu in (False, True):
                tag = "pyr %s C%d G%d %s relu%d" % (name, C, G, NAME[dt], relu)
                zs = [rnd((B, H, W, C), dt, 1.0 + 0.5 * l, -0.7 * l).permute(0, 3, 1, 2)
                      for l, (H, W) in enumerate(sizes)]
                gs = [rnd((B, H, W, C), dt, 1.0, 0.0).permute(0, 3, 1, 2) for H, W in sizes]
                gamma, beta = vec(C, 0.5, 1.5), vec(C, -0.5, 0.5)
                ys, stats = pyramid_ops.pyramid_gn_fwd(zs, gamma, beta, G, 1e-5, relu)
                dzs, dg, db = pyramid_ops.pyramid_gn_bwd(gs, ys if relu else None, zs, stats, gamma, G, relu)
                put(tag, ["y%d" % l for l in range(len(ys))] + ["stats"] + ["dz%d" % l for l in range(len(dzs))] +
                    ["dgamma", "dbeta"], list(ys) + [stats] + list(dzs) + [dg, db])
torch.cuda.synchronize()
print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "cases": len(digests), "digests": digests}))
