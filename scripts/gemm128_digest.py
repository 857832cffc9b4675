#!/usr/bin/env python
"""sha256 of every output tensor of the ring GEMMs that share csrc/gemm128_core.h (csrc/linear.hip, csrc/deconv.hip) on
seeded inputs built on the CPU: one JSON line {"lib": ..., "cases": n, "digests": {case: sha256}}.  Run it once per build,
each in a fresh process — TDN_LIB=<another build in the package directory> chooses the build, as for
scripts/norm_ab_digest.py — and compare the lines: two builds compute the same bits iff every digest is equal.

Linear: shapes (M, K, O) with forced splits and the column permutation C as tests/test_gpu_linear.py lists them — one
partial tile; two row tiles with a ragged last one and ragged O through the pad launch at 1 / 3 / 7 slices; the permuted
columns — forward (bias, ReLU), dgrad (mask), wgrad with beta 0 and 1.  Deconv: SHAPES of tests/test_gpu_deconv.py —
forward, dgrad, wgrad at 0 / 1 / 3 slices (clamped as its wg_splits does) with and without dbias.  Both dtypes."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch_detection_amd import _lib, deconv_ops as D, linear_ops as L  # noqa: E402

BF, FP = torch.bfloat16, torch.float16
NAME = {BF: "bf16", FP: "fp16"}
LINEAR = [((1, 64, 1), 0, None), ((130, 448, 81), 1, None), ((130, 448, 81), 3, None), ((130, 448, 81), 7, None),
          ((257, 3136, 64), 0, 64)]
DECONV = [(1, 1, 1, 64, 64), (3, 5, 7, 128, 64), (5, 3, 9, 64, 192), (2, 14, 14, 256, 256)]
gen = torch.Generator().manual_seed(128)
digests = {}


def rnd(*shape):
    return torch.randn(*shape, generator=gen)


def put(tag, **tensors):
    for name, t in tensors.items():
        if t is not None:
            flat = t.detach().contiguous().reshape(-1).cpu()
            digests["%s %s" % (tag, name)] = hashlib.sha256(flat.view(torch.uint8).numpy().tobytes()).hexdigest()


def wg_splits(splits, M):
    return min(splits, max(1, (M + 63) // 64))


def linear(M, K, O, splits, C, dt):
    tag = "linear M%d K%d O%d s%d C%s %s" % (M, K, O, splits, C, NAME[dt])
    x, g = rnd(M, K).to(dt).cuda(), rnd(M, O).to(dt).cuda()
    w, b = (rnd(O, K) / K ** 0.5).cuda(), rnd(O).cuda()
    mask = rnd(M, K).to(dt).cuda()
    w_fwd, w_dgrad = L.pack_linear_weight(w, C, True, dt)
    put(tag, w_fwd=w_fwd, w_dgrad=w_dgrad, y=L.linear_fwd(x, w_fwd, O, b, True, False, splits),
        y_f32=L.linear_fwd(x, w_fwd, O, None, False, True, splits), dx=L.linear_dgrad(g, w_dgrad, mask, splits))
    for beta in (0.0, 1.0):
        dw, db = rnd(O, K).cuda(), rnd(O).cuda()
        L.linear_wgrad(x, g, C, dw, db, beta, True, wg_splits(splits, M))
        put("%s beta%d" % (tag, beta), dw=dw, dbias=db)


def deconv(R, H, W, Cin, Cout, dt):
    tag = "deconv R%d %dx%d Cin%d Cout%d %s" % (R, H, W, Cin, Cout, NAME[dt])
    x = rnd(R, H, W, Cin).to(dt).cuda().permute(0, 3, 1, 2)
    g = rnd(R, 2 * H, 2 * W, Cout).to(dt).cuda().permute(0, 3, 1, 2)
    w, b = (rnd(Cin, Cout, 2, 2) / Cin ** 0.5).cuda(), rnd(Cout).cuda()
    w_fwd, w_dgrad = D.pack_deconv_weight(w, True, dt)
    put(tag, w_fwd=w_fwd, w_dgrad=w_dgrad, y=D.deconv2x2_fwd(x, w_fwd, b, True), y_plain=D.deconv2x2_fwd(x, w_fwd),
        dx=D.deconv2x2_dgrad(g, w_dgrad))
    for splits in (0, 1, 3):
        for beta, want in ((0.0, True), (0.0, False), (1.0, True)):
            dw, db = rnd(Cin, Cout, 2, 2).cuda(), rnd(Cout).cuda()
            D.deconv2x2_wgrad(x, g, dw, db if want else None, beta, want, wg_splits(splits, R * H * W))
            put("%s s%d beta%d dbias%d" % (tag, splits, beta, want), dw=dw, dbias=db if want else None)


for dt in (BF, FP):
    for (M, K, O), splits, C in LINEAR:
        linear(M, K, O, splits, C, dt)
    for shape in DECONV:
        deconv(*shape, dt)
torch.cuda.synchronize()
print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "cases": len(digests), "digests": digests}))
