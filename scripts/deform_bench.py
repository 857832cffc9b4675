#!/usr/bin/env python
"""Deformable convolution (csrc/deform.hip) at the ResNet-50 c3-c5 shapes of an 800x1344 batch — B = 2,
(C 128, 100x168), (256, 50x84), (512, 25x42), Cout = C, stride 1, one deformable group, DCN v2 (with a mask) — beside the
plain 3x3 conv of the same shape on the existing kernels:

  ``deform_fwd`` / ``deform_fwd_bwd``   ``deform_conv2d`` without / with its backward (all five gradients);
  ``conv_fwd`` / ``conv_fwd_bwd``       ``ops.conv2d_fwd`` alone / with ``conv2d_dgrad`` and ``conv2d_wgrad``;
  ``sample``, ``coord_grad``, ``input_grad``, ``input_grad_one_pixel``   the kernels of this family alone, the last one on
                                        the adversarial offsets that put every sample of an image on pixel (3, 4).

Offsets are N(0, 2 px).  Method (scripts/pyramid_conv_bench.py): every arm is captured as a graph of ``--inner`` calls and
replayed; device events after warm-up; the arms of one shape are alternated inside each of ``--repeats`` windows; median,
min and max are reported.  The one-pixel arm is serial by construction and is timed with one call per graph.  Every shape
runs in a child process of its own under its own time limit; the first that fails or times out ends the run.

``--trace`` runs every arm of every shape a few times eagerly and measures nothing: the run to put under
``rocprofv3 --kernel-trace --stats`` for the per-kernel times.  Prints one JSON object per measurement and appends it to
``--out``."""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from pyramid_conv_bench import COPY_RATE, PEAK_FLOPS, emit, measure  # noqa: E402

B, SIGMA = 2, 2.0
SHAPES = [(128, 100, 168), (256, 50, 84), (512, 25, 42)]


def arms_of(C, H, W, dtype):
    import torch_detection_amd as T
    from torch_detection_amd import deform_ops as D
    from torch_detection_amd import functional, ops
    functional.REPACK_IN_CAPTURE = False       # time the layers: the weight repack of a captured step is no part of an arm
    gen = torch.Generator().manual_seed(C)
    nhwc = lambda ch, scale=1.0, dt=dtype: (torch.randn(B, H, W, ch, generator=gen) * scale).cuda().to(dt)
    x, gy = nhwc(C), nhwc(C)
    off, msk = nhwc(18, SIGMA), torch.rand(B, H, W, 9, generator=gen).cuda().to(dtype)
    w = (torch.randn(C, C, 3, 3, generator=gen) / (9 * C) ** 0.5).cuda()
    b = torch.randn(C, generator=gen).cuda()
    lx, lo, lm, lg = (t.permute(0, 3, 1, 2) for t in (x, off, msk, gy))
    # every sample of an image on pixel (3, 4)
    k = torch.arange(9)
    by = torch.arange(H).view(1, H, 1) - 1 + (k // 3).view(9, 1, 1)
    bx = torch.arange(W).view(1, 1, W) - 1 + (k % 3).view(9, 1, 1)
    one = torch.stack([(3 - by).expand(9, H, W), (4 - bx).expand(9, H, W)], 1).reshape(18, H, W)
    one = one.permute(1, 2, 0).expand(B, H, W, 18).contiguous().cuda().float().permute(0, 3, 1, 2)
    w_fwd, w_dgrad = ops.pack_conv_weight(w, None, True, dtype)
    dcol = D.deform_sample(lx, lo, lm)          # any (B, H, W, 9 C) tensor of ordinary size serves as a cotangent
    leaves = [t.detach().requires_grad_() for t in (lx, lo, lm, w, b)]

    def deform_fwd():
        with torch.no_grad():
            return T.deform_conv2d(lx, lo, w, b, mask=lm)

    def deform_fwd_bwd():
        y = T.deform_conv2d(leaves[0], leaves[1], leaves[3], leaves[4], mask=leaves[2])
        return torch.autograd.grad(y, leaves, lg)

    def conv_fwd_bwd():
        y = ops.conv2d_fwd(x, w_fwd, 3, 1, 1, None, b)
        dx = ops.conv2d_dgrad(gy, w_dgrad, (H, W), 3, 1, 1)
        return y, dx, ops.conv2d_wgrad(x, gy, w_fwd, 3, 1, 1)

    arms = {"deform_fwd": deform_fwd, "deform_fwd_bwd": deform_fwd_bwd,
            "conv_fwd": lambda: ops.conv2d_fwd(x, w_fwd, 3, 1, 1, None, b), "conv_fwd_bwd": conv_fwd_bwd,
            "sample": lambda: D.deform_sample(lx, lo, lm),
            "coord_grad": lambda: D.deform_coord_grad(dcol, lx, lo, lm),
            "input_grad": lambda: D.deform_input_grad(dcol, lo, lm, (B, C, H, W))}
    slow = {"input_grad_one_pixel": lambda: D.deform_input_grad(dcol, one, None, (B, C, H, W))}
    return arms, slow


def run_step(idx, args):
    C, H, W = SHAPES[idx]
    dtype = getattr(torch, args.dtype)
    arms, slow = arms_of(C, H, W, dtype)
    if args.trace:
        for fn in list(arms.values()) + list(slow.values()):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        return
    us = measure(arms, args.inner, args.iters, args.repeats)
    us.update(measure(slow, 1, 1, 3))
    M = B * H * W
    ok = lambda k: isinstance(us.get(k), list)
    ratio = lambda a, c: round(us[a][0] / us[c][0], 2) if ok(a) and ok(c) else None
    # the gather's traffic: x read (from cache, 4 corners) and cols written; the GEMM then reads cols again
    cols_bytes = M * 9 * C * 2
    # the input gradient must read dcol once and write dx once
    ig_bytes = cols_bytes + M * C * 2
    line = {"layer": "deform_conv", "dtype": args.dtype, "B": B, "C": C, "Cout": C, "H": H, "W": W, "dg": 1, "mask": True,
            "offset_sigma_px": SIGMA, "us_median_min_max": us,
            "fwd_ratio_to_conv": ratio("deform_fwd", "conv_fwd"),
            "fwd_bwd_ratio_to_conv": ratio("deform_fwd_bwd", "conv_fwd_bwd"),
            "gflop_fwd": round(2.0 * M * 9 * C * C / 1e9, 2), "cols_mbytes": round(cols_bytes / 1e6, 2),
            "gemm_roofline_us": round(max(2.0 * M * 9 * C * C / PEAK_FLOPS, cols_bytes / COPY_RATE) * 1e6, 1),
            "input_grad_byte_bound_us": round(ig_bytes / COPY_RATE * 1e6, 1),
            "input_grad_fraction_of_copy_rate": (round(ig_bytes / COPY_RATE * 1e6 / us["input_grad"][0], 3)
                                                 if ok("input_grad") else None),
            "inner": args.inner, "iters": args.iters, "repeats": args.repeats}
    emit(line, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--trace", action="store_true", help="run the arms eagerly and measure nothing (for rocprofv3)")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds granted to each shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_bench.jsonl"))
    ap.add_argument("--step", type=int, default=None, help="internal: the shape to run in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args)
        return 0
    for idx in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(idx), "--inner", str(args.inner), "--iters",
               str(args.iters), "--repeats", str(args.repeats), "--dtype", args.dtype, "--out", args.out]
        if args.trace:
            cmd.append("--trace")
        try:
            rc = subprocess.run(cmd, timeout=args.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("shape %s ended with status %d: stopping" % (SHAPES[idx], rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
