#!/usr/bin/env python
"""CARAFE upsampling (csrc/carafe.hip) at the four top-down shapes of the benchmark step's FPN — B = 2,
256 channels, sources 13x21, 25x42, 50x84, 100x168, k = 5, s = 2, one group — beside the same computation composed from
torch ops on the same GPU:

  ``fused_fwd`` / ``fused_fwd_bwd``   the logits-variant reassembly launch alone / with its feature and logit gradients
                                      (``feature_grad`` / ``logit_grad``: those two launches alone);
  ``torch_fwd`` / ``torch_fwd_bwd``   ``F.pixel_shuffle`` + softmax + ``F.unfold`` + einsum, without / with autograd's
                                      backward for the features and the logits;
  ``pack_fwd`` / ``pack_fwd_bwd``     a whole ``CARAFEPack`` (compressor, encoder, reassembly, and their adjoints);
  ``torch_pack_fwd`` / ``torch_pack_fwd_bwd``   the same from ``F.conv2d`` and the composition above.

The record also holds the bytes each fused arm must move (every operand once) and the rate that time amounts to.  Method
(scripts/pyramid_conv_bench.py): every arm is captured as a graph of ``--inner`` calls and replayed; device events after
warm-up; the arms of one shape are alternated inside each of ``--repeats`` windows; median, min and max are reported.  Every
shape runs in a child process of its own under its own time limit; the first that fails or times out ends the run.
Prints one JSON object per shape and appends it to ``--out``."""
import argparse
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from pyramid_conv_bench import COPY_RATE, emit, measure  # noqa: E402

B, C, K, S, CM = 2, 256, 5, 2, 64
SHAPES = [(13, 21), (25, 42), (50, 84), (100, 168)]


def torch_carafe(x, logits):
    """(B, C, H, W), (B, K^2 S^2, H, W) -> (B, C, S H, S W) from torch ops: the unfold holds K^2 times the feature map"""
    N, _, H, W = x.shape
    p = F.softmax(F.pixel_shuffle(logits, S).reshape(N, K * K, H, S, W, S).float(), dim=1).to(x.dtype)
    cols = F.unfold(x, K, padding=K // 2).reshape(N, C, K * K, H, W)
    return torch.einsum("nckhw,nkhywx->nchywx", cols, p).reshape(N, C, H * S, W * S)


def arms_of(H, W, dtype):
    import torch_detection_amd as T
    from torch_detection_amd import carafe_ops as D
    from torch_detection_amd import functional
    functional.REPACK_IN_CAPTURE = False       # time the layers: the weight repack of a captured step is no part of an arm
    gen = torch.Generator().manual_seed(H)
    nhwc = lambda ch, h, w, scale=1.0: (torch.randn(B, h, w, ch, generator=gen) * scale).cuda().to(dtype).permute(0, 3, 1, 2)
    x, logits, gout = nhwc(C, H, W), nhwc(K * K * S * S, H, W, 2.0), nhwc(C, S * H, S * W)
    pack = T.CARAFEPack(C, S, K, 1, compressed_channels=CM).cuda()
    with torch.no_grad():
        pack.content_encoder.weight.mul_(500.0)            # logits of ordinary spread instead of the initial 1e-3
    ws = [p.detach().to(dtype) for p in (pack.channel_compressor.weight, pack.channel_compressor.bias,
                                          pack.content_encoder.weight, pack.content_encoder.bias)]
    lx, ll = x.detach().requires_grad_(), logits.detach().requires_grad_()
    lw = [w.detach().requires_grad_() for w in ws]
    px = x.detach().requires_grad_()

    def fused_fwd_bwd():
        return (D.carafe_forward(x, K, 1, S, logits=logits), D.carafe_feature_grad(gout, (B, C, H, W), K, 1, S, logits=logits),
                D.carafe_mask_grad(gout, x, K, 1, S, logits=logits))

    def torch_fwd():
        with torch.no_grad():
            return torch_carafe(x, logits)

    def torch_pack(xx, w):
        return torch_carafe(xx, F.conv2d(F.conv2d(xx, w[0], w[1]), w[2], w[3], padding=1))

    def torch_pack_fwd():
        with torch.no_grad():
            return torch_pack(x, ws)

    def pack_fwd():
        with torch.no_grad():
            return pack(x)

    def pack_fwd_bwd():
        return torch.autograd.grad(pack(px), [px] + list(pack.parameters()), gout)

    return {"fused_fwd": lambda: D.carafe_forward(x, K, 1, S, logits=logits), "fused_fwd_bwd": fused_fwd_bwd,
            "feature_grad": lambda: D.carafe_feature_grad(gout, (B, C, H, W), K, 1, S, logits=logits),
            "logit_grad": lambda: D.carafe_mask_grad(gout, x, K, 1, S, logits=logits),
            "torch_fwd": torch_fwd, "torch_fwd_bwd": lambda: torch.autograd.grad(torch_carafe(lx, ll), [lx, ll], gout),
            "pack_fwd": pack_fwd, "pack_fwd_bwd": pack_fwd_bwd, "torch_pack_fwd": torch_pack_fwd,
            "torch_pack_fwd_bwd": lambda: torch.autograd.grad(torch_pack(lx, lw), [lx] + lw, gout)}


def run_step(idx, args):
    H, W = SHAPES[idx]
    us = measure(arms_of(H, W, getattr(torch, args.dtype)), args.inner, args.iters, args.repeats)
    ok = lambda k: isinstance(us.get(k), list)
    ratio = lambda a, c: round(us[a][0] / us[c][0], 3) if ok(a) and ok(c) else None
    src, out, lg = B * H * W * C * 2, B * S * H * S * W * C * 2, B * H * W * K * K * S * S * 2
    fwd_bytes = out + lg + src
    bwd_bytes = (out + lg + src) + (out + src + lg + lg)          # dx: gout, logits -> dx;  dlogits: gout, x, logits -> dlogits
    rate = lambda k, nbytes: round(nbytes / (us[k][0] * 1e-6) / 1e12, 3) if ok(k) else None
    emit({"layer": "carafe", "dtype": args.dtype, "B": B, "C": C, "H": H, "W": W, "k": K, "s": S, "group": 1,
          "compressed_channels": CM, "us_median_min_max": us,
          "fused_fwd_ratio_to_torch": ratio("fused_fwd", "torch_fwd"),
          "fused_fwd_bwd_ratio_to_torch": ratio("fused_fwd_bwd", "torch_fwd_bwd"),
          "pack_fwd_ratio_to_torch": ratio("pack_fwd", "torch_pack_fwd"),
          "pack_fwd_bwd_ratio_to_torch": ratio("pack_fwd_bwd", "torch_pack_fwd_bwd"),
          "fwd_mbytes": round(fwd_bytes / 1e6, 2), "fwd_bwd_mbytes": round((fwd_bytes + bwd_bytes) / 1e6, 2),
          "fwd_byte_bound_us": round(fwd_bytes / COPY_RATE * 1e6, 1),
          "fwd_bwd_byte_bound_us": round((fwd_bytes + bwd_bytes) / COPY_RATE * 1e6, 1),
          "fused_fwd_tbytes_per_s": rate("fused_fwd", fwd_bytes),
          "fused_fwd_bwd_tbytes_per_s": rate("fused_fwd_bwd", fwd_bytes + bwd_bytes),
          "inner": args.inner, "iters": args.iters, "repeats": args.repeats}, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds granted to each shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carafe_bench.jsonl"))
    ap.add_argument("--step", type=int, default=None, help="internal: the shape to run in this process")
    args = ap.parse_args()
    if args.step is not None:
        run_step(args.step, args)
        return 0
    for idx in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(idx), "--inner", str(args.inner), "--iters",
               str(args.iters), "--repeats", str(args.repeats), "--dtype", args.dtype, "--out", args.out]
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
