#!/usr/bin/env python
"""Median device-event time of gn_fwd / bn_train_fwd (+ residual add, ReLU) and of gn_bwd / bn_train_bwd at
(2, 256, 200, 336) bf16: 30 warm-up calls, then 300 timed replays each; prints one JSON line (median, 10th and 90th
percentile in microseconds).
TDN_LIB=<another build in the package directory> times that build instead, for an A/B run in alternation."""
import json
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from torch_detection_amd import ops, _lib

N, C, H, W = 2, 256, 200, 336
g = torch.Generator(device="cuda").manual_seed(1)
z = (torch.randn(N, H, W, C, device="cuda", generator=g) * 1.5 + 0.3).bfloat16()
res = torch.randn(N, H, W, C, device="cuda", generator=g).bfloat16()
gamma = torch.rand(C, device="cuda", generator=g) + 0.5
beta = torch.rand(C, device="cuda", generator=g) - 0.5
rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
fns = {"gn_fwd": lambda: ops.gn_fwd(z, gamma, beta, 32, 1e-5, res, True),
       "bn_train_fwd": lambda: ops.bn_train_fwd(z, gamma, beta, rm, rv, 0.1, 1e-5, res, True)}
gn_stats, bn_stats = fns["gn_fwd"]()[1], fns["bn_train_fwd"]()[1]
fns["gn_bwd"] = lambda: ops.gn_bwd(res, z, gn_stats, gamma, 32)
fns["bn_train_bwd"] = lambda: ops.bn_train_bwd(res, z, bn_stats, gamma)
out = {"lib": os.path.basename(_lib.LIB_PATH)}
for name, fn in fns.items():
    for _ in range(30):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(300):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    out[name] = {"median_us": round(ts[len(ts) // 2], 2), "p10_us": round(ts[len(ts) // 10], 2),
                 "p90_us": round(ts[len(ts) * 9 // 10], 2)}
y, st = fns["gn_fwd"]()
out["gn_y_checksum"] = float(y.float().sum())
print(json.dumps(out))
