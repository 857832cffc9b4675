#!/usr/bin/env python3
"""Every workspace size query of the detection-head files, and the plan and workspace queries of the pyramid-wide heads
(csrc/pyramid_core.h), over a fixed grid of arguments (host arithmetic: no device is touched).  For comparing two builds of the library:

    python scripts/workspace_query_grid.py OTHER/libtdn.so [THIS/libtdn.so]

loads each library in a child process of its own, prints the number of points and a digest per query, and exits 1 if
any returned value differs.  `--one LIB` is the child: it prints `query args -> value` lines.
"""
import ctypes
import hashlib
import itertools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pyramid(H, W, L, empty_level=None):
    maps = [((H + (1 << l) - 1) >> l, (W + (1 << l) - 1) >> l) for l in range(L)]
    if empty_level is not None and empty_level < L:
        maps[empty_level] = (0, 0)
    return maps


def points(_lib):
    B5 = (0, 1, 2, 64, 65)
    G7 = (-1, 0, 1, 63, 64, 256, 257)
    for N in (-1, 0, 1, 63, 64, 65, 4096, 512000, 512001):
        yield "tdn_nms_workspace", (N,), (N,)
    for N, S in itertools.product((-1, 0, 1, 63, 64, 65, 4095, 4096, 4097, 100000), (-1, 0, 1, 5, 80)):
        yield "tdn_batched_nms_workspace", (N, S), (N, S)
    dummy = 0x1000
    bases = ((0, 0), (1, 1), (3, 5), (13, 21), (50, 84), (100, 168), (200, 336))
    for L, (H, W), A, pre, B, empty in itertools.product((1, 2, 5, 8, 9), bases, (1, 3, 9), (0, 1, 1000, 4096), B5,
                                                        (None, 1)):
        if empty is not None and L == 1:
            continue
        maps = pyramid(H, W, L, empty)
        lv = (_lib.RpnLevel * L)()
        for l, (h, w) in enumerate(maps):
            lv[l].logits = lv[l].deltas = lv[l].anchors = dummy
            lv[l].dtype, lv[l].H, lv[l].W, lv[l].A = _lib.TDN_F32, h, w, A
        for nms_post, max_num in ((1000, 1000), (0, 1000), (1000, 8193)):
            cfg = _lib.RpnConfig(nms_pre=pre, nms_post=nms_post, max_num=max_num, nms_thr=0.7, min_bbox_size=0.0)
            yield "tdn_rpn_proposals_workspace", (lv, L, B, ctypes.byref(cfg)), (L, H, W, A, pre, B, empty, nms_post,
                                                                                 max_num)
    for B, G in itertools.product(B5, G7):
        yield "tdn_assign_max_iou_workspace_bytes", (B, G), (B, G)
        for N in (-1, 0, 1, 255, 256, 257, 268569, 1 << 20, (1 << 20) + 1):
            yield "tdn_anchor_target_workspace_bytes", (B, N, G), (B, N, G)
        for P, add in itertools.product((-1, 0, 1, 2000, (1 << 20) - 256, (1 << 20) - 255), (0, 1)):
            yield "tdn_sample_rois_workspace_bytes", (B, P, G, add), (B, P, G, add)
    for R in (-1, 0, 1, 5, 16, 17, 1000, (1 << 31) - 1, 1 << 31):
        yield "tdn_roi_align_bwd_workspace", (R,), (R,)
    for R in (-1, 0, 1, 3, 4, 5, 15, 16, 17, 1031, 4096, 4097, 1 << 20, (1 << 20) + 1):
        yield "tdn_loss_roi_workspace_bytes", (R,), (R,)
    lbases = ((1, 1), (3, 5), (13, 21), (50, 84), (100, 168), (200, 336),
              (1 << 15, 1), ((1 << 15) - 1, 1),         # with B = 64, C = 1024: a level of exactly 2^31 elements / just under
              (1024, 1024), (1024, 1025), (0, 4))       # A = 1: TDN_LOSS_MAX_ROWS anchors / just over; an empty map
    for L, (H, W), dt, A, C, B in itertools.product((0, 1, 5, 8, 9), lbases, (_lib.TDN_BF16, _lib.TDN_F16, _lib.TDN_F32, 3),
                                                    (0, 1, 9), (1, 80, 1024, 1025), (0, 1, 64, 65)):
        maps = pyramid(H, W, max(L, 1))
        lv = (_lib.LossLevel * max(L, 1))()
        for l, (h, w) in enumerate(maps):
            lv[l].H, lv[l].W = h, w                      # the pointers stay NULL: a size query does not look at them
        cfg = _lib.LossConfig(dtype=dt, num_anchors=A, num_classes=C, focal=0, beta=1.0 / 9.0)
        yield "tdn_loss_dense_workspace_bytes", (lv, L, B, ctypes.byref(cfg)), (L, H, W, dt, A, C, B)
    yield "tdn_loss_dense_workspace_bytes", (None, 1, 1, None), "NULL"
    # the pyramid-wide heads (csrc/pyramid_core.h): level counts 0..9, an empty level, row totals on both sides of the
    # wgrad slice threshold (64 slices x 128 rows for the predictors), refused kinds, channels and sizes
    pbases = ((1, 1), (3, 5), (13, 21), (50, 84), (64, 127), (64, 128), (64, 129), (100, 168), (200, 336), (1 << 15, 1 << 15))
    for kind, L, (H, W), B, empty in itertools.product((-1, 0, 1, 2, 3), (0, 1, 2, 5, 8, 9), pbases, (0, 1, 2), (None, 1)):
        if (empty is not None and L < 2) or (kind in (-1, 3) and (L, B) != (5, 2)):
            continue
        maps = pyramid(H, W, max(L, 1), empty)
        hw = (ctypes.c_int32 * (2 * len(maps)))(*[v for m in maps for v in m])
        rows = (ctypes.c_int64 * len(maps))(*[B * h * w for h, w in maps])
        for A, C in ((1, 64), (3, 256), (12, 512), (0, 64), (13, 64), (3, 0), (3, 96), (3, 576)):
            yield "tdn_pred_workspace_bytes", (kind, rows, L, C, A), (kind, L, H, W, B, empty, C, A)
            yield "tdn_pred_plan", (kind, rows, L, C, A), (kind, L, H, W, B, empty, C, A, "plan")
        for Cin, Cout in ((64, 1), (64, 9), (64, 65), (256, 36), (512, 720), (64, 1024), (64, 0), (64, 1025), (96, 9), (576, 9)):
            yield "tdn_pyr_workspace_bytes", (kind, B, hw, L, Cin, Cout), (kind, L, H, W, B, empty, Cin, Cout)
            yield "tdn_pyr_plan", (kind, B, hw, L, Cin, Cout), (kind, L, H, W, B, empty, Cin, Cout, "plan")
        if kind < 2:
            for C, G in ((64, 32), (128, 32), (256, 32), (512, 2), (512, 1), (96, 32), (256, 3), (256, 0)):
                yield "tdn_pyr_gn_workspace_bytes", (kind, B, hw, L, C, G), (kind, L, H, W, B, empty, C, G)
                yield "tdn_pyr_gn_plan", (kind, B, hw, L, C, G), (kind, L, H, W, B, empty, C, G, "plan")
    for B in (-1, 8191, 8192):
        hw = (ctypes.c_int32 * 2)(3, 5)
        yield "tdn_pyr_gn_workspace_bytes", (0, B, hw, 1, 64, 32), (B, "B")
        yield "tdn_pyr_workspace_bytes", (2, B, hw, 1, 64, 9), (B, "B")
    yield "tdn_pred_plan", (2, None, 1, 64, 3), ("NULL", "plan")
    yield "tdn_pyr_plan", (2, 1, None, 1, 64, 9), ("NULL", "plan")
    yield "tdn_pyr_gn_plan", (0, 1, None, 1, 64, 32), ("NULL", "plan")


def one(lib_path):
    from torch_detection_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib_path)
    lib = _lib.load()
    for name, args, key in points(_lib):
        if name.endswith("_plan"):                       # a plan query: the record it wrote, or the refusal's text
            out = (ctypes.c_int32 * 32)(*([-7] * 32))
            rc = getattr(lib, name)(*(args + (out,)))
            print(name, key, "->", rc, list(out) if rc == 0 else lib.tdn_last_error().decode())
        else:
            print(name, key, "->", getattr(lib, name)(*args))


def main(argv):
    if argv[:1] == ["--one"]:
        one(argv[1])
        return 0
    libs = argv + [os.path.join(ROOT, "torch_detection_amd", "libtdn.so")] if len(argv) == 1 else argv
    outs = [subprocess.check_output([sys.executable, os.path.abspath(__file__), "--one", p]).decode().splitlines()
            for p in libs]
    per = {}
    for a, b in zip(*outs):
        q = a.split()[0]
        n, d, h, r = per.setdefault(q, [0, 0, hashlib.sha256(), 0])
        per[q][0] += 1
        per[q][1] += a != b
        per[q][3] += a.endswith("-> -1") or "-> -1 " in a
        h.update(a.encode())
    assert len(outs[0]) == len(outs[1])
    for q, (n, d, h, r) in per.items():
        print("%-38s %6d points (%5d refused)  %d differ  %s" % (q, n, r, d, h.hexdigest()[:16]))
    total, diff = sum(v[0] for v in per.values()), sum(v[1] for v in per.values())
    print("total %d points, %d differ" % (total, diff))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
