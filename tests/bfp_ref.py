"""NumPy oracle of the Balanced Feature Pyramid (csrc/bfp.hip), restated from the specification with
per-axis index tables built on the host.

Maps are float32 arrays (B, C, H, W) holding values of the 16-bit storage type; ``rnd`` rounds an fp32 array once to that
type (``quant(dtype)``; the identity keeps fp32, which is what the comparisons with torch's CPU ops use).  Sums are fp32,
term by term in the stated order, starting from +0.

  pool window o of n -> m      [floor(o n / m), ceil((o + 1) n / m))        (adaptive_max_pool2d; windows may overlap)
  nearest source of d, n -> m  min(int(floorf(fp32(d) * (fp32(n) / fp32(m)))), n - 1), in fp32   (interpolate)
  maximum of a window          the FIRST one in row-major order: strict > against a running maximum that starts at the
                               window's first element
"""
import numpy as np

F32 = np.float32


def quant(dtype):
    """torch dtype -> a function rounding an fp32 array once (to nearest even) to it and back to fp32."""
    import torch

    def rnd(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dtype).float().numpy()
    return rnd


def pool_windows(n, m):
    """[(lo, hi)] for the m outputs of an adaptive pool over n inputs."""
    return [((o * n) // m, -((-(o + 1) * n) // m)) for o in range(m)]


def nearest_src(n_in, n_out):
    """The source index of each of n_out destinations, torch's fp32 rule."""
    scale = F32(n_in) / F32(n_out)
    return [min(int(np.floor(F32(d) * scale)), n_in - 1) for d in range(n_out)]


def windows(mode, n_src, n_dst):
    """Per destination index the window [lo, hi) of source indices: 'pool' or 'nearest' (a window of one)."""
    if mode == "pool":
        return pool_windows(n_src, n_dst)
    return [(s, s + 1) for s in nearest_src(n_src, n_dst)]


def first_argmax(win):
    """win (B, C, h, w) -> (flat index (B, C) of the first maximum of every 2-D window in row-major order, that maximum):
    strict > against a running maximum that starts at the window's first element."""
    h, w = win.shape[2:]
    best = win[:, :, 0, 0].copy()
    at = np.zeros(best.shape, np.int64)
    for k in range(1, h * w):
        v = win[:, :, k // w, k % w]
        m = v > best
        best = np.where(m, v, best)
        at = np.where(m, k, at)
    return at, best


def resize(mode, src, size):
    """(B, C, Hs, Ws) -> (values (B, C, H, W), arg (B, C, H, W, 2) int: the source element each destination took)."""
    B, C, Hs, Ws = src.shape
    H, W = size
    wy, wx = windows(mode, Hs, H), windows(mode, Ws, W)
    out = np.empty((B, C, H, W), F32)
    arg = np.empty((B, C, H, W, 2), np.int64)
    for y in range(H):
        for x in range(W):
            (y0, y1), (x0, x1) = wy[y], wx[x]
            at, v = first_argmax(src[:, :, y0:y1, x0:x1])
            out[:, :, y, x] = v
            arg[:, :, y, x, 0] = y0 + at // (x1 - x0)
            arg[:, :, y, x, 1] = x0 + at % (x1 - x0)
    return out, arg


def resize_adjoint(arg, cot, src_size):
    """The adjoint of ``resize``: per source element the fp32 sum, in row-major order of the destinations, of the
    cotangents of the destinations that took it."""
    B, C, H, W = cot.shape
    out = np.zeros((B, C) + tuple(src_size), F32)
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    for y in range(H):
        for x in range(W):
            sy, sx = arg[:, :, y, x, 0], arg[:, :, y, x, 1]          # one target per (image, channel): no collisions
            out[bi, ci, sy, sx] = (out[bi, ci, sy, sx] + cot[:, :, y, x]).astype(F32)
    return out


def modes(l, refine_level):
    """(gather mode, scatter mode) of level l"""
    return ("pool", "nearest") if l < refine_level else ("nearest", "pool")


def gather_fwd(xs, refine_level, rnd=lambda a: a):
    """-> (bsf, args): bsf = rnd((0 + M_0(x_0) + M_1(x_1) + ...) / L)"""
    size = xs[refine_level].shape[2:]
    acc = np.zeros(xs[0].shape[:2] + tuple(size), F32)
    args = []
    for l, x in enumerate(xs):
        v, a = resize(modes(l, refine_level)[0], np.asarray(x, F32), size)
        acc = (acc + v).astype(F32)
        args.append(a)
    return rnd((acc / F32(len(xs))).astype(F32)), args


def scatter_fwd(xs, bsf, refine_level, rnd=lambda a: a):
    """-> (outs, args): out_l = rnd(N_l(bsf) + x_l)"""
    outs, args = [], []
    for l, x in enumerate(xs):
        v, a = resize(modes(l, refine_level)[1], np.asarray(bsf, F32), x.shape[2:])
        outs.append(rnd((v + np.asarray(x, F32)).astype(F32)))
        args.append(a)
    return outs, args


def scatter_bwd(gs, scatter_args, size, rnd=lambda a: a):
    """-> d bsf' = rnd(0 + s_0 + s_1 + ...), s_l the adjoint of N_l of g_l"""
    acc = np.zeros(gs[0].shape[:2] + tuple(size), F32)
    for g, a in zip(gs, scatter_args):
        acc = (acc + resize_adjoint(a, np.asarray(g, F32), size)).astype(F32)
    return rnd(acc)


def gather_bwd(gs, gather_args, dbsf, rnd=lambda a: a):
    """-> dx_l = rnd(g_l + adjoint of M_l of d bsf / L)"""
    L = F32(len(gs))
    out = []
    for g, a in zip(gs, gather_args):
        s = resize_adjoint(a, np.asarray(dbsf, F32), g.shape[2:])
        out.append(rnd((np.asarray(g, F32) + (s / L).astype(F32)).astype(F32)))
    return out


def bfp(xs, gs, refine_level, rnd=lambda a: a, refine=None, refine_bwd=None):
    """The whole neck without (``refine`` None) or with a refine step given as two callables on (B, C, Hg, Wg) arrays.
    -> dict(bsf, refined, outs, dbsf_refined, dbsf, dxs)"""
    bsf, ga = gather_fwd(xs, refine_level, rnd)
    refined = bsf if refine is None else refine(bsf)
    outs, sa = scatter_fwd(xs, refined, refine_level, rnd)
    dref = scatter_bwd(gs, sa, bsf.shape[2:], rnd)
    dbsf = dref if refine_bwd is None else refine_bwd(dref)
    dxs = gather_bwd(gs, ga, dbsf, rnd)
    return dict(bsf=bsf, refined=refined, outs=outs, dbsf_refined=dref, dbsf=dbsf, dxs=dxs)


# ---- inputs with ties everywhere ------------------------------------------------------------------------------------------
VALUES = np.array([-2.0, -1.0, -0.5, 0.25, 0.5, 1.0, 1.5], F32)     # exact in bf16 and fp16


def tied(shape, seed, values=VALUES):
    """An array drawn from a handful of 16-bit values, so that equal neighbours are everywhere."""
    rng = np.random.RandomState(seed)
    return values[rng.randint(0, len(values), size=shape)].astype(F32)


def planted(xs):
    """Plant, in place, in every level: channel 0 of image 0 all negative and rising along rows and columns in steps of
    1/64 (modulo 64), so that the maximum of nearly every window is its LAST element and a running maximum started at 0
    fails; channel 1 all equal, so that the first element of every window takes the whole gradient."""
    for x in xs:
        yy, xx = np.meshgrid(np.arange(x.shape[2]), np.arange(x.shape[3]), indexing="ij")
        x[0, 0] = -1.0 - (63 - (yy + xx) % 64) / 64.0
        if x.shape[1] > 1:
            x[:, 1] = 0.25
    return xs
