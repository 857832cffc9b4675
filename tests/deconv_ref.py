"""fp64 oracle of the 2x2 stride-2 transposed convolution (csrc/deconv.hip) and its a-priori rounding
bounds (test infrastructure; pure CPU, torch only).

The taps of the layer do not overlap, so it IS a linear layer over the input pixels: with ``x2d`` (M, Cin) the input
pixels in memory order, ``w2d(weight)`` (4 Cout, Cin) and the output ``unshuffle``d to (M, 4 Cout) in column order
(a, b, o), forward, input gradient, weight gradient and bias gradient are ``linear_ref.fwd / dgrad / wgrad`` on those
matrices, and the allowances are ``linear_ref``'s bounds on them: no tolerance of this file's own.

Conventions.  Activations are NHWC tensors — ``x`` (R, H, W, Cin), ``y`` and ``g`` (R, 2H, 2W, Cout) — fp32 containers of
16-bit values; ``weight`` is (Cin, Cout, 2, 2) as ``nn.ConvTranspose2d`` holds it, already rounded (``round16``).
"""
import torch

import linear_ref as L

round16 = L.round16
within = L.within


def unshuffle(y):
    """NHWC (R, 2H, 2W, Cout) -> (M, 4 Cout): row (r, i, j), column (a * 2 + b) * Cout + o = y[r, 2i+a, 2j+b, o]."""
    R, H2, W2, C = y.shape
    H, W = H2 // 2, W2 // 2
    return y.reshape(R, H, 2, W, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(R * H * W, 4 * C)


def shuffle(Y, R, H, W):
    """inverse of ``unshuffle``: (M, 4 Cout) -> NHWC (R, 2H, 2W, Cout)."""
    C = Y.shape[1] // 4
    return Y.reshape(R, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(R, 2 * H, 2 * W, C)


def w2d(weight):
    """(Cin, Cout, 2, 2) -> (4 Cout, Cin), row (a * 2 + b) * Cout + o."""
    Cin, Cout = weight.shape[:2]
    return weight.permute(2, 3, 1, 0).reshape(4 * Cout, Cin)


def w4d(m):
    """inverse of ``w2d``: (4 Cout, Cin) -> (Cin, Cout, 2, 2)."""
    Cin = m.shape[1]
    return m.reshape(2, 2, m.shape[0] // 4, Cin).permute(3, 2, 0, 1)


def x2d(x):
    return x.reshape(-1, x.shape[-1])


def _b4(b):
    return None if b is None else b.repeat(4)


def fwd(x, weight, b=None, relu=False):
    """-> y NHWC (R, 2H, 2W, Cout), fp64."""
    R, H, W, _ = x.shape
    return shuffle(L.fwd(x2d(x), w2d(weight), _b4(b), relu), R, H, W)


def dgrad(g, weight):
    """-> dx NHWC (R, H, W, Cin), fp64."""
    R, H2, W2, _ = g.shape
    return L.dgrad(unshuffle(g), w2d(weight)).reshape(R, H2 // 2, W2 // 2, weight.shape[0])


def wgrad(x, g):
    """-> (dw (Cin, Cout, 2, 2), dbias (Cout,)), fp64."""
    dw, _ = L.wgrad(x2d(x), unshuffle(g))
    g4 = g.reshape(-1, g.shape[-1])                  # the cotangent as (4M, Cout): its column sums are dbias
    return w4d(dw), L.wgrad(torch.zeros(g4.shape[0], 1), g4)[1]


def fwd_bound(x, weight, b=None, relu=False, cheap=False):
    """Bound of ``unshuffle(y)`` (M, 4 Cout, 1, 1)."""
    return L.fwd_bound(x2d(x), w2d(weight), _b4(b), relu, cheap=cheap)


def dgrad_bound(g, weight, cheap=False):
    """Bound of ``x2d(dx)`` (M, Cin, 1, 1)."""
    return L.dgrad_bound(unshuffle(g), w2d(weight), cheap=cheap)


def wgrad_bound(x, g, cheap=False, mult=1.0):
    """Bound of ``w2d(dw)`` (4 Cout, Cin, 1, 1)."""
    return L.wgrad_bound(x2d(x), unshuffle(g), cheap=cheap, mult=mult)


def dbias_bound(g, mult=1.0):
    """Bound of dbias (Cout, 1, 1, 1): the cotangent viewed as (4M, Cout)."""
    return L.dbias_bound(g.reshape(-1, g.shape[-1]), mult=mult)
