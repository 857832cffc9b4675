"""Inputs of the deformable-convolution tests (tests/test_gpu_deform.py, tests/test_deform_oracle.py): NumPy only.

Offsets are N(0, 3 px) with 5 % of the (n, g, k) planes (at least one) replaced by U(-40, 40): most samples stay inside
the map, a visible share lands across the border or far outside.  Every value is exactly representable in the 16-bit type
it is made for, so the float32 and the 16-bit copy of an operand hold the same numbers."""
import numpy as np
import torch

import deform_ref as R

# ((H, W), stride, pad = dilation)
GEOMETRIES = [((13, 19), 1, 1), ((13, 19), 2, 1), ((13, 19), 1, 2), ((26, 37), 2, 2), ((9, 11), 1, 1)]
# (C, deformable groups)
CHANNELS = [(64, 1), (64, 2), (64, 4), (128, 1)]
N, COUT = 2, 64
SHARE = (0.5, 0.9)         # the in-range share of samples every test asserts first


class Case(object):
    pass


def make(seed, hw, stride, pad, C, dg, dtype, n=N, cout=COUT):
    """x (N, C, H, W), offset (N, 18 dg, Ho, Wo), mask in (0, 1) and logit (N, 9 dg, Ho, Wo), weight (Cout, C, 3, 3), bias,
    dcol (N, Ho, Wo, 9, C), gy (N, Cout, Ho, Wo): float32 arrays of values representable in ``dtype``."""
    rng = np.random.default_rng([seed, hw[0], hw[1], stride, pad, C, dg])
    H, W = hw
    Ho, Wo = R.out_size(H, stride, pad), R.out_size(W, stride, pad)
    c = Case()
    c.H, c.W, c.Ho, c.Wo, c.stride, c.pad, c.C, c.dg, c.N, c.Cout, c.dtype = H, W, Ho, Wo, stride, pad, C, dg, n, cout, dtype
    r16 = lambda a: R.round16(a, dtype)
    c.x = r16(rng.standard_normal((n, C, H, W)))
    off = rng.standard_normal((n, dg, 9, 2, Ho, Wo)) * 3.0
    planes = n * dg * 9
    far = rng.choice(planes, size=max(1, int(round(0.05 * planes))), replace=False)
    for p in far:
        off[p // (dg * 9), (p // 9) % dg, p % 9] = rng.uniform(-40.0, 40.0, size=(2, Ho, Wo))
    c.offset = r16(off.reshape(n, 18 * dg, Ho, Wo))
    c.mask = r16(rng.uniform(0.05, 1.0, size=(n, 9 * dg, Ho, Wo)))
    c.logit = r16(rng.standard_normal((n, 9 * dg, Ho, Wo)) * 2.0)
    c.weight = r16(rng.standard_normal((cout, C, 3, 3)) / np.sqrt(9.0 * C))
    c.bias = rng.standard_normal(cout).astype(np.float32)
    c.dcol = r16(rng.standard_normal((n, Ho, Wo, 9, C)))
    c.gy = r16(rng.standard_normal((n, cout, Ho, Wo)))
    return c


def one_pixel_offsets(c, y=3, x=4, frac=(0.25, 0.625)):
    """Offsets that put every sample of ``c`` at (y + frac[0], x + frac[1]): all four corners of all samples are the
    pixels (y, x) .. (y + 1, x + 1); with frac = (0, 0) every sample lands on pixel (y, x) alone."""
    k = np.arange(9)
    by = np.arange(c.Ho)[None, :, None] * c.stride - c.pad + (k // 3)[:, None, None] * c.pad
    bx = np.arange(c.Wo)[None, None, :] * c.stride - c.pad + (k % 3)[:, None, None] * c.pad
    off = np.zeros((c.N, c.dg, 9, 2, c.Ho, c.Wo), dtype=np.float32)
    off[:, :, :, 0] = (y + frac[0]) - by
    off[:, :, :, 1] = (x + frac[1]) - bx
    return off.reshape(c.N, 18 * c.dg, c.Ho, c.Wo)


def t16(a, dtype, device=None):
    """float32 array -> 16-bit torch tensor (exact for the arrays of ``make``)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(device or "cpu")


def nhwc(a, dtype, device):
    """(N, C, H, W) array -> logical (N, C, H, W) tensor of ``dtype`` (torch.float32 allowed) in channels_last memory"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)))
    return t.to(dtype).to(device).permute(0, 3, 1, 2)
