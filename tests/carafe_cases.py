"""Inputs of the CARAFE tests (tests/test_gpu_carafe.py, tests/test_carafe_oracle.py): NumPy only.

The case list is the smallest set of shapes at which the kernels can go wrong: a 1 x 1 map, a map narrower than the
window, a ragged single tile, more than one tile ragged both ways; every (kernel size, scale) the library takes on the
second and the last of those; every (C, group) split; the three crops with and without an addend; both 16-bit types;
weights in float32 and in the compute dtype.  Logits are U(-4, 4): the softmax is neither flat nor one-hot.  Every value is
exactly representable in the 16-bit type it is made for, so the float32 and the 16-bit copy of an operand hold the same
numbers."""
import numpy as np
import torch

import carafe_ref as R

SIZES = [(1, 1), (2, 3), (7, 9), (13, 17)]
KS = [(5, 2), (3, 2), (1, 2), (7, 2), (5, 1), (3, 3), (3, 4)]
CHANNELS = [(64, 1), (128, 2), (192, 1), (64, 8)]
MAX_WEIGHT_CHANNELS = 1024
BF16, F16 = torch.bfloat16, torch.float16


class Case(object):
    def __repr__(self):
        return self.id


def _spec(i, hw, k, s, C, g):
    c = Case()
    c.H, c.W, c.k, c.s, c.C, c.g = hw[0], hw[1], k, s, C, g
    c.N = 2 if hw[0] * hw[1] <= 63 else 1
    c.dtype = (BF16, F16)[i % 2]
    c.w32 = (i // 2) % 2 == 0                        # masks / logits in float32, else in the compute dtype
    crop = i % 3                                     # (sH, sW), (sH - 1, sW), (sH - 1, sW - 1); no crop at scale 1
    sH, sW = c.H * s, c.W * s
    c.out_size = (sH - (crop >= 1 and s > 1), sW - (crop >= 2 and s > 1))
    c.with_addend = (i // 3) % 2 == 1
    c.seed = i
    c.id = "%dx%d-k%d-s%d-C%d-g%d-%s-%s-o%dx%d%s" % (c.H, c.W, k, s, C, g, str(c.dtype).split(".")[-1][:4],
                                                   "w32" if c.w32 else "w16", c.out_size[0], c.out_size[1],
                                                   "-add" if c.with_addend else "")
    return c


def _specs():
    out = []
    geos = [(hw, 5, 2) for hw in SIZES] + [(hw, k, s) for k, s in KS[1:] for hw in (SIZES[1], SIZES[3])]
    for gi, (hw, k, s) in enumerate(geos):
        fits = [(C, g) for C, g in CHANNELS if g * k * k * s * s <= MAX_WEIGHT_CHANNELS]
        chans = fits if (k, s) == (5, 2) else [fits[gi % len(fits)]]
        for C, g in chans:
            out.append(_spec(len(out), hw, k, s, C, g))
    return out


CASES = _specs()


def make(c):
    """Fills ``c`` with float32 arrays of values representable in ``c.dtype``: x (N, C, H, W), logits (N, g k^2 s^2, H, W),
    masks (N, g k^2, sH, sW) — the rounded softmax of the logits —, gout and addend (N, C, Ho, Wo)."""
    rng = np.random.default_rng([c.seed, c.H, c.W, c.k, c.s, c.C, c.g])
    r16 = lambda a: R.round16(a, c.dtype)
    Ho, Wo = c.out_size
    c.x = r16(rng.standard_normal((c.N, c.C, c.H, c.W)))
    c.logits = r16(rng.uniform(-4.0, 4.0, size=(c.N, c.g * c.k * c.k * c.s * c.s, c.H, c.W)))
    c.masks = r16(R.normalize(c.logits, c.k, c.g, c.s))
    c.gout = r16(rng.standard_normal((c.N, c.C, Ho, Wo)))
    c.addend = r16(rng.standard_normal((c.N, c.C, Ho, Wo))) if c.with_addend else None
    return c


def custom(N, C, g, hw, k, s, dtype, seed=0, out_size=None, with_addend=False, w32=True):
    c = Case()
    c.N, c.C, c.g, c.H, c.W, c.k, c.s, c.dtype, c.seed, c.w32 = N, C, g, hw[0], hw[1], k, s, dtype, seed, w32
    c.out_size = (hw[0] * s, hw[1] * s) if out_size is None else tuple(out_size)
    c.with_addend = with_addend
    c.id = "custom"
    return make(c)


def nhwc(a, dtype, device):
    """(N, C, H, W) array -> logical (N, C, H, W) tensor of ``dtype`` (torch.float32 allowed) in channels_last memory"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32).transpose(0, 2, 3, 1)))
    return t.to(dtype).to(device).permute(0, 3, 1, 2)
