"""Inputs of the GHM tests (tests/test_ghm_oracle.py on the CPU, tests/test_gpu_ghm.py on the GPU): random heads and
targets whose gradient norms are PLACED (drawn inside the bins, away from the edges, and inverted to logits / deltas),
and the boundary inputs: for every interior edge the two adjacent representable values of a storage type between which
the oracle's bin changes, found by bisection on the float ordering.
"""
import numpy as np

import ghm_ref as R
from loss_ref import unflatten_head

f32 = np.float32
LEVELS = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 1)]
MARGIN = 1e-5                 # what the float64 restatement needs between a gradient norm and an edge
PLACE = 0.05                  # placed norms keep this fraction of a bin's width from both of its edges


def placed_g(rng, shape, bins):
    """Gradient norms drawn bin by bin (uniform over the bins, so the easy and the hard ones are all met), each at least
    PLACE of the bin's width from the bin's edges and at least 1e-3 from 0 and 1."""
    b = rng.integers(0, bins, shape)
    frac = rng.uniform(PLACE, 1 - PLACE, shape)
    return np.clip((b + frac) / bins, 1e-3, 1 - 1e-3)


def case(B, A, C, levels, seed, bins_cls=30, bins_reg=10, mu=0.02, poison=True, valid=0.7, pos=0.05):
    """-> (cls, reg, labels, lw, bt, bw): float32 numpy head outputs per level and ``anchor_target_all``-shaped targets.
    Weights take the values 0, 0.5, 1 and 2 (only > 0 matters); with ``poison`` the logits under weight 0 hold NaN / Inf."""
    rng = np.random.default_rng(seed)
    N = sum(h * w for h, w in levels) * A
    labels = np.where(rng.random((B, N)) < pos, rng.integers(1, C + 1, (B, N)), 0).astype(np.int64)
    labels[:, ::7] = rng.integers(1, C + 1, labels[:, ::7].shape)              # positives on every level
    lw = rng.choice(np.array([0, 0.5, 1, 2], f32), (B, N), p=[1 - valid, 0.1, valid - 0.2, 0.1])
    lw[:, 0] = 1                                                               # the 1 x 1 level's neighbours stay valid
    lw[:, -A:] = 1
    bt = rng.normal(0, 0.3, (B, N, 4)).astype(f32)
    bw = np.where((labels > 0)[..., None], rng.choice(np.array([1, 0.5], f32), (B, N, 4)), 0).astype(f32)
    bw[:, 1::11, 2] = 0                                                        # a positive with one coordinate switched off
    cls, reg, n0 = [], [], 0
    for h, w in levels:
        n1 = n0 + h * w * A
        t = labels[:, n0:n1, None] == np.arange(1, C + 1)[None, None, :]
        g = placed_g(rng, t.shape, bins_cls)
        x = np.log(g / (1 - g))                                               # sigma(x) = g; a target wants sigma(-x) = g
        x = np.where(t, -x, x).astype(f32)
        g = placed_g(rng, (B, n1 - n0, 4), bins_reg)
        d = mu * g / np.sqrt(1 - g * g) * rng.choice([-1.0, 1.0], g.shape)
        p = (bt[:, n0:n1].astype(np.float64) + d).astype(f32)
        if poison:
            w0 = np.broadcast_to((lw[:, n0:n1] <= 0)[..., None], x.shape)
            x = np.where(w0, rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], f32), x.shape), x).astype(f32)
            b0 = bw[:, n0:n1] <= 0
            p = np.where(b0 & (rng.random(b0.shape) < 0.5), f32(np.nan), p).astype(f32)
        cls.append(unflatten_head(x, A, C, h, w))
        reg.append(unflatten_head(p, A, 4, h, w))
        n0 = n1
    return cls, reg, labels, lw, bt, bw


# ---- the float ordering of a storage type ---------------------------------------------------------------------------
KINDS = {"f32": (np.uint32, 32), "bf16": (np.uint16, 16), "f16": (np.uint16, 16)}


def from_key(key, dt):
    """key >= 0: the non-negative value whose bit pattern is key; key < 0: minus the value of -key.  -> float32."""
    key = np.asarray(key, np.int64)
    mag = np.abs(key)
    if dt == "f32":
        v = mag.astype(np.uint32).view(f32)
    elif dt == "bf16":
        v = (mag.astype(np.uint32) << np.uint32(16)).view(f32)
    else:
        v = mag.astype(np.uint16).view(np.float16).astype(f32)
    return np.where(key < 0, -v, v).astype(f32)


def to_key(v, dt):
    """The key of a float32 value that the storage type holds exactly."""
    v = f32(v)
    a = np.abs(v)
    if dt == "f32":
        k = int(np.asarray(a, f32).view(np.uint32))
    elif dt == "bf16":
        k = int(np.asarray(a, f32).view(np.uint32)) >> 16
    else:
        k = int(np.asarray(a, np.float16).view(np.uint16))
    return -k if v < 0 else k


def _bisect(bin_at, lo, hi, bins):
    """For every interior edge i in 1..bins-1 the adjacent keys (k - 1, k) with bin_at(k - 1) < i <= bin_at(k); bin_at
    is monotone from bin 0 at ``lo`` to bin bins - 1 at ``hi`` (asserted at the ends and at the crossing)."""
    want = np.arange(1, bins)
    lo = np.full(bins - 1, lo, np.int64)
    hi = np.full(bins - 1, hi, np.int64)
    assert np.all(bin_at(lo) == 0) and np.all(bin_at(hi) == bins - 1)
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        up = bin_at(mid) >= want
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    assert np.array_equal(bin_at(lo), want - 1) and np.array_equal(bin_at(hi), want), "no clean crossing"
    return lo, hi


def cls_crossings(bins, dt, t):
    """-> float32 logits (2, bins - 1): row 0 the last input in bin i - 1, row 1 the first in bin i, for every interior
    edge i; for a target element (t) the inputs are mirrored, so that the rows mean the same."""
    def bin_at(key):
        x = from_key(key, dt)
        return R.bin_of(R.elem_cls(-x if t else x, np.full(x.shape, t))[0], bins)
    lo, hi = _bisect(bin_at, to_key(-60.0, dt), to_key(60.0, dt), bins)
    x = np.stack([from_key(lo, dt), from_key(hi, dt)])
    return (-x if t else x).astype(f32)


def reg_crossings(bins, dt, mu, sign):
    """The same for GHM-R: deltas d = sign * |d| against a target of 0."""
    def bin_at(key):
        return R.bin_of(R.elem_reg(from_key(key, dt) * f32(sign), f32(0), mu)[0], bins, True)
    lo, hi = _bisect(bin_at, 0, to_key(1000.0, dt), bins)
    return (np.stack([from_key(lo, dt), from_key(hi, dt)]) * f32(sign)).astype(f32)
