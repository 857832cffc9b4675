"""Input recipes of the element-wise oracle tests (tests/test_elementwise_oracle.py checks, on the CPU, that each
recipe meets the condition it is used for; tests/test_gpu_elementwise.py feeds them to the kernels).  Pure CPU.
"""
import torch

from golden_util import _hash_u01, det_tensor

DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
MANT = {torch.bfloat16: 8, torch.float16: 11}          # significand bits, hidden one included


def grid(shape, seed, lo, hi, step):
    """Deterministic multiples of ``step`` in [lo, hi] (fp32): few levels, so ties are common and 16-bit exact."""
    return (det_tensor(shape, seed, lo, hi, bf16=False) / step).round() * step


def _f32(vals):
    return torch.tensor(vals, dtype=torch.float64).float()


def _next(t, up):
    """The fp32 neighbour of each (positive, finite) value."""
    return (t.view(torch.int32) + (1 if up else -1)).view(torch.float32)


# ---- rounding at the fp32 -> 16-bit boundary ------------------------------------------------------------------------
TABLE_LEN = 4608            # = 3 * 32 * 48 = 64 * 8 * 3 * 3; the special values come first


def rounding_classes():
    """name -> fp32 tensor of the positive special values of that class (the table holds them with both signs)."""
    cls = {}
    for dtype, tag, exps in ((torch.bfloat16, "bf16", (-60, -14, -3, 0, 1, 7, 15, 60)),
                             (torch.float16, "f16", (-14, -3, 0, 1, 7, 15))):
        p = MANT[dtype]
        even, odd = [], []
        for e in exps:
            ulp = 2.0 ** (e - (p - 1))
            for m in (0, 2, 2 ** (p - 1) - 4):          # even significands: 1.0, 1 + 2 ulp, the last but one
                even.append(2.0 ** e + m * ulp + ulp / 2)
                odd.append(2.0 ** e + (m + 1) * ulp + ulp / 2)
        cls[tag + "_mid_even"] = _f32(even)              # exact midpoints, the lower neighbour even / odd
        cls[tag + "_mid_odd"] = _f32(odd)
        mids = torch.cat([cls[tag + "_mid_even"], cls[tag + "_mid_odd"]])
        cls[tag + "_mid_minus"] = _next(mids, False)     # one fp32 ulp below / above a midpoint
        cls[tag + "_mid_plus"] = _next(mids, True)
    bmax = torch.tensor([0x7f7f0000], dtype=torch.int32).view(torch.float32)        # largest finite bf16
    binf = torch.tensor([0x7f7f8000], dtype=torch.int32).view(torch.float32)        # first fp32 that rounds to inf
    cls["bf16_max"] = torch.cat([bmax, _next(binf, False)])
    cls["bf16_to_inf"] = torch.cat([binf, _next(binf, True)])
    h = _f32([65520.0])
    cls["f16_max"] = torch.cat([_f32([65504.0, 65519.996]), _next(h, False)])
    cls["f16_to_inf"] = torch.cat([h, _next(h, True), _f32([65536.0, 1e6])])
    q = 2.0 ** -24                                       # fp16 subnormal spacing; every input here is an fp32 NORMAL
    cls["f16_sub"] = _f32([k * q for k in (1, 2, 3, 5, 512, 1022, 1023, 1024)])
    sub_mid = _f32([q / 2, 1.5 * q, 2.5 * q, 3.5 * q, 1022.5 * q, 1023.5 * q])
    cls["f16_sub_mid"] = sub_mid                         # 2^-25 -> 0, 3 * 2^-25 -> 2^-23, ..., 1023.5 q -> 2^-14
    cls["f16_sub_near"] = torch.cat([_next(sub_mid, False), _next(sub_mid, True), _f32([q / 4, 0.75 * q])])
    return cls


def rounding_table():
    """TABLE_LEN fp32 values: the special classes with both signs, +-0, +-inf, a NaN, then ``det_tensor(bf16=False)``
    values at three magnitudes.  No fp32 subnormal."""
    sp = torch.cat(list(rounding_classes().values()))
    sp = torch.cat([sp, -sp, torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])])
    n = TABLE_LEN - sp.numel()
    assert n >= 3000, n
    rnd = det_tensor((n,), 4242, -3, 3, bf16=False)
    k = torch.arange(n) % 3
    rnd = rnd * torch.where(k == 0, 1.0, torch.where(k == 1, 2.0 ** -11, 2.0 ** 12)).float()
    t = torch.cat([sp, rnd]).contiguous()
    assert t.numel() == TABLE_LEN and t.dtype == torch.float32
    return t


def finite_table():
    """The table with its five non-finite entries replaced (weights of the scaled dgrad operands)."""
    t = rounding_table()
    return torch.where(torch.isfinite(t), t, torch.full_like(t, 1.4142135))


# ---- max pool -------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 8), (1, 1, 7, 8), (1, 7, 1, 8), (1, 2, 2, 8), (2, 3, 5, 24), (1, 15, 21, 64), (2, 16, 24, 72)]
POOL_KINDS = ["relu", "signed", "special"]


def pool_input(kind, shape, seed=51):
    """NCHW pool input of an (N, H, W, C) case.  'relu': the tie-heavy post-ReLU recipe of test_gpu_kernels.test_maxpool;
    'signed': half-integers in [-4, 1], most windows have a negative or zero maximum; 'special': the signed recipe with
    NaN (1 in 37) and -inf (1 in 5) sprinkled in and the whole corner window (0, 0) at -inf."""
    N, H, W, C = shape
    if kind == "relu":
        return torch.relu((det_tensor((N, C, H, W), seed, -2, 2) * 2).round() / 2)
    x = grid((N, C, H, W), seed + 1, -4, 1, 0.5)
    if kind == "signed":
        return x
    u = torch.from_numpy(_hash_u01(x.numel(), seed + 2)).view(x.shape)
    x = torch.where(u < 0.2, torch.full_like(x, float("-inf")), x)
    x = torch.where(u > 1 - 1.0 / 37, torch.full_like(x, float("nan")), x)
    x[:, :, :2, :2] = float("-inf")
    return x


# ---- per-channel affine ---------------------------------------------------------------------------------------------
def affine_vectors(C, seed):
    """fp32 (scale, shift, mean, invstd), not 16-bit representable."""
    return tuple(det_tensor((C,), seed + j, lo, hi, bf16=False)
                 for j, (lo, hi) in enumerate(((0.5, 1.5), (-0.5, 0.5), (-0.2, 0.2), (0.7, 1.4))))


def affine_exact_inputs(C, npix, seed=7):
    """(g, x, mean) of the exactly summable recipe, NCHW with N = 1, H = 1: g multiples of 2^-4 in [-2, 2], x multiples
    of 2^-3 in [-4, 4], mean multiples of 2^-3 in [-1, 1].  Every g and every g * (x - mean) is a multiple of 2^-7 below
    16, so a sum of fewer than 2048 of them has under 2^22 levels: exact in fp32 in any order, with or without fma."""
    assert npix < 2048
    g = grid((1, C, 1, npix), seed, -2, 2, 2.0 ** -4)
    x = grid((1, C, 1, npix), seed + 1, -4, 4, 2.0 ** -3)
    mean = grid((C,), seed + 2, -1, 1, 2.0 ** -3)
    return g, x, mean


def relu6_knee_inputs(C, npix, seed=9):
    """(x, scale, shift), NCHW with N = 1, H = 1, for the ReLU6 knee: scale in {1, 1/2, 2}, x multiples of 1/4 — half of
    them exactly 6 / scale —, shift an ODD multiple of 2^-10 in (-2^-5, 2^-5).  Every pre-activation is an odd multiple
    of 2^-10 (never 0 or 6, exact in fp32 with or without fma), and those of the x = 6 / scale elements walk through
    (5.96875, 6) — the channels with shift -1 and -3 times 2^-10 also through (5.99609375, 6) — and through
    (6, 6.03125)."""
    c = torch.arange(C)
    scale = torch.tensor([1.0, 0.5, 2.0])[c % 3]
    shift = ((2 * ((c * 5) % 32) - 31).float() / 1024.0)
    shift = torch.where(c % 4 == 0, ((2 * (c // 4 % 4) - 3).float() / 1024.0), shift)     # -3, -1, 1, 3 (x 2^-10)
    x = grid((1, C, 1, npix), seed, -4, 12, 0.25)
    u = torch.from_numpy(_hash_u01(x.numel(), seed + 1)).view(x.shape)
    x = torch.where(u < 0.5, (6.0 / scale).view(1, C, 1, 1).expand_as(x), x)
    return x.contiguous(), scale, shift


AFFINE_BWD_CASES = [(8, 1), (8, 513), (24, 5), (24, 1537), (64, 511), (64, 512), (320, 513), (1600, 37), (2048, 513),
                    (2112, 1025), (4104, 513)]

