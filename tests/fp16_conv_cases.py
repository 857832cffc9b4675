"""Case tables and CPU-side constructions of the float16 conv-family tests (test_fp16_conv_cases_oracle.py on the CPU,
test_gpu_fp16_conv.py on the GPU).  Pure CPU, torch only.

Five parts:
  1. every generic tile of csrc/conv_igemm.hip (TDN_GEMM_CFGS) forced on ONE shape that every tile divides and that
     leaves a partial last M tile for every BM;
  2. the LDS-patch ("halo") kernel's configurations on the smallest shapes that reach every id;
  3. the other conv routes (grouped, dilated, the FPN epilogues, the ReLU6 knee of a 16-bit store);
  4. range edges with EXACTLY known answers: inputs whose every product is a multiple of one power-of-two quantum and
     whose sums stay below 2^24 quanta, so that the fp32 accumulator is exact in any summation order and the stored
     16-bit value must equal ``exact.to(float32).to(dtype)`` bit for bit;
  5. poison confinement: one NaN / +inf input element may change only the outputs whose receptive field holds it.

Every expectation is derived here from the format definitions and the conv geometry, none is read off a run.
"""
import collections
import functools
import itertools

import torch
import torch.nn.functional as F

import bound_util as B
from golden_util import det_tensor

H16, BF16 = torch.float16, torch.bfloat16
DTYPES = collections.OrderedDict([("f16", H16), ("bf16", BF16)])


def q(t, dtype):
    """Make ``t`` representable in ``dtype`` (fp32 container)."""
    return t.to(dtype).float()


def ints(shape, seed, lo, hi):
    """Deterministic integers in [lo, hi] as float32."""
    return det_tensor(shape, seed, lo, hi + 1, bf16=False).floor().clamp_(lo, hi)


def signed_12(shape, seed):
    """Deterministic values in {-2, -1, 1, 2}: no zeros."""
    v = ints(shape, seed, 0, 3)
    return (1.0 + (v % 2)) * (1.0 - 2.0 * (v >= 2).float())


def conv_out(h, k, s, pad, d=1):
    return (h + 2 * pad - (d * (k - 1) + 1)) // s + 1


# ---- part 1: the generic tiles -------------------------------------------------------------------------------------------
# id -> (BM, BN, BK) of TDN_GEMM_CFGS (csrc/conv_igemm.hip); ids are names, not row numbers
TILES = collections.OrderedDict([(0, (64, 64, 64)), (1, (64, 128, 64)), (2, (128, 128, 64)), (3, (192, 256, 64)),
                                 (25, (64, 64, 64)), (46, (128, 128, 64)), (50, (64, 64, 128))])
P1_SHAPE = (3, 9, 11, 256, 256)                     # N, H, W, Cin, Cout
P1_GEOMS = [(1, 1), (3, 1), (3, 2), (1, 2)]         # k, stride (pad = k // 2)
# what today's bf16 lists leave out: the forced dgrad on tiles 0, 1, 2 and tile 2's forward
P1_BF16_DGRAD_TILES = (0, 1, 2)
P1_BF16_FWD_TILES = (2,)


def gemm_dims(kind, N, H, W, Cin, Cout, k, s, pad=None, d=1):
    """The implicit GEMM of a forward (kind 0) or input-gradient (kind 1) launch: {"classes": pixel count of every
    output-parity class (one for a forward or a stride-1 dgrad), "M": the largest, "ngemm", "ktap"} — restating
    build_fwd / build_dgrad of csrc/conv_igemm.hip."""
    pad = k // 2 if pad is None else pad
    if kind == 0:
        classes = [N * conv_out(H, k, s, pad, d) * conv_out(W, k, s, pad, d)]
        ngemm, ktap = Cout, Cin
    else:
        classes = [N * ((H - ph + s - 1) // s) * ((W - pw + s - 1) // s) for ph in range(s) for pw in range(s)]
        ngemm, ktap = Cin, Cout
    return {"classes": classes, "M": max(classes), "ngemm": ngemm, "ktap": ktap}


def tile_divides(tile, ngemm, ktap):
    """choose_cfg's test of a forced tile: BN divides the GEMM's N, BK divides the channels of one tap."""
    _, bn, bk = TILES[tile]
    return ngemm % bn == 0 and ktap % bk == 0


Problem = collections.namedtuple("Problem", "x w scale shift res fwd_bound g w_eff add msk dgrad_bound geom")


@functools.lru_cache(maxsize=None)
def conv_problem(dtname, N, H, W, Cin, Cout, k, s, pad=None, d=1, seed=0):
    """Full-epilogue forward (scale, shift, residual ADD_SAME, ReLU) and dgrad (folded weight, addend, ReLU mask) of
    one conv with its fp64 bounds; operands representable in the element type.  Cached: shared by every tile / config /
    store type that runs the shape, and never modified."""
    dtype = DTYPES[dtname]
    pad = k // 2 if pad is None else pad
    x = q(det_tensor((N, Cin, H, W), seed + 1, -1, 1, bf16=False), dtype)
    w = q(det_tensor((Cout, Cin, k, k), seed + 2, -0.2, 0.2, bf16=False), dtype)
    scale = det_tensor((Cout,), seed + 3, 0.5, 1.5, bf16=False)
    shift = det_tensor((Cout,), seed + 4, -0.5, 0.5, bf16=False)
    Ho, Wo = conv_out(H, k, s, pad, d), conv_out(W, k, s, pad, d)
    res = q(det_tensor((N, Cout, Ho, Wo), seed + 5, -1, 1, bf16=False), dtype)
    fb = B.fwd_bound(x, w, s, pad, scale, shift, res, "same", True, dilation=d)
    g = q(det_tensor((N, Cout, Ho, Wo), seed + 11, -1, 1, bf16=False), dtype)
    w_eff = q(w * scale.view(-1, 1, 1, 1), dtype)          # the folded operand as the launch reads it
    add = q(det_tensor((N, Cin, H, W), seed + 14, -1, 1, bf16=False), dtype)
    msk = q(det_tensor((N, Cin, H, W), seed + 15, -1, 1, bf16=False), dtype)
    db = B.dgrad_bound(g, w_eff, (H, W), s, pad, add, "same", msk, dilation=d)
    return Problem(x, w, scale, shift, res, fb, g, w_eff, add, msk, db, (N, H, W, Cin, Cout, k, s, pad, d))


# ---- part 2: the halo kernel ----------------------------------------------------------------------------------------------
# configuration ids of kHalo3 / kHalo1 (csrc/conv_halo.hip) and the output-channel multiple each needs
CFG3 = collections.OrderedDict([(0, 128), (1, 128), (2, 64), (3, 64), (4, 128), (5, 128), (8, 128), (9, 128), (10, 64),
                                (11, 128)])
CFG1 = collections.OrderedDict([(0, 128), (1, 128), (2, 64), (3, 64), (4, 128), (6, 128), (7, 256), (8, 128), (9, 128),
                                (10, 64)])
HALO3_SHAPES = [(3, 9, 10, 64, 64), (2, 13, 21, 128, 128), (2, 7, 7, 192, 384)]         # N, H, W, Cin, Cout
HALO1_SHAPES = [(1, 20, 24, 64, 256, 1), (1, 12, 16, 256, 512, 2)]                      # ..., stride
HALO_PATCHES = [(3, 42), (10, 12)]
HALO_PATCH_SHAPE = (2, 25, 42, 128, 128)
HALO_EPI_SHAPE = (2, 12, 16, 128)                   # N, H, W, C: dilation 2, ADD_UP2X forward, ADD_SUMPOOL2 dgrad


def halo3_applies(cfg, kind, case):
    """Channel-multiple rule of a 3x3 halo configuration: the GEMM's N (Cout forward, Cin for the input gradient)."""
    return (case[4] if kind == 0 else case[3]) % CFG3[cfg] == 0


def halo1_applies(cfg, case):
    return case[4] % CFG1[cfg] == 0


# Configurations 0 and 8 keep a 7-deep ring of 128-channel weight tiles (112 KB): beside it LDS holds ONE 64-channel
# patch image, so they take a conv only where the GEMM's K is 64 channels and its N a multiple of 128 — none of the three
# shapes above.  The smallest such shape of the bf16 suite, and its transpose for the input gradient, run those two ids.
HALO3_ONE_CHUNK = {0: [(1, 20, 24, 64, 128), (1, 20, 24, 128, 64)], 8: [(1, 20, 24, 64, 128), (1, 20, 24, 128, 64)]}
HALO3_PARAMS = [(cfg, case) for case in HALO3_SHAPES for cfg in CFG3
                if halo3_applies(cfg, 0, case) or halo3_applies(cfg, 1, case)] + \
               [(cfg, case) for cfg, cases in HALO3_ONE_CHUNK.items() for case in cases]
HALO1_PARAMS = [(cfg, case) for case in HALO1_SHAPES for cfg in CFG1 if halo1_applies(cfg, case)]

# ---- part 3: the other routes ------------------------------------------------------------------------------------------------
GROUPED = [(1, 13, 21, 256, 32, 3, 2), (1, 10, 12, 128, 2, 3, 1)]      # N, H, W, C, groups, k, stride
DILATED = [(1, 16, 20, 64, 64, 2, 2), (1, 9, 9, 256, 256, 8, 1)]       # N, H, W, Cin, Cout, dilation, stride
EPI_SHAPE = (2, 8, 12, 64)                                             # N, H, W, C
TOP6 = {H16: 5.99609375, BF16: 5.96875}                                # the largest element value under 6

# ---- part 4: range edges with exactly known answers ------------------------------------------------------------------------
# (name, planted value, exponent e of the channel's quantum 2^e).  A channel's outputs are value + n * 2^e with small
# integers n (n = 0 at EDGE_PIX), so besides the planted value itself its neighbourhood is swept: around 65504 in steps
# of 1 (every value in (65504, 65520) must store as 65504, 65520 and up as inf), through the whole subnormal range in
# steps of 2^-25 (every odd multiple is a tie), around 1 in half-ulp steps.
_SUB = [("2^-14", 2.0 ** -14), ("2^-24", 2.0 ** -24), ("2^-25 tie->0", 2.0 ** -25), ("3*2^-25 tie->2^-23", 3 * 2.0 ** -25),
        ("2^-14-2^-25", 2.0 ** -14 - 2.0 ** -25)]
PLANTS = {
    "f16": [("65504", 65504.0, 0), ("65519->65504", 65519.0, 0), ("65520->inf", 65520.0, 0), ("65536->inf", 65536.0, 0),
            ("-65520->-inf", -65520.0, 0)]
           + [(n, v, -25) for n, v in _SUB] + [("-(" + n + ")", -v, -25) for n, v in _SUB]
           + [("1+2^-11 tie->1", 1 + 2.0 ** -11, -11), ("1+3*2^-11 tie->1+2^-9", 1 + 3 * 2.0 ** -11, -11)],
    "bf16": [("1+2^-8 tie->1", 1 + 2.0 ** -8, -8), ("1+3*2^-8 tie->1+2^-6", 1 + 3 * 2.0 ** -8, -8),
             ("0.5", 0.5, -9)],
}
# the expected bit pattern of every planted value, written down from the format definitions (fp16: 1-5-10, bias 15,
# subnormal unit 2^-24, largest finite 0x7bff = 65504, 0x7c00 = inf; bf16: 1-8-7, bias 127)
PLANT_BITS = {
    "f16": {"65504": 0x7bff, "65519->65504": 0x7bff, "65520->inf": 0x7c00, "65536->inf": 0x7c00, "-65520->-inf": 0xfc00,
            "2^-14": 0x0400, "2^-24": 0x0001, "2^-25 tie->0": 0x0000, "3*2^-25 tie->2^-23": 0x0002,
            "2^-14-2^-25": 0x0400,      # a tie between 0x03ff (odd) and 0x0400 (even): up, to the smallest normal
            "-(2^-14)": 0x8400, "-(2^-24)": 0x8001, "-(2^-25 tie->0)": 0x8000, "-(3*2^-25 tie->2^-23)": 0x8002,
            "-(2^-14-2^-25)": 0x8400,
            "1+2^-11 tie->1": 0x3c00, "1+3*2^-11 tie->1+2^-9": 0x3c02},
    "bf16": {"1+2^-8 tie->1": 0x3f80, "1+3*2^-8 tie->1+2^-6": 0x3f82, "0.5": 0x3f00},
}
RELU6_PLANTS = {"f16": [("relu6 knee", 6.0 - 2.0 ** -9, -12)], "bf16": [("relu6 knee", 6.0 - 2.0 ** -6, -9)]}
EDGE_PIX = (4, 4)
# routes of part 4.  A generic tile runs where it divides 64 input channels (BK = 128 does not) and 64 or 128 output
# channels (BN = 256 does not): Cout = 128 where the tile or halo configuration needs it.
EDGE_TILES = collections.OrderedDict([(0, 64), (25, 64), (1, 128), (2, 128), (46, 128)])      # tile -> GEMM N
EDGE_HALO3 = (5, 128)
EDGE_HALO1 = (2, 64)
EDGE_BLOCK = (1, 8, 16, 64)                         # N, H, W, C of the one-launch bottleneck (x has 4C channels)

Edge = collections.namedtuple("Edge", "x w scale shift exact plants relu k")


def bits16(t):
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xffff


def _zero_block(t, k):
    r = k // 2
    t[:, :, EDGE_PIX[0] - r:EDGE_PIX[0] + r + 1, EDGE_PIX[1] - r:EDGE_PIX[1] + r + 1] = 0
    return t


@functools.lru_cache(maxsize=None)
def edge_fwd(dtname, k, cout, cin=64, H=8, W=8, relu=0):
    """Forward with exactly known answers: x small integers (zero in the k x k window of EDGE_PIX: the conv is 0
    there), w in {+-1, +-2}, per-channel scale 2^e and shift = the planted value.  ``exact`` is fp64 (NCHW), before
    the activation.  ``plants``: [(name, value, channel)] — the value sits at (0, channel, *EDGE_PIX)."""
    table = RELU6_PLANTS[dtname] if relu == 2 else PLANTS[dtname]
    x = _zero_block(ints((1, cin, H, W), 401 + k, -3, 3), k)
    w = signed_12((cout, cin, k, k), 402 + k)
    scale = torch.tensor([2.0 ** table[c % len(table)][2] for c in range(cout)])
    shift = torch.tensor([table[c % len(table)][1] for c in range(cout)], dtype=torch.float64)
    assert torch.equal(shift.float().double(), shift)
    exact = F.conv2d(x.double(), w.double(), None, 1, k // 2) * scale.double().view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    plants = [(table[c % len(table)][0], table[c % len(table)][1], c) for c in range(cout)]
    return Edge(x, w, scale, shift.float(), exact, plants, relu, k)


def representable(v, dtype):
    t = torch.tensor(v, dtype=torch.float64).to(dtype)
    return bool(torch.isfinite(t)) and float(t.double()) == v


NDELTA = 6              # cotangent channels 0..5 carry 2^j at EDGE_PIX: the weights' coefficients compose any small integer


@functools.lru_cache(maxsize=None)
def _compose(value, e, dtype):
    """Coefficients c_j in {+-1, +-2} and a ``dtype``-representable addend a with value = a + 2^e * sum_j c_j 2^j; the
    combination with the smallest |sum| whose sum is not 0 (so the planted value needs the conv's contribution)."""
    best = None
    for cs in itertools.product((1, -1, 2, -2), repeat=NDELTA):
        d = sum(c * 2 ** j for j, c in enumerate(cs))
        a = value - d * 2.0 ** e
        if d != 0 and representable(a, dtype) and (best is None or abs(d) < abs(best[0])):
            best = (d, cs, a)
    assert best is not None, (value, e)
    return best


EdgeD = collections.namedtuple("EdgeD", "g w_eff add exact plants k")
G_UNIT = 2.0 ** -12


@functools.lru_cache(maxsize=None)
def edge_dgrad(dtname, k, cin, cout=64, H=8, W=8):
    """Input gradient with exactly known answers.  g: small integers times 2^-12, zero in the window of EDGE_PIX except
    2^j * 2^-12 in channels j < NDELTA at EDGE_PIX itself; w_eff[co][ci] = +-{1, 2} * 2^(e_ci + 12), all normal numbers;
    addend: one representable value per input channel.  dx = addend + 2^e_ci * integer, and at EDGE_PIX the integer is
    the composed one that makes dx the planted value."""
    dtype = DTYPES[dtname]
    table = PLANTS[dtname]
    g = _zero_block(ints((1, cout, H, W), 411 + k, -3, 3), k) * G_UNIT
    for j in range(NDELTA):
        g[0, j, EDGE_PIX[0], EDGE_PIX[1]] = 2.0 ** j * G_UNIT
    w = signed_12((cout, cin, k, k), 412 + k)
    add = torch.zeros(1, cin, H, W)
    for ci in range(cin):
        _, value, e = table[ci % len(table)]
        _, cs, a = _compose(value, e, dtype)
        w[:NDELTA, ci, k // 2, k // 2] = torch.tensor(cs, dtype=torch.float32)
        w[:, ci] *= 2.0 ** e / G_UNIT
        add[0, ci] = a
    assert torch.equal(q(g, dtype), g) and torch.equal(q(w, dtype), w) and torch.equal(q(add, dtype), add)
    assert float(w.abs().min()) >= (2.0 ** -14 if dtype == H16 else 2.0 ** -126)       # no subnormal operand here
    exact = F.conv_transpose2d(g.double(), w.double(), None, 1, k // 2) + add.double()
    plants = [(table[c % len(table)][0], table[c % len(table)][1], c) for c in range(cin)]
    return EdgeD(g, w, add, exact, plants, k)


def expected16(exact, dtype, relu=0):
    """The one correct stored tensor: activation on the exact value (ReLU6 as relu6_top of csrc/common.h defines it:
    6 from 6 up, otherwise at most the largest element value under 6), one rounding to fp32 (exact here, asserted by
    the CPU-side test), one round-to-nearest-even to the storage type."""
    v = exact
    if relu:
        v = v.clamp(min=0)
    if relu == 2:
        v = torch.where(v >= 6, torch.full_like(v, 6.0), v.clamp(max=TOP6[dtype]))
    return v.float().to(dtype)


@functools.lru_cache(maxsize=None)
def subnormal_operands(k, cout=64, cin=64, H=8, W=8):
    """fp16 subnormal operands: values m * 2^-24, m in 1..1023 (every one below the smallest normal 2^-14), against
    weights in {+-1, +-2}.  Returns (values NCHW, w OIHW, exact forward fp64, exact dgrad fp64) — the values serve as x
    of the forward and as g of the input gradient (cin == cout)."""
    assert cin == cout
    v = ints((1, cin, H, W), 421 + k, 1, 1023) * 2.0 ** -24
    w = signed_12((cout, cin, k, k), 422 + k)
    fwd = F.conv2d(v.double(), w.double(), None, 1, k // 2)
    dg = F.conv_transpose2d(v.double(), w.double(), None, 1, k // 2)
    return v, w, fwd, dg


# ---- part 5: poison confinement ---------------------------------------------------------------------------------------------
POISON_TILES = (0, 3, 25, 50)
POISON_HALO = (5, (2, 13, 21, 128, 128))
POISON_BLOCK = (2, 13, 21, 64)
POISON_CH = 5                                        # the poisoned channel of the pixel


def poison_positions(N, H, W):
    """(name, (n, h, w)): an interior pixel (even coordinates: a stride-2 1x1 conv reads it), a corner, the last pixel
    of the last image."""
    return [("interior", (N // 2, H // 2 // 2 * 2, W // 2 // 2 * 2)), ("corner", (0, 0, 0)),
            ("last", (N - 1, H - 1, W - 1))]


def field_fwd(in_shape, pos, k, s, pad, d=1):
    """Bool (N, Ho, Wo): the outputs whose receptive field holds input pixel ``pos`` = (n, h, w)."""
    N, H, W = in_shape
    ind = torch.zeros(N, 1, H, W, dtype=torch.float64)
    ind[pos[0], 0, pos[1], pos[2]] = 1
    return F.conv2d(ind, torch.ones(1, 1, k, k, dtype=torch.float64), None, s, pad, d)[:, 0] > 0


def field_dgrad(in_shape, pos, k, s, pad, d=1):
    """Bool (N, H, W): the input-gradient pixels that cotangent pixel ``pos`` (in the (N, Ho, Wo) grid) scatters to —
    the adjoint's footprint."""
    N, H, W = in_shape
    Ho, Wo = conv_out(H, k, s, pad, d), conv_out(W, k, s, pad, d)
    ind = torch.zeros(N, 1, Ho, Wo, dtype=torch.float64)
    ind[pos[0], 0, pos[1], pos[2]] = 1
    op = (H - ((Ho - 1) * s - 2 * pad + d * (k - 1) + 1), W - ((Wo - 1) * s - 2 * pad + d * (k - 1) + 1))
    return F.conv_transpose2d(ind, torch.ones(1, 1, k, k, dtype=torch.float64), None, s, pad, op, 1, d)[:, 0] > 0


def field_fwd_loops(in_shape, pos, k, s, pad, d=1):
    """The same set from the definition: output (oh, ow) reads input (oh * s - pad + kh * d, ow * s - pad + kw * d)."""
    N, H, W = in_shape
    Ho, Wo = conv_out(H, k, s, pad, d), conv_out(W, k, s, pad, d)
    m = torch.zeros(N, Ho, Wo, dtype=torch.bool)
    for oh in range(Ho):
        for ow in range(Wo):
            for kh in range(k):
                for kw in range(k):
                    if (oh * s - pad + kh * d, ow * s - pad + kw * d) == (pos[1], pos[2]):
                        m[pos[0], oh, ow] = True
    return m


def field_dgrad_loops(in_shape, pos, k, s, pad, d=1):
    N, H, W = in_shape
    m = torch.zeros(N, H, W, dtype=torch.bool)
    for kh in range(k):
        for kw in range(k):
            h, w = pos[1] * s - pad + kh * d, pos[2] * s - pad + kw * d
            if 0 <= h < H and 0 <= w < W:
                m[pos[0], h, w] = True
    return m


@functools.lru_cache(maxsize=None)
def poison_problem(dtname, N, H, W, Cin, Cout, k, s):
    """A plain conv with the affine only and weights without zeros: (x, w, scale, shift, g, w_eff); scale > 0."""
    dtype = DTYPES[dtname]
    x = q(det_tensor((N, Cin, H, W), 501, -1, 1, bf16=False), dtype)
    w = det_tensor((Cout, Cin, k, k), 502, -0.2, 0.2, bf16=False)
    w = q(torch.where(w.abs() < 0.02, torch.full_like(w, 0.02), w), dtype)
    scale = det_tensor((Cout,), 503, 0.5, 1.5, bf16=False)
    shift = det_tensor((Cout,), 504, -0.5, 0.5, bf16=False)
    Ho, Wo = conv_out(H, k, s, k // 2), conv_out(W, k, s, k // 2)
    g = q(det_tensor((N, Cout, Ho, Wo), 505, -1, 1, bf16=False), dtype)
    return x, w, scale, shift, g, w
