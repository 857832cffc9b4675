"""CPU proof that tests/bound_util.py is right (valid evaluations stay inside the bound) and has teeth (single-element
defects that the old norm-wise metric accepts are rejected).  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import bound_util as B
from golden_util import det_tensor, rel_l2

DTYPES = [torch.bfloat16, torch.float16]


def q(t, dtype):
    return t.to(dtype).float()


# ---- rounding ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_half_ulp16_matches_the_neighbours(dtype):
    """Every positive finite value of the type (normal, subnormal, power-of-two boundaries) and its upper neighbour:
    their distance is twice half_ulp16 anywhere in [x, next), and just below a power of two the spacing halves."""
    bits = torch.arange(0, 0x7F80 if dtype == torch.bfloat16 else 0x7C00, dtype=torch.int16)
    x = bits.view(dtype).double()
    nxt, x = x[1:], x[:-1]                                   # the last finite value has no finite neighbour
    gap = nxt - x
    assert bool((gap > 0).all())
    assert torch.equal(B.half_ulp16(x, dtype) * 2, gap)
    assert torch.equal(B.half_ulp16(x + gap * 0.5, dtype) * 2, gap)          # the midpoint rounds within this gap
    assert torch.equal(B.half_ulp16(x + gap * 0.999, dtype) * 2, gap)
    assert torch.equal(B.half_ulp16(-x, dtype), B.half_ulp16(x, dtype))
    # a round-to-nearest store never moves a value further than half_ulp16 of it
    v = det_tensor((1 << 16,), 5, -4, 4, bf16=False).double() * torch.logspace(-9, 3, 1 << 16, dtype=torch.float64)
    assert bool(((v.float().to(dtype).double() - v.float().double()).abs() <= B.half_ulp16(v.float(), dtype)).all())
    # subnormal floor
    tiny = 2.0 ** -133 if dtype == torch.bfloat16 else 2.0 ** -24
    assert float(B.half_ulp16(torch.zeros(1), dtype)) == tiny / 2 == float(B.half_ulp16(torch.tensor([tiny]), dtype))


# ---- the reference alone stays inside the bound ------------------------------------------------------------------
GEOMS = [(1, 1, 0), (3, 1, 1), (3, 2, 1), (7, 2, 3)]      # k, stride, pad


def _fwd_variants(x, w, s, p):
    """Three valid fp32 evaluations of conv(x, w): torch's, channel order reversed, K in 4 chunks."""
    yield "torch", F.conv2d(x, w, None, s, p)
    yield "reversed", F.conv2d(x.flip(1).contiguous(), w.flip(1).contiguous(), None, s, p)
    acc = None
    for xc, wc in zip(x.chunk(4, 1), w.chunk(4, 1)):
        part = F.conv2d(xc.contiguous(), wc.contiguous(), None, s, p)
        acc = part if acc is None else acc + part
    yield "chunked", acc


def _dgrad_variants(g, w, s, p, op):
    yield "torch", F.conv_transpose2d(g, w, None, s, p, op)
    yield "reversed", F.conv_transpose2d(g.flip(1).contiguous(), w.flip(0).contiguous(), None, s, p, op)
    acc = None
    for gc, wc in zip(g.chunk(4, 1), w.chunk(4, 0)):
        part = F.conv_transpose2d(gc.contiguous(), wc.contiguous(), None, s, p, op)
        acc = part if acc is None else acc + part
    yield "chunked", acc


def _case(k, dtype, Cin=None, Cout=64, N=2, H=19, W=26):
    Cin = Cin or (4 if k == 7 else 64)
    x = q(det_tensor((N, Cin, H, W), 1, -1, 1, bf16=False), dtype)
    w = q(det_tensor((Cout, Cin, k, k), 2, -0.2, 0.2, bf16=False), dtype)
    scale = det_tensor((Cout,), 3, 0.5, 1.5, bf16=False)
    shift = det_tensor((Cout,), 4, -0.5, 0.5, bf16=False)
    return x, w, scale, shift


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("k,s,p", GEOMS)
def test_reference_forward_inside_bound(k, s, p, dtype):
    x, w, scale, shift = _case(k, dtype)
    Ho, Wo = (x.shape[2] + 2 * p - k) // s + 1, (x.shape[3] + 2 * p - k) // s + 1
    res = q(det_tensor((x.shape[0], w.shape[0], Ho, Wo), 5, -1, 1, bf16=False), dtype)
    b = B.fwd_bound(x, w, s, p, scale, shift, res, "same", True)
    cheap = B.fwd_bound(x, w, s, p, scale, shift, res, "same", True, cheap=True, conv32=True)
    assert bool((cheap.S >= b.S).all()), "Cauchy-Schwarz bound below S"
    assert bool(((cheap.v - b.v).abs() <= cheap.R).all()), "fp32 reference outside its own error term"
    for name, c in _fwd_variants(x, w, s, p):
        y = F.relu(c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res)       # fp32 epilogue
        for bound in (b, cheap):
            B.assert_within(y, bound, torch.float32, name)
            B.assert_within(y.to(dtype), bound, dtype, name + " 16-bit")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("k,s,p", GEOMS)
def test_reference_dgrad_inside_bound(k, s, p, dtype):
    x, w, scale, _ = _case(k, dtype)
    N, Cin, H, W = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = q(det_tensor((N, w.shape[0], Ho, Wo), 11, -1, 1, bf16=False), dtype)
    wd = q(w * scale.view(-1, 1, 1, 1), dtype)
    add = q(det_tensor((N, Cin, H, W), 14, -1, 1, bf16=False), dtype)
    msk = det_tensor((N, Cin, H, W), 15, -1, 1)
    op = (H - ((Ho - 1) * s - 2 * p + k), W - ((Wo - 1) * s - 2 * p + k))
    b = B.dgrad_bound(g, wd, (H, W), s, p, add, "same", msk)
    cheap = B.dgrad_bound(g, wd, (H, W), s, p, add, "same", msk, cheap=True, conv32=True)
    assert bool((cheap.S >= b.S).all())
    assert bool(((cheap.v - b.v).abs() <= cheap.R).all())
    for name, c in _dgrad_variants(g, wd, s, p, op):
        dx = (c + add) * (msk > 0).float()
        for bound in (b, cheap):
            B.assert_within(dx, bound, torch.float32, name)
            B.assert_within(dx.to(dtype), bound, dtype, name + " 16-bit")
    # the FPN adjoint's 2x2 sum-pool addend
    fine = q(det_tensor((N, Cin, 2 * H, 2 * W), 16, -1, 1, bf16=False), dtype)
    b2 = B.dgrad_bound(g, wd, (H, W), s, p, fine, "sumpool")
    assert b2.T == w.shape[0] * k * k + 4
    B.assert_within(F.conv_transpose2d(g, wd, None, s, p, op) + F.avg_pool2d(fine, 2) * 4, b2, torch.float32)


def test_reference_long_k_and_bn_fold_inside_bound():
    """Cin = 2048 (layer4's 1x1 convs) with a non-trivial BN fold: gamma, beta, running statistics -> scale, shift."""
    x = F.relu(det_tensor((2, 2048, 13, 21), 21, -1, 1))
    w = det_tensor((128, 2048, 1, 1), 22, -0.05, 0.05)
    gamma, beta = det_tensor((128,), 23, 0.5, 1.5, bf16=False), det_tensor((128,), 24, -0.1, 0.1, bf16=False)
    mean, var = det_tensor((128,), 25, -0.1, 0.1, bf16=False), det_tensor((128,), 26, 0.5, 1.5, bf16=False)
    scale = gamma / torch.sqrt(var + 1e-5)
    shift = beta - mean * scale
    b = B.fwd_bound(x, w, 1, 0, scale, shift, relu=True)
    assert b.T == 2048 + 2
    cheap = B.fwd_bound(x, w, 1, 0, scale, shift, relu=True, cheap=True, conv32=True)
    assert bool((cheap.S >= b.S).all())
    worst = 0.0
    for name, c in _fwd_variants(x, w, 1, 0):
        y = F.relu(c * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
        worst = max(worst, B.assert_within(y, b, torch.float32, name)["ratio"])
        B.assert_within(y.bfloat16(), b, torch.bfloat16, name)
        B.assert_within(y.bfloat16(), cheap, torch.bfloat16, name)
    assert worst < 0.5          # round-to-nearest (2^-24) chains against a 2^-23 allowance


def test_one_launch_deep_residual_inside_bound():
    """conv3 + BN + residual + ReLU where the residual is the downsample launch recomputed on the CPU: the 'GPU' side
    (another valid evaluation order, its own 16-bit residual) stays inside the bound once operand_slack — derived, not
    measured — is added."""
    dtype = torch.bfloat16
    bx = F.relu(det_tensor((2, 64, 20, 24), 31, -1, 1))
    h2 = F.relu(det_tensor((2, 64, 20, 24), 32, -1, 1))
    wdn, w3 = det_tensor((256, 64, 1, 1), 33, -0.2, 0.2), det_tensor((256, 64, 1, 1), 34, -0.2, 0.2)
    sd, bd, s3, b3 = (det_tensor((256,), 35 + i, lo, hi, bf16=False) for i, (lo, hi) in
                      enumerate(((0.5, 1.5), (-0.1, 0.1), (0.5, 1.5), (-0.1, 0.1))))
    aff = lambda c, s, b: c * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)      # noqa: E731
    bd_ = B.fwd_bound(bx, wdn, 1, 0, sd, bd)
    res_cpu = q(aff(F.conv2d(bx, wdn), sd, bd), dtype)                                       # what the oracle uses
    res_gpu = q(aff(list(_fwd_variants(bx, wdn, 1, 0))[2][1], sd, bd), dtype)                # what the GPU used
    extra = B.operand_slack(bd_, dtype)
    assert bool(((res_gpu - res_cpu).abs().double() <= extra).all())
    b = B.fwd_bound(h2, w3, 1, 0, s3, b3, res_cpu, "same", True)
    out_gpu = F.relu(aff(list(_fwd_variants(h2, w3, 1, 0))[1][1], s3, b3) + res_gpu).to(dtype)
    B.assert_within(out_gpu, b, dtype, "conv3 + residual", extra=extra)
    assert int((res_gpu != res_cpu).sum()) > 0      # the two residuals do differ somewhere: the case is not vacuous


@pytest.mark.parametrize("k,s,p", [(1, 1, 0), (3, 1, 1), (3, 2, 1)])
def test_reference_wgrad_inside_bound(k, s, p):
    x, w, scale, _ = _case(k, torch.bfloat16)
    N, Cin, H, W = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = det_tensor((N, w.shape[0], Ho, Wo), 41, -1, 1)
    b = B.wgrad_bound(x, g, w.shape, s, p, scale)
    cheap = B.wgrad_bound(x, g, w.shape, s, p, scale, cheap=True)
    assert b.T == N * Ho * Wo + 1 and bool((cheap.S >= b.S).all())
    assert bool(((cheap.v - b.v).abs() <= cheap.R).all())
    G = torch.nn.grad.conv2d_weight(x, w.shape, g, s, p) * scale.view(-1, 1, 1, 1)
    G2 = sum(torch.nn.grad.conv2d_weight(x[i:i + 1], w.shape, g[i:i + 1], s, p) for i in range(N)) * scale.view(-1, 1, 1, 1)
    for got in (G, G2):
        r = B.assert_within(got, b, torch.float32, "dw")
        assert r["where"] == "weights"
        B.assert_within(got, cheap, torch.float32, "dw")


# ---- mutations: rejected by the checker, accepted by rel_l2 <= 1e-3 ----------------------------------------------
OLD_TOL = 1e-3
MN, MC, MH, MW = 2, 4, 1200, 1600        # 3.84e6 pixels, 1.5e7 elements (a pixel of O(1) errors stays under 1e-3 in L2)


@pytest.fixture(scope="module")
def conv3():
    """A 3x3 conv + BN + ReLU launch stored in bf16: operands, the pre-activation, the bound and an honest result."""
    x = det_tensor((MN, 8, MH, MW), 51, -1, 1)
    w = det_tensor((MC, 8, 3, 3), 52, -0.2, 0.2)
    scale = det_tensor((MC,), 53, 0.5, 1.5, bf16=False)
    shift = det_tensor((MC,), 54, -0.5, 0.5, bf16=False)
    b = B.fwd_bound(x, w, 1, 1, scale, shift, relu=True)
    pre = F.conv2d(x, w, None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    good = F.relu(pre).bfloat16()
    ref = b.v.float().bfloat16().float()            # what the old metric compares with: the rounded reference
    assert good.numel() >= 1e6
    assert B.check(good, b, torch.bfloat16)["ratio"] <= 1.0
    return {"x": x, "w": w, "scale": scale, "shift": shift, "b": b, "pre": pre, "good": good, "ref": ref}


def _rejected(bad, c, index, dtype=torch.bfloat16):
    old = rel_l2(bad.float(), c["ref"])
    assert old <= OLD_TOL, "the old metric was meant to accept this: %g" % old
    r = B.check(bad, c["b"], dtype)
    assert r["ratio"] > 1.0, r
    assert tuple(r["index"][:1] + r["index"][2:]) == tuple(index[:1] + index[2:]), (r["index"], index)
    with pytest.raises(AssertionError) as e:
        B.assert_within(bad, c["b"], dtype, "mutant")
    assert str(tuple(r["index"])) in str(e.value)           # the failure message names the element
    return r


def test_mutation_right_neighbour(conv3):
    bad = conv3["good"].clone()
    bad[0, 2, 100, 200] = bad[0, 2, 100, 201]
    assert _rejected(bad, conv3, [0, 2, 100, 200])["index"] == [0, 2, 100, 200]


def test_mutation_zeroed_element(conv3):
    good = conv3["good"]
    med = float(good.float().abs().flatten()[::97].median())
    flat = good.flatten()
    i = 1234567 + int((flat[1234567:].float().abs() > med).nonzero()[0])      # first above-median element from there
    bad = flat.clone()
    bad[i] = 0
    idx = list(int(v) for v in torch.unravel_index(torch.tensor(i), good.shape))
    assert _rejected(bad.view_as(good), conv3, idx)["index"] == idx


def test_mutation_dropped_tap_on_a_border_pixel(conv3):
    """The pixel (h, w) = (0, 700) of image 1 computed without its (kh, kw) = (1, 2) tap — a valid tap there."""
    x, w, c = conv3["x"], conv3["w"], conv3
    n, h, wq = 1, 0, 700
    tap = (w[:, :, 1, 2] * x[n, :, h + 1 - 1, wq + 2 - 1].view(1, -1)).sum(1)
    conv = (c["pre"][n, :, h, wq] - c["shift"]) / c["scale"]
    bad = c["good"].clone()
    bad[n, :, h, wq] = F.relu((conv - tap) * c["scale"] + c["shift"]).bfloat16()
    r = _rejected(bad, c, [n, 0, h, wq])
    assert "image border" in r["where"]


def test_mutation_swapped_channels(conv3):
    bad = conv3["good"].clone()
    bad[1, 1, 640, 77], bad[1, 2, 640, 77] = conv3["good"][1, 2, 640, 77], conv3["good"][1, 1, 640, 77]
    _rejected(bad, conv3, [1, 1, 640, 77])


def test_mutation_image_boundary(conv3):
    bad = conv3["good"].clone()
    bad[0, :, MH - 1, MW - 1] = bad[1, :, 0, 0]
    r = _rejected(bad, conv3, [0, 0, MH - 1, MW - 1])
    assert "image boundary in M" in r["where"] and "last row" in r["where"] and "last column" in r["where"]


def test_mutation_missing_relu(conv3):
    pre = conv3["pre"].flatten()
    med = float(pre.abs()[::97].median())
    i = 7654321 + int((pre[7654321:] < -med).nonzero()[0])                   # a negative pre-activation, not a tiny one
    bad = conv3["good"].flatten().clone()
    assert float(bad[i]) == 0.0
    bad[i] = pre[i].bfloat16()
    idx = list(int(v) for v in torch.unravel_index(torch.tensor(i), conv3["good"].shape))
    assert _rejected(bad.view_as(conv3["good"]), conv3, idx)["index"] == idx


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_mutation_four_ulp16(dtype):
    """One element of a K = 64 1x1 output moved by 4 ulp16 (the old 16-bit allowance, 2^-7 relative, is 4 bf16 ulps)."""
    x = q(det_tensor((2, 64, 96, 96), 61, -1, 1, bf16=False), dtype)
    w = q(det_tensor((64, 64, 1, 1), 62, -0.2, 0.2, bf16=False), dtype)
    b = B.fwd_bound(x, w)
    good = F.conv2d(x, w).to(dtype)
    assert good.numel() >= 1e6 and b.T == 64
    assert B.check(good, b, dtype)["ratio"] <= 1.0
    c = {"b": b, "ref": b.v.float().to(dtype).float()}
    for idx, step in (([1, 17, 40, 41], 4), ([0, 63, 95, 95], -4)):
        bad = good.clone()
        bits = bad.view(torch.int16)
        assert abs(float(good[tuple(idx)])) > 2.0 ** -10
        bits[tuple(idx)] += step                           # 4 representable values away, same sign
        assert _rejected(bad, c, idx, dtype)["index"] == idx
