"""tests/elementwise_ref.py — the oracle the GPU tests of csrc/elementwise.hip compare with — against independent
references (PyTorch float64 ops and autograd, permute + explicit zero fill, literal arrays), the proof that its
comparison helpers fail when they should, and the conditions the input recipes of tests/elementwise_cases.py promise.
CPU only.
"""
import pytest
import torch
import torch.nn.functional as F

import bound_util as B
import elementwise_cases as EC
import elementwise_ref as R
from golden_util import det_tensor

NAN, INF = float("nan"), float("inf")


def _codes_from_torch(flat, H, W):
    """Flat h * W + w index of F.max_pool2d(..., return_indices=True) -> window code kh * 3 + kw."""
    Ho, Wo = flat.shape[2:]
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    kh = flat // W - (2 * ho - 1)
    kw = flat % W - (2 * wo - 1)
    assert bool(((kh >= 0) & (kh < 3) & (kw >= 0) & (kw < 3)).all())
    return (kh * 3 + kw).to(torch.uint8)


# ---- the oracle against independent references ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", EC.POOL_KINDS)
@pytest.mark.parametrize("shape", EC.POOL_SHAPES)
def test_pool_forward_vs_torch_float64(shape, kind):
    x = EC.pool_input(kind, shape)
    N, H, W, C = shape
    y, code = R.maxpool3x3s2_fwd(x)
    ty, ti = F.max_pool2d(x.double(), 3, 2, 1, return_indices=True)
    R.assert_bits(y.v, ty, "pool values %s %s" % (shape, kind))
    R.assert_bits(code, _codes_from_torch(ti, H, W), "pool codes %s %s" % (shape, kind))
    if kind == "special":
        assert bool(torch.isnan(y.v).any()) or H * W <= 7                   # the smallest planes are the -inf corner
        assert bool((y.v[:, :, 0, 0] == -INF).all()) and bool((code[:, :, 0, 0] == 4).all())    # first in-bounds: (1, 1)
    if kind == "signed" and H > 2:
        assert bool((y.v <= 0).any())


def test_pool_nan_rule_is_pytorchs():
    """NaNs at (1, 1) and (2, 2) of a 5 x 5 plane: window (1, 1) covers rows / columns 1..3, the later NaN wins — flat
    index 2 * 5 + 2 = 12, code (2 - 1) * 3 + (2 - 1) = 4 — and F.max_pool2d agrees."""
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 1, 1] = NAN
    x[0, 0, 2, 2] = NAN
    y, code = R.maxpool3x3s2_fwd(x)
    ty, ti = F.max_pool2d(x.double(), 3, 2, 1, return_indices=True)
    assert int(ti[0, 0, 1, 1]) == 12 and int(code[0, 0, 1, 1]) == 4      # (2, 2) of the plane = (1, 1) of window (1, 1)
    assert int(ti[0, 0, 0, 0]) == 6 and int(code[0, 0, 0, 0]) == 8       # window (0, 0): NaN at its last position
    R.assert_bits(code, _codes_from_torch(ti, 5, 5), "codes")
    R.assert_bits(y.v, ty, "values")


@pytest.mark.parametrize("dtype", EC.DTYPES, ids=EC.DT_IDS)
@pytest.mark.parametrize("shape", EC.POOL_SHAPES)
def test_pool_adjoint_vs_float64_autograd(shape, dtype):
    N, H, W, C = shape
    x = EC.pool_input("relu", shape).double().requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    _, code = R.maxpool3x3s2_fwd(x.detach())
    # on the grid: every sum of <= 4 multiples of 1/8 below 2 is exact — the chain EQUALS autograd
    dy = EC.grid(tuple(y.shape), 52, -1, 1, 0.125)
    (gx,) = torch.autograd.grad(y, x, dy.double(), retain_graph=True)
    ref = R.maxpool3x3s2_bwd(dy, code, (H, W), dtype)
    R.assert_bits(ref.v, gx, "float64 adjoint")
    R.assert_bits(ref.bits.double(), gx, "fp32 chain on the grid")
    # off the grid: the UN-ROUNDED fp32 chain lies within 4 * 2^-24 * sum|dy| of it (no ulp term), and the expected bits
    # are that accumulator rounded once
    dy = det_tensor(tuple(y.shape), 53, -1, 1, bf16=False).to(dtype).float()
    (gx,) = torch.autograd.grad(y, x, dy.double(), retain_graph=True)
    (ga,) = torch.autograd.grad(y, x, dy.double().abs())
    ref = R.maxpool3x3s2_bwd(dy, code, (H, W), dtype)
    R.assert_bits(ref.v, gx, "float64 adjoint")
    assert ref.acc32.dtype == torch.float32
    assert bool(((ref.acc32.double() - gx).abs() <= 4 * 2.0 ** -24 * ga).all())
    R.assert_bits(ref.bits, R.r16(ref.acc32, dtype), "bits = the accumulator rounded once")
    # the masks
    xm = x.detach()
    for kw in (dict(mask_src=xm), dict(pooled=y.detach())):
        R.assert_bits(R.maxpool3x3s2_bwd(dy, code, (H, W), dtype, **kw).v, torch.where(xm > 0, gx, 0.0), str(list(kw)))


def test_affine_backward_vs_float64_autograd():
    C, npix = 24, 37
    g = det_tensor((1, C, 1, npix), 1, -1, 1)
    x = det_tensor((1, C, 1, npix), 2, -2, 2)
    gamma, beta, mean, var = (det_tensor((C,), 3 + j, lo, hi, bf16=False).double()
                              for j, (lo, hi) in enumerate(((0.5, 1.5), (-1, 1), (-1, 1), (0.5, 1.5))))
    gamma.requires_grad_(True)
    beta.requires_grad_(True)
    xd = x.double().requires_grad_(True)
    eps = 1e-5
    F.batch_norm(xd, mean, var, gamma, beta, False, 0.0, eps).backward(g.double())
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = (gamma.detach() * invstd)
    # the oracle takes fp32 vectors: hand it float64-exact ones by rounding the inputs of BOTH sides first
    sc32, mu32, is32 = scale.float(), mean.float(), invstd.float()
    dx, db, dg, s1 = R.channel_affine_bwd(g, x, sc32, mu32, is32, torch.bfloat16)
    assert torch.allclose(dx.v, xd.grad, rtol=1e-6, atol=0)
    assert torch.allclose(db.v, beta.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dg.v, gamma.grad, rtol=1e-6, atol=1e-9)        # fp32-rounded mean / invstd on our side
    assert torch.allclose(s1 * is32.double(), dg.v, rtol=0, atol=0)
    assert db.T == npix + 2 and dg.T == npix + 2 and bool((dg.S >= dg.v.abs()).all())
    R.assert_bits(dx.bits, (g * sc32.view(1, -1, 1, 1)).bfloat16().float(), "dx chain")


def _gconv_loops(w, groups, scale16):
    """Block-diagonal operands by explicit loops over groups (independent of the index arithmetic of the oracle)."""
    C, cpg, kh, kw = w.shape
    f = torch.zeros(C, kh, kw, 64, dtype=w.dtype)
    d = torch.zeros(C, kh, kw, 64, dtype=w.dtype)
    for gi in range(groups):
        for o in range(cpg):
            co = gi * cpg + o
            for l in range(cpg):
                ci = gi * cpg + l
                f[co, :, :, ci % 64] = w[co, l]                 # the row of output channel co, slot of input ci
                d[ci, :, :, co % 64] = scale16[co, l]           # the row of input channel ci, slot of output co
    return f, d


@pytest.mark.parametrize("dtype", EC.DTYPES, ids=EC.DT_IDS)
def test_packers_vs_permute_and_zero_fill(dtype):
    for C, groups, k in ((64, 32, 3), (128, 32, 1), (64, 1, 1), (128, 2, 3)):
        w = det_tensor((C, C // groups, k, k), 10 + C + groups, -1, 1, bf16=False)
        scale = det_tensor((C,), 11, 0.5, 1.5, bf16=False)
        fwd, dg = R.pack_gconv_weight(w, groups, dtype, scale)
        w16 = w.to(dtype).float()
        ws16 = (w16 * scale.view(-1, 1, 1, 1)).to(dtype).float()
        f, d = _gconv_loops(w16, groups, ws16)
        R.assert_bits(fwd.bits, f, "gconv w_fwd %s" % ((C, groups, k),))
        R.assert_bits(dg.bits, d, "gconv w_dgrad %s" % ((C, groups, k),))
        R.assert_bits(fwd.v, _gconv_loops(w.double(), groups, w.double())[0], "gconv w_fwd float64")
        assert float(fwd.bits.abs().sum()) > 0 and int((fwd.bits == 0).sum()) >= C * k * k * (64 - C // groups)
    w = det_tensor((5, 3, 7, 7), 12, -1, 1, bf16=False)
    z = torch.zeros(5, 7, 8, 4)
    for co in range(5):
        for c in range(3):
            z[co, :, :7, c] = w[co, c].to(dtype).float()
    R.assert_bits(R.pack_stem_weight(w, dtype).bits, z, "stem")
    w = det_tensor((6, 4, 3, 2), 13, -1, 1, bf16=False)
    scale = det_tensor((6,), 14, 0.5, 1.5, bf16=False)
    fwd, dg = R.pack_conv_weight(w, dtype, scale)
    R.assert_bits(fwd.bits, w.to(dtype).float().permute(0, 2, 3, 1), "w_fwd")
    R.assert_bits(dg.bits, (w.to(dtype).float() * scale.view(-1, 1, 1, 1)).to(dtype).float().permute(1, 2, 3, 0), "w_dg")
    img = det_tensor((2, 3, 5, 7), 15, -3, 3, bf16=False)
    st = R.stage_image(img, dtype).bits
    assert tuple(st.shape) == (2, 11, 15, 4)
    R.assert_bits(st[:, 3:8, 3:10, :3], img.to(dtype).float().permute(0, 2, 3, 1), "staged interior")
    assert float(st.abs().sum()) == float(st[:, 3:8, 3:10, :3].abs().sum())


def test_literal_cases():
    bf = torch.bfloat16
    one = torch.tensor([[[[3.0]]]])
    y, code = R.maxpool3x3s2_fwd(one)                                   # 1 x 1: the only pixel is position (1, 1)
    assert y.v.tolist() == [[[[3.0]]]] and code.tolist() == [[[[4]]]]
    x = torch.tensor([[[[1.0, 2.0], [2.0, -1.0]]]])                     # 2 x 2: one window, first 2.0 is (1, 2) = 5
    y, code = R.maxpool3x3s2_fwd(x)
    assert y.v.tolist() == [[[[2.0]]]] and code.tolist() == [[[[5]]]]
    dx = R.maxpool3x3s2_bwd(torch.tensor([[[[0.5]]]]), code, (2, 2), bf)
    assert dx.bits.tolist() == [[[[0.0, 0.5], [0.0, 0.0]]]] and dx.v.tolist() == dx.bits.tolist()
    assert R.maxpool3x3s2_bwd(torch.tensor([[[[0.5]]]]), code, (2, 2), bf, mask_src=-x).bits.abs().sum() == 0
    assert R.subsample2_fwd(x).bits.tolist() == [[[[1.0]]]]
    sb = R.subsample2_bwd(torch.tensor([[[[0.25]]]]), (2, 2), bf, dx_in=x)
    assert sb.bits.tolist() == [[[[1.25, 2.0], [2.0, -1.0]]]]
    assert R.subsample2_bwd(torch.tensor([[[[-0.0]]]]), (1, 1), bf).bits.view(torch.int32).tolist() == [[[[0]]]]
    # 1 + 2^-8 is a bf16 tie: 1.0 + 2^-8 in fp32, then to even
    a = R.add_relu_mask(torch.tensor([[[[1.0, 1.0]]]]), bf, torch.tensor([[[[2.0 ** -8, 3 * 2.0 ** -8]]]]))
    assert a.bits.tolist() == [[[[1.0, 1.015625]]]]
    a = R.add_relu_mask(x, bf, x, mask_src=torch.tensor([[[[1.0, 0.0], [-1.0, 2.0]]]]))
    assert a.bits.tolist() == [[[[2.0, 0.0], [0.0, -2.0]]]]
    h = R.add_relu_mask(torch.tensor([[[[60000.0]]]]), torch.float16, torch.tensor([[[[60000.0]]]]))
    assert h.bits.tolist() == [[[[INF]]]] and h.v.tolist() == [[[[120000.0]]]]
    assert R.clamp_max_(torch.tensor([7.0, 6.0, -0.0, 5.5]), 6.0).bits.tolist() == [6.0, 6.0, -0.0, 5.5]
    assert R.act_mask(torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([0.0, 5.5, 6.0, -1.0]), 6.0).bits.tolist() == \
        [0.0, 2.0, 0.0, 0.0]
    # the rounding facts the whole file rests on
    f = torch.tensor([65520.0, 65519.996, 2.0 ** -25, 3 * 2.0 ** -25]).half().float().tolist()
    assert f == [INF, 65504.0, 0.0, 2.0 ** -23]
    assert torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]).bfloat16().float().tolist() == [1.0, 1.015625]
    b, pre = R.channel_affine_fwd(torch.tensor([[[[5.98, 6.0, 7.0, -1.0]]]]), torch.ones(1), torch.zeros(1), 2, bf)
    assert b.v.flatten().tolist() == [5.96875, 6.0, 6.0, 0.0] and b.T == 2


# ---- the comparisons have teeth -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", EC.DTYPES, ids=EC.DT_IDS)
def test_teeth_one_ulp_and_signed_zero(dtype):
    want = det_tensor((2, 3, 4, 5), 1, -1, 1, bf16=False).to(dtype)
    R.assert_bits(want.clone(), want, "same")
    R.assert_bits(want.float(), want, "fp32 container")
    got = want.clone()
    got.view(torch.int16)[1, 2, 3, 4] += 1                               # one 16-bit ulp
    with pytest.raises(AssertionError, match=r"first at \(n, c, h, w\) = \(1, 2, 3, 4\)"):
        R.assert_nchw(got, want, "moved")
    with pytest.raises(AssertionError, match=r"first at index = \(1, 2, 3, 4\)"):
        R.assert_bits(got, want, "moved, layout unknown")
    z = torch.zeros(1, 1, 1, 2, dtype=dtype)
    with pytest.raises(AssertionError):
        R.assert_bits(-z, z, "signed zero")
    n = torch.full((1, 1, 1, 2), NAN, dtype=dtype)
    R.assert_bits(n, (-n.float()).to(dtype), "any NaN matches any NaN")
    with pytest.raises(AssertionError):
        R.assert_bits(n, z, "NaN against a number")
    # and the Bound: dbeta with one pixel dropped
    g, x, mean = EC.affine_exact_inputs(8, 513)
    sc, _, _, inv = EC.affine_vectors(8, 3)
    _, db, _, _ = R.channel_affine_bwd(g, x, sc, mean, inv, dtype)
    B.assert_within(db.v.float(), db, torch.float32, "dbeta")
    k = int(g[0, :, 0, 0].abs().argmax())
    assert float(g[0, k, 0, 0]) != 0
    with pytest.raises(AssertionError, match="dbeta"):
        B.assert_within((db.v - g[0, :, 0, 0].double()).float(), db, torch.float32, "dbeta")


def test_teeth_last_max_rule():
    x = EC.pool_input("relu", (1, 15, 21, 64))
    first, last = R.maxpool3x3s2_fwd(x)[1], R.maxpool3x3s2_fwd(x, last_max=True)[1]
    assert int((first != last).sum()) > 100                               # the recipe really has ties
    with pytest.raises(AssertionError):
        R.assert_bits(last, first, "last max")


@pytest.mark.parametrize("dtype", EC.DTYPES, ids=EC.DT_IDS)
def test_teeth_descending_sum(dtype):
    """An input where the order matters: pixel (1, 1) is the maximum of its four windows, whose dy in ascending
    (ho, wo) order are (B, s, s, -B) with B = 2^12 and s = 2^-12, half an fp32 ulp of B.  Ascending: B + s ties to
    even (B), again B, minus B: 0.  Descending: -B + s and (-B + s) + s are exact, plus B: 2^-11 — the exact sum."""
    big, small = 2.0 ** 12, 2.0 ** -12
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 1, 1] = 1.0
    _, code = R.maxpool3x3s2_fwd(x)
    assert code[0, 0, :2, :2].tolist() == [[8, 6], [2, 0]]               # all four point at pixel (1, 1)
    dy = torch.zeros(1, 1, 3, 3)
    dy[0, 0, :2, :2] = torch.tensor([[big, small], [small, -big]])
    assert torch.equal(dy.to(dtype).float(), dy)
    up = R.maxpool3x3s2_bwd(dy, code, (5, 5), dtype)
    down = R.maxpool3x3s2_bwd(dy, code, (5, 5), dtype, descending=True)
    assert float(up.bits[0, 0, 1, 1]) == 0.0 and float(down.bits[0, 0, 1, 1]) == 2 * small
    assert float(up.v[0, 0, 1, 1]) == 2 * small
    with pytest.raises(AssertionError, match=r"\(0, 0, 1, 1\)"):
        R.assert_nchw(down.bits, up.bits, "descending")


@pytest.mark.parametrize("dtype", EC.DTYPES, ids=EC.DT_IDS)
def test_teeth_truncation(dtype):
    t = EC.finite_table()
    t = t[(t.abs() > 2.0 ** -14) & (t.abs() < 60000)].view(1, 1, 1, -1)
    want = R.nchw_to_nhwc(t, dtype).bits
    with pytest.raises(AssertionError):
        R.assert_bits(R.trunc16(t, dtype).permute(0, 2, 3, 1), want, "truncated")
    exact = want.permute(0, 3, 1, 2)
    R.assert_bits(R.trunc16(exact, dtype), exact, "representable values survive truncation")


# ---- the recipes meet their conditions ------------------------------------------------------------------------------
@pytest.mark.parametrize("C,npix", EC.AFFINE_BWD_CASES)
def test_exactly_summable_affine_inputs_are_exact(C, npix):
    g, x, mean = EC.affine_exact_inputs(C, npix)
    for dtype in EC.DTYPES:
        assert torch.equal(g.to(dtype).float(), g) and torch.equal(x.to(dtype).float(), x)
    terms = (g * (x - mean.view(1, -1, 1, 1)))                            # fp32
    assert torch.equal(terms.double(), g.double() * (x.double() - mean.double().view(1, -1, 1, 1)))
    for t in (g, terms):
        seq = torch.zeros(C, dtype=torch.float32)
        for p in range(npix):                                             # the fp32 sequential sum
            seq = seq + t[0, :, 0, p]
        assert torch.equal(seq.double(), t.double().sum((0, 2, 3)))
        assert torch.equal(t.flip(3).cumsum(3)[0, :, 0, -1].double(), t.double().sum((0, 2, 3)))


def test_rounding_table_has_every_class():
    t = EC.rounding_table()
    assert t.numel() == EC.TABLE_LEN
    tiny = torch.finfo(torch.float32).tiny
    assert not bool(((t != 0) & (t.abs() < tiny)).any()), "fp32 subnormal in the table"
    assert int(torch.isnan(t).sum()) == 1 and int(torch.isinf(t).sum()) == 2
    z = t[t == 0].view(torch.int32).tolist()
    assert 0 in z and -2 ** 31 in z
    cls = EC.rounding_classes()
    for dtype, tag in zip(EC.DTYPES, EC.DT_IDS):
        for par, name in ((0, "_mid_even"), (1, "_mid_odd")):
            m = cls[tag + name]
            lo = R.trunc16(m, dtype)
            hi = (lo.to(dtype).view(torch.int16) + 1).view(dtype).float()
            assert torch.equal(m.double() - lo.double(), hi.double() - m.double()) and bool((lo < m).all())   # midpoints
            low_bit = lo.to(dtype).view(torch.int16) & 1
            assert bool((low_bit == par).all())
            assert torch.equal(m.to(dtype).float(), hi if par else lo)                    # ties go to the even one
        mids = torch.cat([cls[tag + "_mid_even"], cls[tag + "_mid_odd"]])
        lo = R.trunc16(mids, dtype)
        hi = (lo.to(dtype).view(torch.int16) + 1).view(dtype).float()
        assert torch.equal(cls[tag + "_mid_minus"].to(dtype).float(), lo)
        assert torch.equal(cls[tag + "_mid_plus"].to(dtype).float(), hi)
        assert bool(torch.isfinite(cls[tag + "_max"].to(dtype).float()).all())
        assert torch.equal(cls[tag + "_max"].to(dtype).float(), torch.full((cls[tag + "_max"].numel(),),
                                                                           torch.finfo(dtype).max))
        assert bool(torch.isinf(cls[tag + "_to_inf"].to(dtype).float()).all())
    q = 2.0 ** -24
    sub = torch.cat([cls["f16_sub"], cls["f16_sub_mid"], cls["f16_sub_near"]])
    assert bool((sub >= tiny).all()) and bool((sub.half().float() <= 2.0 ** -14).all())
    assert cls["f16_sub_mid"].half().float().tolist() == [0.0, 2 * q, 2 * q, 4 * q, 1022 * q, 1024 * q]
    assert torch.equal(cls["f16_sub"].half().float(), cls["f16_sub"])
    for name, v in cls.items():                                            # all of it, both signs, is in the table
        for s in (v, -v):
            assert bool((t.view(1, -1) == s.view(-1, 1)).any(1).all()), name
    rnd = t[-3000:]
    for dtype in EC.DTYPES:
        assert float((rnd.to(dtype).float() != rnd).float().mean()) > 0.95              # these all need rounding


@pytest.mark.parametrize("dtype", EC.DTYPES, ids=EC.DT_IDS)
@pytest.mark.parametrize("C", [8, 24, 64, 520])
def test_relu6_inputs_leave_almost_nothing_undecided(C, dtype):
    npix = 37 if C == 520 else 301
    x, scale, shift = EC.relu6_knee_inputs(C, npix)
    assert torch.equal(x.to(dtype).float(), x)
    b, pre = R.channel_affine_fwd(x, scale, shift, 2, dtype)
    lat = pre * 1024
    assert torch.equal(lat, lat.round()) and bool((lat.abs() % 2 == 1).all())             # odd multiples of 2^-10
    assert torch.equal(pre.float().double(), pre)
    near = ((pre - 6).abs() <= b.E) | (pre.abs() <= b.E)
    assert float(near.double().mean()) <= 1e-3 and int(near.sum()) == 0
    assert int(((pre > R.TOP6[dtype]) & (pre < 6)).sum()) >= 300
    assert int((pre >= 6).sum()) >= 300 and int((pre < 0).sum()) > 0
    stored, und = R.knee_resolved(b.v.float(), b, pre, dtype)
    assert und == 0 and bool((stored[pre < 6] < 6).all()) and bool((stored[pre >= 6] == 6).all())
