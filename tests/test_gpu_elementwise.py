"""The kernels of csrc/elementwise.hip against the oracle of tests/elementwise_ref.py, element by element.

Where a kernel is a fixed chain of IEEE fp32 operations the comparison is ``assert_bits`` (NaN matches NaN, -0 is not
+0); where the compiler may contract a multiply-add it is ``bound_util.assert_within`` on every element.  Inputs come
from tests/elementwise_cases.py, whose recipes tests/test_elementwise_oracle.py checks on the CPU.

What is exercised that the parity tests do not reach: rounding of fp32 sources that are NOT 16-bit representable
(midpoints, overflow to inf, fp16 subnormals), the second trip of every grid-stride / tile-stride loop (the sizes are
the smallest that take it: grid_for caps a launch at 4096 x 256 lanes, the transposes at 8192 tiles), every thread
layout of channel_affine_bwd and its beta != 0 path, the pool's window codes, NaN and -inf, the ReLU6 knee, and the
block-diagonal / padded layouts of the grouped and stem weight packers including their zeros.

Not pinned (the project specifies neither behaviour): NaN or inf into channel_affine_*, clamp_max_ and the mask
operand of add_relu_mask (fmaxf / fminf do not propagate NaN); fp32 subnormal sources.
"""
import ctypes

import pytest
import torch

import bound_util as B
import elementwise_cases as EC
import elementwise_ref as R
from golden_util import det_tensor

pytestmark = pytest.mark.gpu

both = pytest.mark.parametrize("dtype", EC.DTYPES, ids=EC.DT_IDS)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from torch_detection_amd import ops as _ops
    from torch_detection_amd import _lib
    _lib.load()
    return _ops


def dev(t, dtype):
    """NCHW fp32 container of 16-bit values (CPU) -> NHWC ``dtype`` on the GPU."""
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def host(t):
    """NHWC on the GPU -> NCHW on the CPU, same element type."""
    return t.cpu().permute(0, 3, 1, 2).contiguous()


def q16(t, dtype):
    return t.to(dtype).float()


# ---- rounding at the fp32 -> 16-bit boundary ------------------------------------------------------------------------
@both
def test_rounding_to_nhwc(ops, dtype):
    t = EC.rounding_table().view(2, 36, 8, 8)
    want = R.nchw_to_nhwc(t, dtype).bits
    g = t.cuda()
    R.assert_bits(ops.to_nhwc_bf16(g, dtype), want, "contiguous source")
    R.assert_bits(ops.to_nhwc_bf16(g.contiguous(memory_format=torch.channels_last), dtype), want, "channels_last")
    wide = torch.full((2, 36, 8, 16), 7.0, device="cuda")
    wide[..., ::2] = g
    src = wide[..., ::2]
    assert not src.is_contiguous()
    R.assert_bits(ops.to_nhwc_bf16(src, dtype), want, "step-2 sliced source")


@both
def test_rounding_stage_image(ops, dtype):
    t = EC.rounding_table().view(1, 3, 32, 48)
    want = R.stage_image(t, dtype).bits
    R.assert_bits(ops.stage_image(t.cuda(), dtype), want, "contiguous image")
    R.assert_bits(ops.stage_image(t.cuda().contiguous(memory_format=torch.channels_last), dtype), want, "channels_last")


@both
def test_rounding_pack_conv_weight(ops, dtype):
    w = EC.rounding_table().view(64, 8, 3, 3)
    want, _ = R.pack_conv_weight(w, dtype)
    for src, nm in ((w.cuda(), "contiguous"), (w.cuda().contiguous(memory_format=torch.channels_last), "channels_last")):
        wf, wd = ops.pack_conv_weight(src, None, False, dtype)
        assert wd is None
        R.assert_bits(wf, want.bits, "w_fwd, %s" % nm)
    # the scaled dgrad operand: fl16(fl32(fl16(w) * scale)), finite weights
    w = EC.finite_table().view(64, 8, 3, 3)
    scale = det_tensor((64,), 21, 0.5, 1.5, bf16=False)
    wf_ref, wd_ref = R.pack_conv_weight(w, dtype, scale)
    for src, nm in ((w.cuda(), "contiguous"), (w.cuda().contiguous(memory_format=torch.channels_last), "channels_last")):
        wf, wd = ops.pack_conv_weight(src, scale.cuda(), True, dtype)
        R.assert_bits(wf, wf_ref.bits, "w_fwd, %s" % nm)
        R.assert_bits(wd, wd_ref.bits, "w_dgrad, %s" % nm)
    _, wd1 = ops.pack_conv_weight(w.cuda(), None, True, dtype)
    R.assert_bits(wd1, R.pack_conv_weight(w, dtype)[1].bits, "w_dgrad without a scale")


@both
def test_rounding_prepare_group(ops, dtype):
    """The grouped launch rounds like the per-layer packer: 64 x 64 tiles of table values, with and without a BN."""
    t = EC.finite_table()
    w1 = t[:4096].reshape(64, 64, 1, 1).contiguous().cuda()
    w3 = t[-2304:].repeat(16).reshape(64, 64, 3, 3).contiguous()
    w3c = w3.cuda().contiguous(memory_format=torch.channels_last)
    bn = tuple(det_tensor((64,), 30 + j, lo, hi, bf16=False).cuda()
               for j, (lo, hi) in enumerate(((0.5, 1.5), (-1, 1), (-1, 1), (0.5, 1.5)))) + (1e-5,)
    scale = ops.bn_fold(*bn)[0].cpu()
    entries = []
    for w, b in ((w1, bn), (w3c, None), (w3.cuda(), bn)):
        O, I, kh, kw = w.shape
        entries.append((w, b, torch.empty(O, kh, kw, I, dtype=dtype, device="cuda"),
                        torch.empty(I, kh, kw, O, dtype=dtype, device="cuda"),
                        torch.empty(3, O, device="cuda") if b else None))
    ops.prepare_group(entries, dtype)
    for i, (w, b, wf, wd, _) in enumerate(entries):
        rf, rd = R.pack_conv_weight(w.cpu(), dtype, scale if b else None)
        R.assert_bits(wf, rf.bits, "prepare_group w_fwd[%d]" % i)
        R.assert_bits(wd, rd.bits, "prepare_group w_dgrad[%d]" % i)


@both
def test_rounding_pack_stem_and_gconv(ops, dtype):
    t = EC.rounding_table()
    ws = t[:147 * 31].reshape(31, 3, 7, 7).contiguous()
    R.assert_bits(ops.pack_stem_weight(ws.cuda(), dtype), R.pack_stem_weight(ws, dtype).bits, "stem")
    wg = t.view(64, 8, 3, 3)
    wf, _ = ops.pack_gconv_weight(wg.cuda(), 8, None, False, dtype)
    R.assert_bits(wf, R.pack_gconv_weight(wg, 8, dtype)[0].bits, "gconv w_fwd")
    wg = EC.finite_table().view(64, 8, 3, 3)
    scale = det_tensor((64,), 22, 0.5, 1.5, bf16=False)
    wf, wd = ops.pack_gconv_weight(wg.cuda(), 8, scale.cuda(), True, dtype)
    rf, rd = R.pack_gconv_weight(wg, 8, dtype, scale)
    R.assert_bits(wf, rf.bits, "gconv w_fwd, finite")
    R.assert_bits(wd, rd.bits, "gconv w_dgrad")


# ---- layouts, directly ----------------------------------------------------------------------------------------------
# the parameter lists are module constants: tests/test_gpu_guarded.py runs the same cases under the guard
GCONV_CASES = [(64, 32), (128, 32), (64, 1), (128, 2)]
GCONV_KS = [3, 1]
STAGE_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 30, 44)]
SUBSAMPLE_SHAPES = [(1, 1, 1, 8), (2, 1, 6, 24), (1, 7, 1, 8), (2, 5, 6, 64), (1, 8, 9, 24), (1, 4, 4, 64)]
AFFINE_FWD_C = [8, 24, 64, 520]
AFFINE_ACTS = [0, 1, 2]
BETA_CASES = [(24, 1537), (2112, 37)]
SECOND_TRIP = ["elementwise", "subsample_fwd", "channel_affine", "maxpool", "stage_image", "converters",
               "pack_conv_weight"]


@both
@pytest.mark.parametrize("with_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("k", GCONV_KS)
@pytest.mark.parametrize("C,groups", GCONV_CASES)
def test_pack_gconv_layout(ops, C, groups, k, with_scale, dtype):
    w = det_tensor((C, C // groups, k, k), 40 + C + groups, -1, 1, bf16=False)
    scale = det_tensor((C,), 41, 0.5, 1.5, bf16=False) if with_scale else None
    wf, wd = ops.pack_gconv_weight(w.cuda(), groups, scale.cuda() if with_scale else None, True, dtype)
    rf, rd = R.pack_gconv_weight(w, groups, dtype, scale)
    assert int((rf.bits == 0).sum()) >= C * k * k * (64 - C // groups)
    R.assert_bits(wf, rf.bits, "w_fwd [C][kh][kw][64]")
    R.assert_bits(wd, rd.bits, "w_dgrad [C][kh][kw][64]")
    wcl = w.cuda().contiguous(memory_format=torch.channels_last)
    R.assert_bits(ops.pack_gconv_weight(wcl, groups, None, False, dtype)[0], rf.bits, "w_fwd, channels_last")


@both
def test_pack_stem_layout(ops, dtype):
    w = det_tensor((64, 3, 7, 7), 42, -0.3, 0.3, bf16=False)
    R.assert_bits(ops.pack_stem_weight(w.cuda(), dtype), R.pack_stem_weight(w, dtype).bits, "[co][kh][8][4]")


@both
@pytest.mark.parametrize("shape", STAGE_SHAPES)
def test_stage_image_every_element(ops, shape, dtype):
    N, H, W = shape
    img = det_tensor((N, 3, H, W), 43, -3, 3, bf16=False)
    want = R.stage_image(img, dtype).bits
    assert float(want[:, :3].abs().sum() + want[:, :, :3].abs().sum() + want[..., 3].abs().sum()) == 0
    R.assert_bits(ops.stage_image(img.cuda(), dtype), want, "staged")
    R.assert_bits(ops.stage_image(img.cuda().contiguous(memory_format=torch.channels_last), dtype), want, "staged, cl")


HW = {1: (1, 1), 31: (1, 31), 32: (4, 8), 33: (3, 11), 117: (9, 13)}
CONVERTER_CASES = [(1, 1), (1, 117), (3, 31), (31, 32), (32, 32), (32, 33), (33, 117), (70, 1), (70, 33), (70, 117)]


@both
@pytest.mark.parametrize("C,hw", CONVERTER_CASES)
def test_converters(ops, C, hw, dtype):
    H, W = HW[hw]
    N = 2
    x = det_tensor((N, C, H, W), 44 + C + hw, -2, 2, bf16=False)
    y = ops.to_nhwc_bf16(x.cuda(), dtype)
    R.assert_bits(y, R.nchw_to_nhwc(x, dtype).bits, "fp32 -> NHWC")
    R.assert_nchw(ops.nhwc_to_nchw_f32(y), R.nhwc_to_nchw_f32(y).bits, "NHWC -> fp32 NCHW")
    R.assert_nchw(ops.nhwc_to_nchw_f32(y), q16(x, dtype), "NHWC -> fp32 NCHW is the rounded source")
    # the 16-bit transpose: plain NCHW, a channel / row / column slice, a step-2 column slice
    big = det_tensor((N, C + 2, H + 3, 2 * W + 2), 45, -2, 2, bf16=False).to(dtype)
    bg = big.cuda()
    for nm, sl in (("plain", (slice(None),) * 4),
                   ("slice", (slice(None), slice(1, C + 1), slice(2, H + 2), slice(1, W + 1))),
                   ("step 2", (slice(None), slice(0, C), slice(0, H), slice(1, 2 * W + 1, 2)))):
        src = bg[sl]
        R.assert_bits(ops.to_nhwc_bf16(src, dtype), R.nchw_to_nhwc(big[sl], dtype).bits, "16-bit transpose, " + nm)


# ---- max pool -------------------------------------------------------------------------------------------------------
def _pool_refs(x, dy, dtype, f64=True):
    """(y, idx, dx plain, dx with mask_src, dx with pooled): the expected bits of one pool case."""
    H, W = x.shape[2:]
    yr, code = R.maxpool3x3s2_fwd(x)
    return (yr.bits, code) + tuple(R.maxpool3x3s2_bwd(dy, code, (H, W), dtype, f64=f64, **kw).bits
                                   for kw in ({}, {"mask_src": x}, {"pooled": yr.bits}))


def _pool_check(ops, x, dy, dtype, what, refs=None):
    H, W = x.shape[2:]
    y_ref, code, dx_ref, dxm_ref, dxp_ref = refs or _pool_refs(x, dy, dtype)
    xg = dev(x, dtype)
    y, idx = ops.maxpool3x3s2_fwd(xg)
    R.assert_nchw(host(y), y_ref, what + ": y")
    R.assert_nchw(host(idx), code, what + ": idx")
    dyg = dev(dy, dtype)
    R.assert_nchw(host(ops.maxpool3x3s2_bwd(dyg, idx, (H, W))), dx_ref, what + ": dx")
    dxm = ops.maxpool3x3s2_bwd(dyg, idx, (H, W), xg)
    R.assert_nchw(host(dxm), dxm_ref, what + ": dx, mask_src")
    dxp = ops.maxpool3x3s2_bwd(dyg, idx, (H, W), pooled=y)
    R.assert_nchw(host(dxp), dxp_ref, what + ": dx, pooled")
    R.assert_bits(dxp, dxm, what + ": pooled form against mask_src form")


@both
@pytest.mark.parametrize("kind", EC.POOL_KINDS)
@pytest.mark.parametrize("shape", EC.POOL_SHAPES)
def test_maxpool(ops, shape, kind, dtype):
    N, H, W, C = shape
    x = EC.pool_input(kind, shape)
    dy = q16(det_tensor((N, C, R.pool_out(H), R.pool_out(W)), 52, -1, 1, bf16=False), dtype)
    _pool_check(ops, x, dy, dtype, "%s %s" % (kind, shape))


# ---- subsample, add, clamp, mask ------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize("shape", SUBSAMPLE_SHAPES)
def test_subsample_add_clamp_mask(ops, shape, dtype):
    N, H, W, C = shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    x, base, b, m = (q16(det_tensor((N, C, H, W), 60 + j, -8, 8, bf16=False), dtype) for j in range(4))
    dy = q16(det_tensor((N, C, Ho, Wo), 64, -8, 8, bf16=False), dtype)
    big = float(torch.tensor(60000.0).to(dtype))            # fp16: 60000 + 60000 overflows to inf, as torch's does
    for t in (x, base, b, dy):
        t[0, 0, 0, 0] = big
        t[-1, -1, -1, -1] = -big if t.numel() > 1 else big
    xg = dev(x, dtype)
    R.assert_nchw(host(ops.subsample2_fwd(xg)), R.subsample2_fwd(x).bits, "subsample2_fwd")
    dyg = dev(dy, dtype)
    R.assert_nchw(host(ops.subsample2_bwd(dyg, (H, W))), R.subsample2_bwd(dy, (H, W), dtype).bits, "subsample2_bwd")
    got = host(ops.subsample2_bwd(dyg, (H, W), dev(base, dtype)))
    want = R.subsample2_bwd(dy, (H, W), dtype, base).bits
    R.assert_nchw(got, want, "subsample2_bwd + dx_in")
    if dtype == torch.float16:
        assert float(want[0, 0, 0, 0]) == float("inf") and float(got[0, 0, 0, 0]) == float("inf")
    for bb in (None, b):
        for mm in (None, m):
            got = ops.add_relu_mask(xg, None if bb is None else dev(bb, dtype), None if mm is None else dev(mm, dtype))
            R.assert_nchw(host(got), R.add_relu_mask(x, dtype, bb, mm).bits,
                          "add_relu_mask b=%s mask=%s" % (bb is not None, mm is not None))
    m[0, 0, 0, 0] = 1.0
    assert dtype != torch.float16 or float(R.add_relu_mask(x, dtype, b, m).bits[0, 0, 0, 0]) == float("inf")
    R.assert_nchw(host(ops.add_relu_mask(xg, dev(b, dtype), dev(m, dtype))), R.add_relu_mask(x, dtype, b, m).bits, "a + b")
    for hi in (6.0, float("inf")):
        R.assert_nchw(host(ops.act_mask(dev(base, dtype), xg, hi)), R.act_mask(base, x, hi).bits, "act_mask hi=%s" % hi)
    y = xg.clone()
    assert ops.clamp_max_(y, 6.0) is y
    R.assert_nchw(host(y), R.clamp_max_(x, 6.0).bits, "clamp_max_")


# ---- channel affine -------------------------------------------------------------------------------------------------
def _affine_fwd_check(ops, x, scale, shift, act, dtype, what):
    b, pre = R.channel_affine_fwd(x, scale, shift, act, dtype)
    y = ops.channel_affine_fwd(dev(x, dtype), scale.cuda(), shift.cuda(), act)
    got = host(y).float()
    und = 0
    if act == 2:
        got, und = R.knee_resolved(got, b, pre, dtype)
    B.assert_within(got, b, dtype, what)
    return y, b, pre, und


@both
@pytest.mark.parametrize("act", AFFINE_ACTS)
@pytest.mark.parametrize("C", AFFINE_FWD_C)
def test_channel_affine_fwd(ops, C, act, dtype):
    N, H, W = (2, 5, 7) if C == 520 else (3, 13, 21)
    x = q16(det_tensor((N, C, H, W), 70 + C, -8, 8, bf16=False), dtype)
    scale, shift, _, _ = EC.affine_vectors(C, 71)
    _, _, _, und = _affine_fwd_check(ops, x, scale, shift, act, dtype, "affine fwd C=%d act=%d" % (C, act))
    assert und <= 1e-3 * x.numel()


@both
@pytest.mark.parametrize("C", AFFINE_FWD_C)
def test_channel_affine_relu6_knee(ops, C, dtype):
    """Stored values decide the backward mask 0 < y < 6: an element whose exact pre-activation is below 6 - E is
    stored below 6, one at or above 6 + E as exactly 6, and act_mask(g, y, 6) is g * (0 < v < 6) bit for bit wherever
    v is further than E from 0 and from 6 (at most 0.1 % of the elements may be that close; the recipe has none)."""
    npix = 37 if C == 520 else 301
    x, scale, shift = EC.relu6_knee_inputs(C, npix)
    y, b, pre, und = _affine_fwd_check(ops, x, scale, shift, 2, dtype, "ReLU6 knee C=%d" % C)
    got = host(y).double()
    assert int(((pre > R.TOP6[dtype]) & (pre < 6)).sum()) >= 300 and int((pre >= 6).sum()) >= 300
    below, above = pre < 6 - b.E, pre >= 6 + b.E
    bad = below & ~(got < 6)
    assert not bool(bad.any()), "a value under 6 stored as %r (exact %r)" % (float(got[bad][0]), float(pre[bad][0]))
    bad = above & ~(got == 6)
    assert not bool(bad.any()), "a value from 6 up stored as %r (exact %r)" % (float(got[bad][0]), float(pre[bad][0]))
    g = q16(det_tensor(tuple(x.shape), 72, -1, 1, bf16=False), dtype)
    out = host(ops.act_mask(dev(g, dtype), y, 6.0)).float()
    decided = ((pre.abs() > b.E) & ((pre - 6).abs() > b.E))
    assert int((~decided).sum()) <= 1e-3 * x.numel()
    want = torch.where((pre > 0) & (pre < 6), g, torch.zeros(()))
    R.assert_nchw(torch.where(decided, out, want), want, "act_mask(g, relu6(affine(x)), 6)")


def _affine_bwd(ops, g, x, scale, mean, invstd, dtype):
    C = g.shape[1]
    dx, dg, db = ops.channel_affine_bwd(dev(g, dtype), dev(x, dtype), scale.cuda(), mean.cuda(), invstd.cuda())
    return host(dx), dg.cpu(), db.cpu()


@both
@pytest.mark.parametrize("C,npix", EC.AFFINE_BWD_CASES)
def test_channel_affine_bwd_exact(ops, C, npix, dtype):
    """Exactly summable inputs: every partial sum is exact in fp32 in any order, with or without fma, so dbeta is the
    float64 sum, dgamma = fl32(sum * invstd) and dx = fl16(fl32(g * scale)) — in bits, in every thread layout."""
    g, x, mean = EC.affine_exact_inputs(C, npix)
    scale, _, _, invstd = EC.affine_vectors(C, 73)
    dxr, dbr, dgr, s1 = R.channel_affine_bwd(g, x, scale, mean, invstd, dtype)
    dx, dg, db = _affine_bwd(ops, g, x, scale, mean, invstd, dtype)
    R.assert_bits(db, dbr.v.float(), "dbeta (%d, %d)" % (C, npix))
    assert torch.equal(s1.float().double(), s1)
    R.assert_bits(dg, s1.float() * invstd, "dgamma (%d, %d)" % (C, npix))
    R.assert_nchw(dx, dxr.bits, "dx (%d, %d)" % (C, npix))


@both
@pytest.mark.parametrize("C,npix", EC.AFFINE_BWD_CASES)
def test_channel_affine_bwd_random(ops, C, npix, dtype):
    g = q16(det_tensor((1, C, 1, npix), 74, -1, 1, bf16=False), dtype)
    x = q16(det_tensor((1, C, 1, npix), 75, -4, 4, bf16=False), dtype)
    scale, _, mean, invstd = EC.affine_vectors(C, 76)
    dxr, dbr, dgr, _ = R.channel_affine_bwd(g, x, scale, mean, invstd, dtype)
    dx, dg, db = _affine_bwd(ops, g, x, scale, mean, invstd, dtype)
    B.assert_within(db, dbr, torch.float32, "dbeta (%d, %d)" % (C, npix))
    B.assert_within(dg, dgr, torch.float32, "dgamma (%d, %d)" % (C, npix))
    R.assert_nchw(dx, dxr.bits, "dx (%d, %d)" % (C, npix))


@both
@pytest.mark.parametrize("C,npix", BETA_CASES)
def test_channel_affine_bwd_beta(ops, C, npix, dtype, seeded=None):
    """The accumulate path of the C ABI: beta = 1 onto known dgamma / dbeta gives old + new — exact on the summable
    recipe with old on the same lattice —, beta = 0.5 gives fl32(0.5 * old + new), possibly one fma (Bound, T = 2).
    ``seeded(t, label)``: how the seeded dgamma / dbeta get to the device (the guarded reuse puts them between bands)."""
    seeded = seeded or (lambda t, label: t.cuda())
    from torch_detection_amd import _lib
    lib = _lib.load()
    g, x, mean = EC.affine_exact_inputs(C, npix)
    scale, _, _, _ = EC.affine_vectors(C, 77)
    invstd = torch.tensor([0.5, 1.0, 2.0, 0.25])[torch.arange(C) % 4]          # powers of two: dgamma stays on a lattice
    _, dbr, dgr, _ = R.channel_affine_bwd(g, x, scale, mean, invstd, dtype)
    gd, xd = dev(g, dtype), dev(x, dtype)
    sc, mu, inv = scale.cuda(), mean.cuda(), invstd.cuda()
    dx = torch.empty_like(xd)
    nbytes = lib.tdn_channel_affine_bwd_workspace(npix, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    old_g = EC.grid((C,), 78, -64, 64, 2.0 ** -7)
    old_b = EC.grid((C,), 79, -64, 64, 2.0 ** -7)
    for beta in (1.0, 0.5):
        dg, db = seeded(old_g, "channel_affine_bwd: seeded dgamma"), seeded(old_b, "channel_affine_bwd: seeded dbeta")
        rc = lib.tdn_channel_affine_bwd(p(gd), p(xd), p(sc), p(mu), p(inv), p(dx), p(dg), p(db), beta, npix, C, p(ws),
                                        nbytes, ops.dtype_code(dtype), _lib.stream_ptr())
        _lib.check(rc, "tdn_channel_affine_bwd")
        for nm, got, old, new in (("dgamma", dg, old_g, dgr.v), ("dbeta", db, old_b, dbr.v)):
            v = beta * old.double() + new
            if beta == 1.0:
                assert torch.equal(v.float().double(), v)
                R.assert_bits(got, v.float(), "%s, beta = 1" % nm)
            else:
                bound = B.Bound(v, (beta * old.double()).abs() + new.abs(), 2, note="beta * old + new", activation=False)
                B.assert_within(got.cpu(), bound, torch.float32, "%s, beta = 0.5" % nm)


# ---- the second trip of every grid-stride / tile-stride loop --------------------------------------------------------
CAP = 4096 * 256            # lanes of the largest grid_for launch
TILE_CAP = 8192             # blocks of the largest transpose launch


class _Big(object):
    """The large inputs and references, computed once per requesting module and shared by its cases (do not modify
    them); dropped when that module's tests are done."""

    def __init__(self):
        self.kept = {}

    def grid(self, shape, seed, lo, hi, step):
        """Grid values: exact in both element types."""
        key = (shape, seed, lo, hi, step)
        if key not in self.kept:
            self.kept[key] = EC.grid(shape, seed, lo, hi, step)
        return self.kept[key]

    def pool(self):
        """Input, cotangent and expected bits of the large pool case, once for both element types: every value — the
        sums of up to four multiples of 1/8 included — is exact in bf16 AND fp16, which is asserted."""
        if "pool" not in self.kept:
            N, H, W, C = 1, 363, 365, 256
            x = EC.grid((N, C, H, W), 88, -2, 2, 0.5)
            dy = EC.grid((N, C, 182, 183), 89, -1, 1, 0.125)
            refs = _pool_refs(x, dy, torch.bfloat16, f64=False)
            for t in (x, dy, refs[0]) + refs[2:]:
                assert torch.equal(t.half().float(), t) and torch.equal(t.bfloat16().float(), t)
            self.kept["pool"] = (x, dy, refs)
        return self.kept["pool"]


@pytest.fixture(scope="module")
def big():
    b = _Big()
    yield b
    b.kept.clear()


@both
def test_second_trip_elementwise(ops, big, dtype):
    N, H, W, C = 1, 129, 128, 512
    assert N * H * W * C // 8 > CAP
    shp = (N, C, H, W)
    a, b, m = big.grid(shp, 80, -8, 8, 0.5), big.grid(shp, 81, -8, 8, 0.5), big.grid(shp, 82, -2, 2, 1.0)
    ag, bg, mg = dev(a, dtype), dev(b, dtype), dev(m, dtype)
    R.assert_nchw(host(ops.add_relu_mask(ag, bg, mg)), R.add_relu_mask(a, dtype, b, m).bits, "add_relu_mask")
    for hi in (6.0, float("inf")):
        R.assert_nchw(host(ops.act_mask(bg, ag, hi)), R.act_mask(b, a, hi).bits, "act_mask hi=%s" % hi)
    dy = big.grid((N, C, 65, 64), 83, -8, 8, 0.5)
    dyg = dev(dy, dtype)
    R.assert_nchw(host(ops.subsample2_bwd(dyg, (H, W))), R.subsample2_bwd(dy, (H, W), dtype).bits, "subsample2_bwd")
    R.assert_nchw(host(ops.subsample2_bwd(dyg, (H, W), ag)), R.subsample2_bwd(dy, (H, W), dtype, a).bits,
                  "subsample2_bwd + dx_in")
    R.assert_nchw(host(ops.clamp_max_(ag, 6.0)), R.clamp_max_(a, 6.0).bits, "clamp_max_")     # in place: last


@both
def test_second_trip_subsample_fwd(ops, big, dtype):
    shp = (1, 512, 257, 258)
    assert 129 * 129 * 64 > CAP
    x = big.grid(shp, 84, -8, 8, 0.5)
    R.assert_nchw(host(ops.subsample2_fwd(dev(x, dtype))), R.subsample2_fwd(x).bits, "subsample2_fwd")


@both
def test_second_trip_channel_affine(ops, big, dtype):
    C, H, W = 520, 127, 128
    assert H * W * C // 8 > CAP
    x = big.grid((1, C, H, W), 85, -8, 8, 0.25)
    g = big.grid((1, C, H, W), 86, -1, 1, 0.125)
    scale, shift, mean, invstd = EC.affine_vectors(C, 87)
    for act in (0, 1, 2):
        _, _, _, und = _affine_fwd_check(ops, x, scale, shift, act, dtype, "affine fwd, act %d" % act)
        assert und <= 1e-3 * x.numel()
    dxr, dbr, dgr, _ = R.channel_affine_bwd(g, x, scale, mean, invstd, dtype)
    dx, dg, db = _affine_bwd(ops, g, x, scale, mean, invstd, dtype)
    B.assert_within(db, dbr, torch.float32, "dbeta")
    B.assert_within(dg, dgr, torch.float32, "dgamma")
    R.assert_nchw(dx, dxr.bits, "dx")


@both
def test_second_trip_maxpool(ops, big, dtype):
    assert 182 * 183 * (256 // 8) > CAP
    x, dy, refs = big.pool()
    _pool_check(ops, x, dy, dtype, "second trip", refs)


@both
def test_second_trip_stage_image(ops, big, dtype):
    H, W = 1020, 1022
    assert (H + 6) * (W + 8) > CAP
    img = det_tensor((1, 3, H, W), 90, -3, 3, bf16=False)
    R.assert_bits(ops.stage_image(img.cuda(), dtype), R.stage_image(img, dtype).bits, "staged")


@both
def test_second_trip_converters(ops, big, dtype):
    N, C, H, W = 1, 70, 257, 341
    assert -(-H * W // 32) * -(-C // 32) > TILE_CAP
    x = det_tensor((N, C, H, W), 91, -2, 2, bf16=False)
    want = R.nchw_to_nhwc(x, dtype).bits
    y = ops.to_nhwc_bf16(x.cuda(), dtype)
    R.assert_bits(y, want, "fp32 -> NHWC")
    R.assert_nchw(ops.nhwc_to_nchw_f32(y), q16(x, dtype), "NHWC -> fp32 NCHW")
    x16 = x.to(dtype)
    R.assert_bits(ops.to_nhwc_bf16(x16.cuda(), dtype), want, "16-bit transpose")


@both
def test_second_trip_pack_conv_weight(ops, big, dtype):
    w = det_tensor((512, 512, 3, 3), 92, -1, 1, bf16=False)
    assert w.numel() > CAP
    scale = det_tensor((512,), 93, 0.5, 1.5, bf16=False)
    wf, wd = ops.pack_conv_weight(w.cuda(), scale.cuda(), True, dtype)
    rf, rd = R.pack_conv_weight(w, dtype, scale)
    R.assert_bits(wf, rf.bits, "w_fwd")
    R.assert_bits(wd, rd.bits, "w_dgrad")
