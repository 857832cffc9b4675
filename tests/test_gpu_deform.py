"""GPU: deformable convolution (csrc/deform.hip) against the CPU oracle of tests/deform_ref.py.

The sampled ``cols`` bit for bit; the offset / mask / input gradients element by element against the float64 oracle under
the bound derived in deform_ref.py, ``dx`` under guard-banded, poisoned allocations with an exact-size workspace; bitwise
reproducibility, eager and graph-replayed; the adversarial all-samples-on-one-pixel input; the forward GEMM under
bound_util's bound; the whole ``ModulatedDeformConvPack`` chain against float64 autograd with a tolerance measured on the
oracle's own 16-bit-staged chain; module behaviour."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bound_util as BU
import deform_cases as DC
import deform_ref as R
import guard_util as G

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CL = torch.channels_last
# (compute dtype, offsets / mask in float32?)
COMBOS = [(BF16, True), (BF16, False), (F16, True), (F16, False)]
GEO_IDS = ["%dx%d-s%d-d%d" % (hw[0], hw[1], s, p) for hw, s, p in DC.GEOMETRIES]
CH_IDS = ["C%d-dg%d" % c for c in DC.CHANNELS]


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd as T
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need cuda:0")
    return T


@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import deform_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, deform_ops, g)
    return g


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def share_ok(c, offset=None):
    P = R.Positions(c.offset if offset is None else offset, c.H, c.W, c.stride, c.pad, c.dg)
    assert DC.SHARE[0] < P.in_range_share() < DC.SHARE[1], P.in_range_share()
    return P


def dev(a, dtype):
    return DC.nhwc(a, dtype, "cuda")


def kw(c):
    return dict(stride=c.stride, padding=c.pad, dilation=c.pad, deformable_groups=c.dg)


def cols_np(t):
    """device cols (N, Ho, Wo, 9 C) -> float32 array (N, Ho, Wo, 9, C)"""
    N, Ho, Wo, K = t.shape
    return t.float().cpu().numpy().reshape(N, Ho, Wo, 9, K // 9)


def nchw_np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def within(got, v, S, T, dtype, what):
    allow = R.allowance(v, S, T, dtype)
    err = np.abs(got - v)
    err = np.where(np.isfinite(err), err, np.inf)
    worst = np.unravel_index(np.argmax(err - allow), err.shape)
    print("%s: worst err %.4g, allowance %.4g at %s (v = %.6g)" % (what, err[worst], allow[worst], worst, v[worst]))
    assert (err <= allow).all(), "%s: element %s off by %.6g, allowance %.6g (got %.9g, exact %.9g)" % (
        what, worst, err[worst], allow[worst], got[worst], v[worst])


# ---- 1. deform_sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chan", DC.CHANNELS, ids=CH_IDS)
@pytest.mark.parametrize("geo", DC.GEOMETRIES, ids=GEO_IDS)
def test_sample_is_bit_identical_to_the_oracle(T, geo, chan):
    from torch_detection_amd import deform_ops as D
    for dtype, f32off in COMBOS:
        c = DC.make(1, geo[0], geo[1], geo[2], chan[0], chan[1], dtype)
        P = share_ok(c)
        odt = F32 if f32off else dtype
        x, off, msk, lgt = dev(c.x, dtype), dev(c.offset, odt), dev(c.mask, odt), dev(c.logit, odt)
        for mask_np, mask_t in ((None, None), (c.mask, msk)):
            got = D.deform_sample(x, off, mask_t, **kw(c))
            assert got.dtype == dtype and tuple(got.shape) == (c.N, c.Ho, c.Wo, 9 * c.C) and got.is_contiguous()
            ref = R.sample(c.x, c.offset, mask_np, c.stride, c.pad, c.dg, dtype, positions=P)
            assert np.array_equal(R.bits16(cols_np(got), dtype), R.bits16(ref, dtype)), (dtype, f32off, mask_np is None)
        # offsets and mask read in place from ONE wider buffer through the pitch
        wide = torch.full((c.N, c.Ho, c.Wo, 64 * ((27 * c.dg + 63) // 64)), float("nan"), dtype=odt, device="cuda")
        wide = wide.permute(0, 3, 1, 2)
        wide[:, :18 * c.dg] = off
        wide[:, 18 * c.dg:27 * c.dg] = msk
        assert same_bits(D.deform_sample(x, wide[:, :18 * c.dg], wide[:, 18 * c.dg:27 * c.dg], **kw(c)), got)
        # the logit: the device's exp is not NumPy's — within one 16-bit ulp, at least 99 % identical
        got = D.deform_sample(x, off, lgt, mask_is_logit=True, **kw(c))
        ref = R.sample(c.x, c.offset, c.logit, c.stride, c.pad, c.dg, dtype, mask_is_logit=True, positions=P)
        gb, rb = R.bits16(cols_np(got), dtype).astype(np.int32), R.bits16(ref, dtype).astype(np.int32)
        assert np.abs(gb - rb).max() <= 1 and (gb == rb).mean() >= 0.99, (np.abs(gb - rb).max(), (gb == rb).mean())


def test_sample_at_hand_placed_positions(T):
    """Records put exactly on integers, on -1 and H (invalid), a hair inside -1, and on NaN, +-inf and 1e30."""
    from torch_detection_amd import deform_ops as D
    for dtype in (BF16, F16):
        c = DC.make(2, (9, 11), 1, 1, 64, 2, dtype)
        off = c.offset.copy().reshape(c.N, c.dg, 9, 2, c.Ho, c.Wo)
        k = np.arange(9)
        by = (np.arange(c.Ho)[None, :, None] - 1 + (k // 3)[:, None, None]).astype(np.float32)
        bx = (np.arange(c.Wo)[None, None, :] - 1 + (k % 3)[:, None, None]).astype(np.float32)
        places = [(3.0, 4.0), (0.0, 0.0), (8.0, 10.0), (-1.0, 4.0), (3.0, -1.0), (9.0, 4.0), (3.0, 11.0),
                  (-1.0 + 2.0 ** -20, 4.0), (3.0, -1.0 + 2.0 ** -20), (9.0 - 2.0 ** -20, 11.0 - 2.0 ** -20),
                  (np.nan, 4.0), (3.0, np.nan), (np.inf, 4.0), (3.0, -np.inf), (1e30, 4.0), (3.0, -1e30)]
        want_valid = [True] * 3 + [False] * 4 + [True] * 3 + [False] * 6
        spots = []
        for i, (py, px) in enumerate(places):
            n, g, kk, ho, wo = i % c.N, i % c.dg, (2 * i) % 9, (3 * i) % c.Ho, (5 * i) % c.Wo
            off[n, g, kk, 0, ho, wo] = np.float32(py) - by[kk, ho, 0]
            off[n, g, kk, 1, ho, wo] = np.float32(px) - bx[kk, 0, wo]
            spots.append((n, g, kk, ho, wo))
        off = off.reshape(c.N, 18 * c.dg, c.Ho, c.Wo)
        with np.errstate(invalid="ignore"):
            P = R.Positions(off, c.H, c.W, 1, 1, c.dg)
        assert [bool(P.valid[s]) for s in spots] == want_valid
        assert float(P.ly[spots[7]]) == 2.0 ** -20 and int(P.y0[spots[7]]) == -1
        got = D.deform_sample(dev(c.x, dtype), dev(off, F32), dev(c.mask, F32), **kw(c))
        ref = R.sample(c.x, off, c.mask, 1, 1, c.dg, dtype, positions=P)
        assert np.array_equal(R.bits16(cols_np(got), dtype), R.bits16(ref, dtype))
        gn = cols_np(got)
        Cg = c.C // c.dg
        for (n, g, kk, ho, wo), ok in zip(spots, want_valid):
            if not ok:
                assert not gn[n, ho, wo, kk, g * Cg:(g + 1) * Cg].any()
        n, g, kk, ho, wo = spots[0]                           # exactly on pixel (3, 4): the pixel's value times the mask
        want = R.round16(c.x[n, g * Cg:(g + 1) * Cg, 3, 4] * c.mask[n, g * 9 + kk, ho, wo], dtype)
        assert np.array_equal(gn[n, ho, wo, kk, g * Cg:(g + 1) * Cg], want)


# ---- 2. the gradients of the gather ----------------------------------------------------------------------------------
@pytest.mark.parametrize("chan", DC.CHANNELS, ids=CH_IDS)
@pytest.mark.parametrize("geo", DC.GEOMETRIES, ids=GEO_IDS)
def test_coord_and_input_gradients_within_the_bound_under_the_guard(T, guard, geo, chan):
    from torch_detection_amd import deform_ops as D
    for dtype, f32off in COMBOS:
        c = DC.make(2, geo[0], geo[1], geo[2], chan[0], chan[1], dtype)
        P = share_ok(c)
        odt = F32 if f32off else dtype
        gc = lambda a, dt, name: guard.guard_copy(dev(a, dt).permute(0, 2, 3, 1), name).permute(0, 3, 1, 2)
        x, off = gc(c.x, dtype, "x"), gc(c.offset, odt, "offset")
        dcol = guard.guard_copy(DC.t16(c.dcol, dtype, "cuda").reshape(c.N, c.Ho, c.Wo, 9 * c.C), "dcol")
        for name, m_np, logit in (("none", None, False), ("mask", c.mask, False), ("logit", c.logit, True)):
            m = gc(m_np, odt, "mask") if m_np is not None else None
            ref = R.Grads(c.x, c.offset, c.dcol, m_np, c.stride, c.pad, c.dg, mask_is_logit=logit)
            what = "%s %s offsets %s" % (dtype, odt, name)
            doff, dmsk = D.deform_coord_grad(dcol, x, off, m, mask_is_logit=logit, **kw(c))
            assert doff.dtype == odt and tuple(doff.shape) == (c.N, 18 * c.dg, c.Ho, c.Wo)
            assert doff.permute(0, 2, 3, 1).is_contiguous()
            within(nchw_np(doff), ref.doffset, ref.S_doffset, ref.T_doffset, odt, what + ": doffset")
            inval = np.repeat(~P.valid.reshape(c.N, 9 * c.dg, c.Ho, c.Wo), 2, axis=1)
            assert not nchw_np(doff)[inval].any()
            if m is None:
                assert dmsk is None
            else:
                within(nchw_np(dmsk), ref.dmask, ref.S_dmask, ref.T_dmask, odt, what + ": dmask")
                assert not nchw_np(dmsk)[~P.valid.reshape(c.N, 9 * c.dg, c.Ho, c.Wo)].any()
            dx = D.deform_input_grad(dcol, off, m, (c.N, c.C, c.H, c.W), mask_is_logit=logit, **kw(c))
            assert dx.dtype == dtype and tuple(dx.shape) == (c.N, c.C, c.H, c.W) and dx.permute(0, 2, 3, 1).is_contiguous()
            within(nchw_np(dx), ref.dx, ref.S_dx, ref.T_dx, dtype, what + ": dx")
            untouched = np.broadcast_to((ref.terms_dx == 0)[:, :, None], (c.N, c.dg, c.C // c.dg, c.H, c.W))
            assert not nchw_np(dx)[untouched.reshape(c.N, c.C, c.H, c.W)].any()
        found = guard.check()                     # every output fully written, nothing outside, exact workspaces
        assert not found, found
    ws = [n for op, n, given in guard.ws_log if op == "deform_input_grad"]
    assert ws and all(n == D.deform_workspace_bytes(c.N, c.H, c.W, c.stride, c.pad, c.dg) for n in ws)


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_backward_is_bitwise_reproducible_eager_and_replayed(T, dtype):
    c = DC.make(3, (13, 19), 1, 1, 64, 2, dtype)
    share_ok(c)
    x, off, msk = (dev(a, dt).requires_grad_() for a, dt in ((c.x, dtype), (c.offset, F32), (c.mask, dtype)))
    w = torch.from_numpy(c.weight).cuda().requires_grad_()
    b = torch.from_numpy(c.bias).cuda().requires_grad_()
    gy = dev(c.gy, dtype)
    ins = (x, off, msk, w, b)

    def grads():
        y = T.deform_conv2d(x, off, w, b, mask=msk, relu=True, **kw(c))
        return torch.autograd.grad(y, ins, gy)

    first = [g.clone() for g in grads()]
    second = grads()
    assert all(torch.isfinite(g.float()).all() for g in first)
    for a, bb in zip(first, second):
        assert same_bits(a, bb)
    out = [torch.zeros_like(g) for g in first]

    def step():
        for o, g in zip(out, grads()):
            o.copy_(g)

    gs = T.GraphedStep(step, warmup=2, verbose=True)
    assert gs.captured, gs.error
    for o in out:
        o.zero_()
    gs()
    torch.cuda.synchronize()
    for a, o in zip(first, out):
        assert same_bits(a, o)


# ---- 4. every sample of an image on one pixel -------------------------------------------------------------------------
@pytest.mark.parametrize("chan", DC.CHANNELS, ids=CH_IDS)
def test_all_samples_on_one_pixel(T, guard, chan):
    from torch_detection_amd import deform_ops as D
    for dtype, f32off in COMBOS:
        c = DC.make(4, (9, 11), 1, 1, chan[0], chan[1], dtype)
        odt = F32 if f32off else dtype
        offset = DC.one_pixel_offsets(c, 3, 4, (0.0, 0.0))
        P = R.Positions(offset, c.H, c.W, 1, 1, c.dg)
        assert P.valid.all() and (P.y0 == 3).all() and (P.x0 == 4).all() and not P.ly.any() and not P.lx.any()
        assert P.valid[0].sum() == 891 * c.dg
        dcol = DC.t16(c.dcol, dtype, "cuda").reshape(c.N, c.Ho, c.Wo, 9 * c.C)
        dx = D.deform_input_grad(dcol, dev(offset, odt), dev(c.mask, odt), (c.N, c.C, c.H, c.W), **kw(c))
        ref = R.Grads(c.x, offset, c.dcol, c.mask, 1, 1, c.dg)
        assert (ref.terms_dx[:, :, 3, 4] == 891).all() and ref.terms_dx.sum() == 891.0 * 4 * c.N * c.dg
        within(nchw_np(dx), ref.dx, ref.S_dx, ref.T_dx, dtype, "%s %s: dx, one pixel" % (dtype, odt))
        got = nchw_np(dx)
        assert got[:, :, 3, 4].all()
        got[:, :, 3, 4] = 0
        assert not got.any()
        assert not guard.check()


# ---- 5. the forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", DC.GEOMETRIES, ids=GEO_IDS)
def test_forward_within_the_gemm_bound_of_the_oracle_cols(T, geo):
    for (C, dg), (dtype, f32off) in zip(DC.CHANNELS, COMBOS):
        c = DC.make(5, geo[0], geo[1], geo[2], C, dg, dtype)
        P = share_ok(c)
        odt = F32 if f32off else dtype
        x, off, msk = dev(c.x, dtype), dev(c.offset, odt), dev(c.mask, odt)
        w, b = torch.from_numpy(c.weight).cuda(), torch.from_numpy(c.bias).cuda()
        for m_np, m in ((None, None), (c.mask, msk)):
            cols = R.sample(c.x, c.offset, m_np, c.stride, c.pad, c.dg, dtype, positions=P)
            cols = torch.from_numpy(cols).reshape(c.N, c.Ho, c.Wo, 9 * C).permute(0, 3, 1, 2)
            w1 = torch.from_numpy(c.weight).reshape(c.Cout, C, 9).permute(0, 2, 1).reshape(c.Cout, 9 * C, 1, 1)
            for relu in (False, True):
                y = T.deform_conv2d(x, off, w, b, mask=m, relu=relu, **kw(c))
                assert y.dtype == dtype and tuple(y.shape) == (c.N, c.Cout, c.Ho, c.Wo)
                assert y.permute(0, 2, 3, 1).is_contiguous()
                bound = BU.fwd_bound(cols, w1, shift=torch.from_numpy(c.bias), relu=relu)
                r = BU.assert_within(y.float().cpu(), bound, dtype, "deform_conv2d %s relu=%s" % (dtype, relu))
                print("forward", geo, C, dg, dtype, "ratio %.3f" % r["ratio"])


@pytest.mark.parametrize("geo", DC.GEOMETRIES, ids=GEO_IDS)
def test_fresh_pack_modules_are_the_plain_convolution(T, geo):
    """Zero-initialised offset convs: zero offsets (and mask logits 0: every mask value exactly 0.5)."""
    from torch_detection_amd import ops
    (H, W), stride, pad = geo
    for dtype, C, dg, cls in ((BF16, 64, 2, T.DeformConvPack), (F16, 128, 1, T.DeformConvPack),
                              (BF16, 64, 4, T.ModulatedDeformConvPack)):
        c = DC.make(6, geo[0], stride, pad, C, dg, dtype)
        m = cls(C, c.Cout, 3, stride=stride, padding=pad, dilation=pad, deformable_groups=dg, bias=True).cuda()
        with torch.no_grad():
            m.weight.copy_(torch.from_numpy(c.weight))
            m.bias.copy_(torch.from_numpy(c.bias))
        x = dev(c.x, dtype)
        y = m(x)
        scale = 0.5 if m.modulated else 1.0
        bound = BU.fwd_bound(torch.from_numpy(c.x), torch.from_numpy(c.weight * scale), stride, pad,
                             shift=torch.from_numpy(c.bias), dilation=pad)
        BU.assert_within(y.detach().float().cpu(), bound, dtype, "fresh %s %s" % (cls.__name__, dtype))
        if not m.modulated:
            w_fwd, _ = ops.pack_conv_weight(m.weight, None, False, dtype)
            ref = ops.conv2d_fwd(x.permute(0, 2, 3, 1), w_fwd, 3, stride, pad, None, m.bias.detach())
            BU.assert_within(ref.permute(0, 3, 1, 2).float().cpu(), bound, dtype, "conv2d_fwd %s" % dtype)


# ---- 6. the whole chain against float64 autograd ----------------------------------------------------------------------
def staged_chain(c, w_off, b_off, dtype):
    """The oracle's own chain with a rounding to ``dtype`` wherever the kernels store 16 bits: the offset conv's output,
    cols, y, dcol, the offset / mask-logit gradient, the two input gradients and their sum."""
    r = lambda a: R.round16(a, dtype).astype(np.float64)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    s, p, dg = c.stride, c.pad, c.dg
    w_off16, w16 = r(w_off), r(c.weight)
    om = r(F.conv2d(t(c.x), t(w_off16), t(b_off), s, p, p).numpy())
    offset, logit = om[:, :18 * dg], om[:, 18 * dg:]
    cols = R.sample(c.x, offset, logit, s, p, dg, dtype, mask_is_logit=True).astype(np.float64)
    y = r(R.cols_gemm(cols, w16, c.bias))
    wk = w16.reshape(c.Cout, c.C, 9).transpose(0, 2, 1)
    dcol = r(np.einsum("nohw,okc->nhwkc", c.gy.astype(np.float64), wk))
    dw = np.einsum("nhwkc,nohw->okc", cols, c.gy.astype(np.float64)).transpose(0, 2, 1).reshape(c.Cout, c.C, 3, 3)
    db = c.gy.astype(np.float64).sum((0, 2, 3))
    g = R.Grads(c.x, offset, dcol, logit, s, p, dg, mask_is_logit=True)
    dom = r(np.concatenate([g.doffset, g.dmask], 1))
    dx_off = r(torch.nn.grad.conv2d_input(c.x.shape, t(w_off16), t(dom), s, p, p).numpy())
    dw_off = torch.nn.grad.conv2d_weight(t(c.x), w_off.shape, t(dom), s, p, p).numpy()
    dx = r(r(g.dx) + dx_off)
    return {"y": y, "dx": dx, "weight": dw, "bias": db, "conv_offset_mask.weight": dw_off,
            "conv_offset_mask.bias": dom.sum((0, 2, 3))}


def exact_chain(c, w_off, b_off):
    d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_()
    x, w, b, wo, bo = d(c.x), d(c.weight), d(c.bias), d(w_off), d(b_off)
    om = F.conv2d(x, wo, bo, c.stride, c.pad, c.pad)
    y = R.deform_conv_autograd(x, om[:, :18 * c.dg], w, b, torch.sigmoid(om[:, 18 * c.dg:]), c.stride, c.pad, c.dg)
    y.backward(torch.from_numpy(c.gy.astype(np.float64)))
    return {"y": y.detach().numpy(), "dx": x.grad.numpy(), "weight": w.grad.numpy(), "bias": b.grad.numpy(),
            "conv_offset_mask.weight": wo.grad.numpy(), "conv_offset_mask.bias": bo.grad.numpy()}


CHAIN_CASES = [((13, 19), 1, 1, 64, 2, BF16), ((13, 19), 1, 1, 128, 1, F16), ((26, 37), 2, 2, 64, 4, BF16),
               ((13, 19), 2, 1, 64, 1, F16)]


@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda s: "%dx%d-s%d-d%d-C%d-dg%d-%s" % (
    s[0][0], s[0][1], s[1], s[2], s[3], s[4], str(s[5]).split(".")[-1]))
def test_modulated_pack_chain_against_float64_autograd(T, case):
    """Every tensor's error against float64 autograd, relative to the tensor's maximum, is at most twice that of the
    oracle's own 16-bit-staged chain (measured figures: profiles/deform_checks.md).  Most of that error is not rounding
    noise: a 16-bit offset moves a sample by up to 2^-9 of its size, across a pixel boundary now and then, and the
    offset gradient jumps there.  The main bias gradient is the one tensor the staged chain reproduces exactly; it is
    held to its a-priori fp32 summation bound instead."""
    hw, stride, pad, C, dg, dtype = case
    c = DC.make(7, hw, stride, pad, C, dg, dtype)
    rng = np.random.default_rng(77)
    w_off = (rng.standard_normal((27 * dg, C, 3, 3)) * (1.5 / np.sqrt(9.0 * C))).astype(np.float32)
    b_off = (rng.standard_normal(27 * dg) * 0.5).astype(np.float32)
    exact = exact_chain(c, w_off, b_off)
    staged = staged_chain(c, w_off, b_off, dtype)
    m = T.ModulatedDeformConvPack(C, c.Cout, 3, stride=stride, padding=pad, dilation=pad, deformable_groups=dg,
                                  bias=True).cuda()
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(c.weight))
        m.bias.copy_(torch.from_numpy(c.bias))
        m.conv_offset_mask.weight.copy_(torch.from_numpy(w_off))
        m.conv_offset_mask.bias.copy_(torch.from_numpy(b_off))
    x = dev(c.x, dtype).requires_grad_()
    y = m(x)
    y.backward(dev(c.gy, dtype))
    got = {"y": nchw_np(y), "dx": nchw_np(x.grad)}
    for name, p in m.named_parameters():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), name
        got[name] = nchw_np(p.grad)
    rel = lambda a, e: float(np.abs(a - e).max() / np.abs(e).max())
    rows = []
    for name in ("y", "dx", "weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"):
        rows.append((name, rel(staged[name], exact[name]), rel(got[name], exact[name])))
        print("chain %s %-24s oracle staged %.3e   gpu %.3e" % (case, *rows[-1]))
    for name, e_oracle, e_gpu in rows:
        if name == "bias":
            continue
        assert e_gpu <= 2.0 * e_oracle, (name, e_gpu, e_oracle)
    # db = sum of gy has no 16-bit-staged operand: the staged chain gives the exact sum (error 0.0) and twice that
    # allows nothing to an fp32 sum.  It gets the a-priori bound of its K = N Ho Wo terms instead (bound_util's form).
    assert rows[3][0] == "bias" and rows[3][1] == 0.0
    gy = c.gy.astype(np.float64)
    allow = R.allowance(exact["bias"], np.abs(gy).sum((0, 2, 3)), c.N * c.Ho * c.Wo, F32)
    assert (np.abs(got["bias"] - exact["bias"]) <= allow).all()


# ---- 7. module behaviour ----------------------------------------------------------------------------------------------
def test_module_state_dict_updates_and_graph_replay(T):
    dtype = BF16
    c = DC.make(8, (13, 19), 1, 1, 64, 2, dtype)
    rng = np.random.default_rng(5)
    mk = lambda: T.ModulatedDeformConvPack(64, c.Cout, 3, padding=1, deformable_groups=2, bias=True).cuda()
    a = mk()
    with torch.no_grad():
        a.conv_offset_mask.weight.copy_(torch.from_numpy(rng.standard_normal((54, 64, 3, 3)).astype(np.float32) * 0.05))
        a.conv_offset_mask.bias.copy_(torch.from_numpy(rng.standard_normal(54).astype(np.float32) * 0.5))
    x = dev(c.x, dtype)
    ya = a(x).detach().clone()
    b = mk()
    assert not same_bits(b(x).detach(), ya)
    b.load_state_dict(a.state_dict())
    assert same_bits(b(x).detach(), ya)
    # an in-place update is seen by the next call
    with torch.no_grad():
        b.weight.mul_(2.0)
        b.bias.mul_(2.0)
    assert same_bits(b(x).detach(), (ya.float() * 2.0).to(dtype))          # a power of two: exact
    with torch.no_grad():
        b.conv_offset_mask.bias.add_(0.25)
    assert not same_bits(b(x).detach(), (ya.float() * 2.0).to(dtype))
    # ... and inside a graph replay
    out = torch.zeros_like(ya)
    xg = dev(c.x, dtype).requires_grad_()
    gy = dev(c.gy, dtype)

    def step():
        a.zero_grad(set_to_none=False)
        y = a(xg)
        y.backward(gy)
        out.copy_(y.detach())

    step()
    for name, p in a.named_parameters():
        assert p.grad is not None and p.grad.abs().max() > 0, name          # the gradients reach conv_offset_mask.*
    grads0 = {n: p.grad.clone() for n, p in a.named_parameters()}
    xg.grad = None
    gs = T.GraphedStep(step, warmup=1, params=None)
    assert gs.captured, gs.error
    gs()
    torch.cuda.synchronize()
    assert same_bits(out, ya)
    for n, p in a.named_parameters():
        assert same_bits(p.grad, grads0[n]), n
    with torch.no_grad():
        a.weight.mul_(2.0)
        a.bias.mul_(2.0)
    gs()
    torch.cuda.synchronize()
    assert same_bits(out, (ya.float() * 2.0).to(dtype))
    # DCN v1 pack: the offsets' gradient reaches conv_offset
    p1 = T.DeformConvPack(64, c.Cout, 3, stride=2, padding=2, dilation=2, deformable_groups=1).cuda()
    with torch.no_grad():
        p1.conv_offset.weight.copy_(torch.from_numpy(rng.standard_normal((18, 64, 3, 3)).astype(np.float32) * 0.05))
    y1 = p1(x)
    y1.backward(torch.ones_like(y1))
    assert tuple(y1.shape) == (c.N, c.Cout, 7, 10)
    for name, p in p1.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
