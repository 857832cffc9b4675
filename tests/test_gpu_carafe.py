"""GPU: CARAFE upsampling (csrc/carafe.hip) against the CPU oracle of tests/carafe_ref.py.

The plain-mask forward bit for bit; the logits forward and the three gradients element by element against the float64
oracle under the bound derived in carafe_ref.py; every launch under guard-banded, poisoned allocations; bitwise
reproducibility, eager and graph-replayed; hand-placed inputs; the ``carafe`` autograd function; ``CARAFEPack`` and a
three-level ``FPN_CARAFE`` against float64 autograd of the torch composition with a tolerance measured on the oracle's own
16-bit-staged chain; graph capture with a weight update."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import carafe_cases as CC
import carafe_ref as R
import guard_util as G

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd as T
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need cuda:0")
    return T


@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import carafe_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, carafe_ops, g)
    return g


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def dev(a, dtype):
    return CC.nhwc(a, dtype, "cuda")


def nchw_np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def kgs(c):
    return c.k, c.g, c.s


def within(got, v, S, T, dtype, what):
    allow = R.allowance(v, S, T, dtype)
    err = np.abs(got - v)
    err = np.where(np.isfinite(err), err, np.inf)
    worst = np.unravel_index(np.argmax(err - allow), err.shape)
    print("%s: worst err %.4g, allowance %.4g at %s (v = %.6g)" % (what, err[worst], allow[worst], worst, v[worst]))
    assert (err <= allow).all(), "%s: element %s off by %.6g, allowance %.6g (got %.9g, exact %.9g)" % (
        what, worst, err[worst], allow[worst], got[worst], v[worst])


def operands(c, guard=None):
    """device copies of a case's arrays (inside NaN bands under a guard): x, masks, logits, gout, addend"""
    wdt = F32 if c.w32 else c.dtype

    def put(a, dt, name):
        if a is None:
            return None
        t = dev(a, dt)
        return t if guard is None else guard.guard_copy(t.permute(0, 2, 3, 1), name).permute(0, 3, 1, 2)

    return (put(c.x, c.dtype, "x"), put(c.masks, wdt, "masks"), put(c.logits, wdt, "logits"), put(c.gout, c.dtype, "gout"),
            put(c.addend, c.dtype, "addend"), wdt)


# ---- (a) the plain-mask forward, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.CASES, ids=repr)
def test_plain_mask_forward_is_bit_identical_to_the_oracle(T, guard, c):
    from torch_detection_amd import carafe_ops as D
    CC.make(c)
    x, masks, _, _, addend, _ = operands(c, guard)
    got = D.carafe_forward(x, *kgs(c), masks=masks, out_size=c.out_size, addend=addend)
    assert got.dtype == c.dtype and tuple(got.shape) == (c.N, c.C) + tuple(c.out_size)
    assert got.permute(0, 2, 3, 1).is_contiguous()
    ref = R.forward(c.x, c.masks, c.k, c.g, c.s, c.dtype, c.out_size, c.addend)
    assert np.array_equal(R.bits16(got.float().cpu().numpy(), c.dtype), R.bits16(ref, c.dtype))
    found = guard.check()
    assert not found, found


def test_forward_on_a_map_of_more_than_1024_tiles(T):
    """From 1024 (image, tile, group) units on, one workgroup of the forward walks all channel chunks of its group
    instead of one: 2 x 128 x 256 source pixels are 1024 tiles of 8 x 8, and 128 channels are two chunks."""
    from torch_detection_amd import carafe_ops as D
    rng = np.random.default_rng(5)
    x = R.round16(rng.standard_normal((2, 128, 128, 256)), BF16)
    masks = R.round16(rng.uniform(0.0, 0.25, size=(2, 9, 128, 256)), BF16)
    got = D.carafe_forward(dev(x, BF16), 3, 1, 1, masks=dev(masks, BF16))
    assert np.array_equal(R.bits16(got.float().cpu().numpy(), BF16), R.bits16(R.forward(x, masks, 3, 1, 1, BF16), BF16))


# ---- (b), (c) the logits forward and the gradients, within the bound, under the guard ----------------------------------
@pytest.mark.parametrize("c", CC.CASES, ids=repr)
def test_logits_forward_and_gradients_within_the_bound_under_the_guard(T, guard, c):
    from torch_detection_amd import carafe_ops as D
    CC.make(c)
    x, masks, logits, gout, addend, wdt = operands(c, guard)
    shape = (c.N, c.C, c.H, c.W)
    f = R.Forward64(c.x, *kgs(c), logits=c.logits, out_size=c.out_size, addend=c.addend)
    got = D.carafe_forward(x, *kgs(c), logits=logits, out_size=c.out_size, addend=addend)
    within(nchw_np(got), f.v, f.S, f.T, c.dtype, "forward from logits")
    for name, kw, ref in (("masks", dict(masks=masks), R.Grads(c.x, c.gout, *kgs(c), masks=c.masks)),
                          ("logits", dict(logits=logits), R.Grads(c.x, c.gout, *kgs(c), logits=c.logits))):
        dx = D.carafe_feature_grad(gout, shape, *kgs(c), **kw)
        assert dx.dtype == c.dtype and tuple(dx.shape) == shape and dx.permute(0, 2, 3, 1).is_contiguous()
        within(nchw_np(dx), ref.dx, ref.S_dx, ref.T_dx, c.dtype, "dx from %s" % name)
        dw = D.carafe_mask_grad(gout, x, *kgs(c), **kw)
        src = logits if name == "logits" else masks
        assert dw.dtype == wdt and dw.shape == src.shape and dw.stride() == src.stride()
        if name == "logits":
            within(nchw_np(dw), ref.dlogits, ref.S_dlogits, ref.T_dlogits, wdt, "dlogits")
        else:
            within(nchw_np(dw), ref.dmasks, ref.S_dmasks, ref.T_dmasks, wdt, "dmasks")
            outside = np.ones(ref.dmasks.shape[2:], dtype=bool)
            outside[:c.out_size[0], :c.out_size[1]] = False
            assert not nchw_np(dw)[:, :, outside].any()                 # gout is zero outside the crop
    found = guard.check()                      # every output fully written (cropped ones too), nothing outside
    assert not found, found
    assert not guard.ws_log                    # no launch takes a workspace


def test_weights_read_and_written_through_the_pitch(T, guard):
    """Logits and masks as channel slices of wider NaN-filled buffers: the same bits as from dense tensors, and the
    gradient written into such a slice leaves the channels beyond it alone."""
    from torch_detection_amd import carafe_ops as D
    for dtype, w32 in ((BF16, False), (F16, True)):
        c = CC.custom(2, 128, 2, (7, 9), 5, 2, dtype, seed=11, out_size=(13, 18), with_addend=True, w32=w32)
        x, masks, logits, gout, addend, wdt = operands(c)
        shape = (c.N, c.C, c.H, c.W)

        def wide(t, pitch):
            N, ch, H, W = t.shape
            buf = torch.full((N, H, W, pitch), float("nan"), dtype=t.dtype, device="cuda").permute(0, 3, 1, 2)
            buf[:, :ch] = t
            return buf

        for name, dense, pitch in (("logits", logits, 256), ("masks", masks, 64)):
            buf = wide(dense, pitch)
            sl = buf[:, :dense.shape[1]]
            a = D.carafe_forward(x, *kgs(c), out_size=c.out_size, addend=addend, **{name: dense})
            assert same_bits(D.carafe_forward(x, *kgs(c), out_size=c.out_size, addend=addend, **{name: sl}), a)
            assert same_bits(D.carafe_feature_grad(gout, shape, *kgs(c), **{name: sl}),
                             D.carafe_feature_grad(gout, shape, *kgs(c), **{name: dense}))
            want = D.carafe_mask_grad(gout, x, *kgs(c), **{name: dense})
            got = D.carafe_mask_grad(gout, x, *kgs(c), **{name: sl})
            assert got.stride() == sl.stride() and same_bits(got, want)
            out = wide(torch.zeros_like(dense), pitch)
            D.carafe_mask_grad(gout, x, *kgs(c), out=out[:, :dense.shape[1]], **{name: sl})
            assert same_bits(out[:, :dense.shape[1]], want) and torch.isnan(out[:, dense.shape[1]:]).all()
    assert not guard.check()


# ---- (d) reproducibility ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_gradients_are_bitwise_reproducible_eager_and_replayed(T, dtype):
    from torch_detection_amd import carafe_ops as D
    c = CC.custom(2, 128, 2, (13, 17), 5, 2, dtype, seed=21, out_size=(25, 33), w32=False)
    x, _, logits, gout, _, _ = operands(c)
    shape = (c.N, c.C, c.H, c.W)

    def grads():
        return (D.carafe_feature_grad(gout, shape, *kgs(c), logits=logits),
                D.carafe_mask_grad(gout, x, *kgs(c), logits=logits))

    first = [g.clone() for g in grads()]
    assert all(torch.isfinite(g.float()).all() for g in first)
    for a, b in zip(first, grads()):
        assert same_bits(a, b)
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


# ---- (e) hand-placed inputs ---------------------------------------------------------------------------------------------
def test_one_hot_masks_reproduce_nearest_upsampling(T):
    from torch_detection_amd import carafe_ops as D
    for dtype, k, s in ((BF16, 5, 2), (F16, 3, 3), (BF16, 7, 4)):
        c = CC.custom(2, 64, 1, (7, 9), k, s, dtype, seed=31)
        m = np.zeros_like(c.masks)
        m[:, (k * k) // 2] = 1.0
        x = dev(c.x, dtype)
        got = D.carafe_forward(x, k, 1, s, masks=dev(m, F32))
        assert torch.equal(got, F.interpolate(x, scale_factor=s, mode="nearest"))
        # a one-hot on the tap to the left: the map shifted by one pixel, zeros in the first column
        m = np.zeros_like(c.masks)
        m[:, (k * k) // 2 - 1] = 1.0
        got = D.carafe_forward(x, k, 1, s, masks=dev(m, dtype))
        want = F.interpolate(F.pad(x, (1, 0))[..., :-1], scale_factor=s, mode="nearest")
        assert torch.equal(got, want)


def test_map_smaller_than_the_window(T, guard):
    from torch_detection_amd import carafe_ops as D
    for dtype, hw in ((BF16, (1, 1)), (F16, (2, 3)), (BF16, (3, 1))):
        c = CC.custom(2, 64, 2, hw, 7, 2, dtype, seed=41, w32=False)
        x, masks, logits, gout, _, wdt = operands(c, guard)
        got = D.carafe_forward(x, 7, 2, 2, masks=masks)
        assert np.array_equal(R.bits16(got.float().cpu().numpy(), dtype), R.bits16(R.forward(c.x, c.masks, 7, 2, 2, dtype), dtype))
        ref = R.Grads(c.x, c.gout, 7, 2, 2, logits=c.logits)
        within(nchw_np(D.carafe_feature_grad(gout, (2, 64) + hw, 7, 2, 2, logits=logits)), ref.dx, ref.S_dx, ref.T_dx, dtype,
               "dx %s" % (hw,))
        within(nchw_np(D.carafe_mask_grad(gout, x, 7, 2, 2, logits=logits)), ref.dlogits, ref.S_dlogits, ref.T_dlogits, wdt,
               "dlogits %s" % (hw,))
        assert not guard.check()


def test_saturated_softmax_gives_finite_outputs_and_exact_zero_gradients(T):
    """Logits of -80 with one +80 per (pixel, group, sub-pixel): every weight is 0 or 1 in float32."""
    from torch_detection_amd import carafe_ops as D
    for dtype, wdt, tiny in ((BF16, BF16, 2.0 ** -134), (F16, F16, 2.0 ** -25), (BF16, F32, 2.0 ** -150)):
        c = CC.custom(2, 64, 2, (7, 9), 5, 2, dtype, seed=51, out_size=(13, 17))
        rng = np.random.default_rng(52)
        l = np.full((c.N, c.g, 25, 4, c.H, c.W), -80.0, dtype=np.float32)
        hot = rng.integers(0, 25, size=(c.N, c.g, 1, 4, c.H, c.W))
        np.put_along_axis(l, hot, 80.0, axis=2)
        l = l.reshape(c.logits.shape)
        x, gout, logits = dev(c.x, dtype), dev(c.gout, dtype), dev(l, wdt)
        out = D.carafe_forward(x, 5, 2, 2, logits=logits, out_size=c.out_size)
        f = R.Forward64(c.x, 5, 2, 2, logits=l, out_size=c.out_size)
        assert torch.isfinite(out.float()).all()
        within(nchw_np(out), f.v, f.S, f.T, dtype, "saturated forward")
        ref = R.Grads(c.x, c.gout, 5, 2, 2, logits=l)
        dx = D.carafe_feature_grad(gout, (c.N, c.C, c.H, c.W), 5, 2, 2, logits=logits)
        dl = D.carafe_mask_grad(gout, x, 5, 2, 2, logits=logits)
        assert torch.isfinite(dx.float()).all() and torch.isfinite(dl.float()).all()
        within(nchw_np(dx), ref.dx, ref.S_dx, ref.T_dx, dtype, "saturated dx")
        small = np.abs(ref.dlogits) < tiny
        assert small.all()                                   # the construction: every exact gradient is below the store's reach
        assert not nchw_np(dl)[small].any()


# ---- (f) the autograd function ----------------------------------------------------------------------------------------
def test_carafe_function_against_the_oracle(T):
    for dtype, C, g, k, s in ((BF16, 64, 1, 5, 2), (F16, 128, 2, 3, 2)):
        c = CC.custom(2, C, g, (7, 9), k, s, dtype, seed=61)
        x = dev(c.x, dtype).requires_grad_()
        masks = torch.from_numpy(c.masks).cuda().requires_grad_()           # NCHW-contiguous float32, as a user hands it in
        y = T.carafe(x, masks, k, g, s)
        assert np.array_equal(R.bits16(y.detach().float().cpu().numpy(), dtype), R.bits16(R.forward(c.x, c.masks, k, g, s, dtype), dtype))
        y.backward(dev(c.gout, dtype))
        ref = R.Grads(c.x, c.gout, k, g, s, masks=c.masks)
        within(nchw_np(x.grad), ref.dx, ref.S_dx, ref.T_dx, dtype, "carafe(): dx")
        assert masks.grad.dtype == F32 and tuple(masks.grad.shape) == tuple(masks.shape)
        within(nchw_np(masks.grad), ref.dmasks, ref.S_dmasks, ref.T_dmasks, F32, "carafe(): dmasks")
        # only one operand differentiable
        y = T.carafe(x.detach(), masks, k, g, s)
        assert y.requires_grad
        assert not T.carafe(x.detach(), masks.detach(), k, g, s).requires_grad


# ---- (g) the modules against float64 autograd ---------------------------------------------------------------------------
class _Round(torch.autograd.Function):
    """A 16-bit store of the device chain: the value is rounded on the way forward, its cotangent on the way back."""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.to(dtype).double()

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).double(), None


class _RoundGrad(torch.autograd.Function):
    """One consumer of a stored value: the cotangent that consumer hands back is a 16-bit store of its own (the output
    convs' and the compressor's input gradients, the reassembly's feature gradient), before the sum with the others."""

    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).double(), None


def _rnd(t, dtype):
    return t if dtype is None else _Round.apply(t, dtype)


def _use(t, dtype):
    return t if dtype is None or not t.requires_grad else _RoundGrad.apply(t, dtype)


def _w16(w, dtype):
    """the packed 16-bit copy of a float32 master weight; its gradient stays unrounded (the device's is float32)"""
    return w if dtype is None else w + (w.to(dtype).double() - w).detach()


def pack_chain(x, p, pre, k, g, s, out_size, addend, dtype):
    comp = _rnd(F.conv2d(x, _w16(p[pre + "channel_compressor.weight"], dtype), p[pre + "channel_compressor.bias"]), dtype)
    logits = _rnd(F.conv2d(comp, _w16(p[pre + "content_encoder.weight"], dtype), p[pre + "content_encoder.bias"], padding=1),
                  dtype)
    # the feature gradient is stored in 16 bits before the compressor's input gradient adds it in its epilogue
    return _rnd(R.carafe_autograd(_use(x, dtype), R.normalize_autograd(logits, k, s), k, g, s, out_size, addend), dtype)


def fpn_chain(xs, p, levels, dtype):
    conv = lambda x, pre, **kw: _rnd(F.conv2d(x, _w16(p[pre + ".conv.weight"], dtype), p[pre + ".conv.bias"], **kw), dtype)
    lat = []
    for i in range(levels):
        if i < len(xs):
            lat.append(conv(xs[i], "lateral_convs.%d" % i))
        else:
            lat.append(conv(xs[-1] if i == len(xs) else _use(lat[-1], dtype), "lateral_convs.%d" % i, stride=2, padding=1))
    for i in range(levels - 1, 0, -1):
        lat[i - 1] = pack_chain(_use(lat[i], dtype), p, "upsample_modules.%d." % (i - 1), 5, 1, 2,
                                tuple(lat[i - 1].shape[2:]), lat[i - 1], dtype)
    return [conv(_use(lat[i], dtype), "fpn_convs.%d" % i, padding=1) for i in range(levels)]


def _randomise(module, seed):
    """Weights at which the logits spread like the cases' (std about 1.5), values any float32"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 4:
                fan = p.shape[1] * p.shape[2] * p.shape[3]
                p.copy_(torch.randn(p.shape, generator=g) * ((1.5 if "content_encoder" in name else 1.0) / fan ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)


def _compare(name, run_chain, module, got_outs, gys, dtype):
    """run_chain(params, dtype or None) -> outputs; compares outputs and parameter gradients of the device (already
    backpropagated) with float64 autograd, allowing twice the staged chain's own deviation"""
    res = {}
    for tag, dt in (("exact", None), ("staged", dtype)):
        p = {n: q.detach().double().cpu().requires_grad_() for n, q in module.named_parameters()}
        outs = run_chain(p, dt)
        torch.autograd.backward(outs, [gy.double().cpu() for gy in gys])
        res[tag] = dict([("out%d" % i, o.detach().numpy()) for i, o in enumerate(outs)] +
                        [(n, q.grad.numpy()) for n, q in p.items()])
    got = dict([("out%d" % i, nchw_np(o)) for i, o in enumerate(got_outs)] +
               [(n, nchw_np(q.grad)) for n, q in module.named_parameters()])
    rel = lambda a, e: float(np.abs(a - e).max() / np.abs(e).max())
    worst = 0.0
    for key in res["exact"]:
        e_oracle, e_gpu = rel(res["staged"][key], res["exact"][key]), rel(got[key], res["exact"][key])
        print("%s %s %-48s oracle staged %.3e   gpu %.3e" % (name, dtype, key, e_oracle, e_gpu))
        worst = max(worst, e_oracle)
        if e_oracle == 0.0:
            # a sum of the cotangent alone (an output conv's bias): the staged chain is exact there and twice that allows
            # nothing to an fp32 sum; it gets the a-priori bound of its N Ho Wo terms instead
            i = int(key.split(".")[1])
            assert key.startswith("fpn_convs.") and key.endswith(".bias")
            gy = gys[i].double().cpu().numpy()
            allow = R.allowance(res["exact"][key], np.abs(gy).sum((0, 2, 3)), gy.shape[0] * gy.shape[2] * gy.shape[3], F32)
            assert (np.abs(got[key] - res["exact"][key]) <= allow).all(), key
        else:
            assert e_gpu <= 2.0 * e_oracle, (key, e_gpu, e_oracle)
    print("%s %s worst staged deviation %.3e" % (name, dtype, worst))


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_carafe_pack_against_float64_autograd(T, dtype):
    """Every tensor's error against float64 autograd, relative to the tensor's maximum, is at most twice that of the
    oracle's own 16-bit-staged chain (measured figures: DESIGN.md §4t)."""
    rng = np.random.default_rng(71)
    m = T.CARAFEPack(64, 2).cuda()
    _randomise(m, 72)
    r16 = lambda a: torch.from_numpy(R.round16(a, dtype))
    x, add, gy = r16(rng.standard_normal((2, 64, 8, 10))), r16(rng.standard_normal((2, 64, 15, 19))), \
        r16(rng.standard_normal((2, 64, 15, 19)))
    xd = dev(x.numpy(), dtype)
    y = m(xd, out_size=(15, 19), addend=dev(add.numpy(), dtype))
    assert y.dtype == dtype and tuple(y.shape) == (2, 64, 15, 19)
    y.backward(dev(gy.numpy(), dtype))
    _compare("CARAFEPack", lambda p, dt: [pack_chain(x.double(), p, "", 5, 1, 2, (15, 19), add.double(), dt)], m, [y], [gy],
             dtype)
    # the plain call: full size, no addend
    y2 = m(xd)
    assert tuple(y2.shape) == (2, 64, 16, 20)
    p = {n: q.detach().double().cpu() for n, q in m.named_parameters()}
    exact, staged = (pack_chain(x.double(), p, "", 5, 1, 2, None, None, dt) for dt in (None, dtype))
    rel = lambda a: float((a - exact).abs().max() / exact.abs().max())
    print("CARAFEPack %s plain call: oracle staged %.3e   gpu %.3e" % (dtype, rel(staged), rel(y2.detach().double().cpu())))
    assert rel(y2.detach().double().cpu()) <= 2.0 * rel(staged)


@pytest.mark.parametrize("num_outs,dtype", [(3, BF16), (5, BF16), (5, F16)], ids=["3-bf16", "5-bf16", "5-f16"])
def test_fpn_carafe_against_float64_autograd(T, num_outs, dtype):
    rng = np.random.default_rng(81)
    n = T.FPN_CARAFE([64, 128, 256], 64, num_outs).cuda()
    _randomise(n, 82)
    r16 = lambda a: torch.from_numpy(R.round16(a, dtype))
    sizes = [(15, 19), (8, 10), (4, 5), (2, 3), (1, 2)][:num_outs]
    xs = [r16(rng.standard_normal((2, C) + hw)) for C, hw in zip((64, 128, 256), sizes)]
    gys = [r16(rng.standard_normal((2, 64) + hw)) for hw in sizes]
    outs = n([dev(x.numpy(), dtype) for x in xs])
    assert [tuple(o.shape) for o in outs] == [(2, 64) + hw for hw in sizes] and all(o.dtype == dtype for o in outs)
    torch.autograd.backward(outs, [dev(g.numpy(), dtype) for g in gys])
    _compare("FPN_CARAFE(%d)" % num_outs, lambda p, dt: fpn_chain([x.double() for x in xs], p, num_outs, dt), n, outs, gys,
             dtype)
    with pytest.raises(ValueError, match="smaller than the lateral"):
        n([dev(x.numpy(), dtype) for x in (xs[0], xs[1][:, :, :7], xs[2])])


# ---- (h) graph capture with a weight update ---------------------------------------------------------------------------
def test_carafe_pack_graph_capture_sees_a_weight_update(T):
    dtype = BF16
    rng = np.random.default_rng(91)
    m = T.CARAFEPack(64, 2).cuda()
    _randomise(m, 92)
    x = dev(R.round16(rng.standard_normal((2, 64, 13, 17)), dtype), dtype).requires_grad_()
    gy = dev(R.round16(rng.standard_normal((2, 64, 26, 34)), dtype), dtype)
    out = torch.zeros((2, 26, 34, 64), dtype=dtype, device="cuda").permute(0, 3, 1, 2)
    dx = torch.zeros((2, 13, 17, 64), dtype=dtype, device="cuda").permute(0, 3, 1, 2)

    def step():
        m.zero_grad(set_to_none=False)
        x.grad = None
        y = m(x)
        y.backward(gy)
        out.copy_(y.detach())
        dx.copy_(x.grad)

    def snapshot():
        torch.cuda.synchronize()
        return [out.clone(), dx.clone()] + [p.grad.clone() for p in m.parameters()]

    step()
    eager0 = snapshot()
    assert all(t.float().abs().max() > 0 and torch.isfinite(t.float()).all() for t in eager0)
    x.grad = None
    gs = T.GraphedStep(step, warmup=1, params=None)
    assert gs.captured, gs.error
    out.zero_()
    gs()
    for a, b in zip(eager0, snapshot()):
        assert same_bits(a, b)
    with torch.no_grad():
        m.content_encoder.weight.mul_(1.5)
        m.channel_compressor.bias.add_(0.25)
    gs()
    replayed = snapshot()
    assert not same_bits(replayed[0], eager0[0])
    step()
    for a, b in zip(replayed, snapshot()):
        assert same_bits(a, b)
    # invalidate_packed reaches the module's packed copies
    m.content_encoder.weight.data.mul_(0.5)            # no version bump
    T.invalidate_packed(m)
    step()
    assert not same_bits(snapshot()[0], replayed[0])
