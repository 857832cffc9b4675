"""GPU: the 2x2 stride-2 transposed convolution (csrc/deconv.hip) — every product through the wrappers of
deconv_ops.py against the fp64 oracle of tests/deconv_ref.py and the a-priori rounding bound of tests/bound_util.py, every
case under guard-banded, poisoned allocations with exact-size workspaces (tests/guard_util.py); bitwise reproducibility,
eager and graph-replayed; the ``conv_transpose2x2`` autograd node and its packed cache; ``FCNMaskHead`` against the same
layers called one by one, its row chunking, and one tiny training step end to end."""
import copy

import numpy as np
import pytest
import torch

import deconv_ref as R
import guard_util as G
import linear_ref as LR
import mask_cases as MC

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
FWD, DGRAD, WGRAD = 0, 1, 2
CL = torch.channels_last


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd as T
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need cuda:0")
    return T


@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import deconv_ops, linear_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, deconv_ops, g)
    G.install(monkeypatch, linear_ops, g)
    return g


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def nhwc(t):
    """logical (R, C, H, W) channels_last tensor -> its NHWC memory as an fp32 CPU tensor"""
    v = t.detach().permute(0, 2, 3, 1)
    assert v.is_contiguous()
    return v.float().cpu()


def nchw(t):
    """NHWC tensor -> the logical (R, C, H, W) view the ops take"""
    return t.permute(0, 3, 1, 2)


_CASES = {}


def case(shape, dtype):
    """CPU operands of one shape, made once: x NHWC, weight (Cin, Cout, 2, 2), bias, cotangent NHWC — fp32 containers of
    16-bit values.  Input pixel 0, the weight slice of output channel 0 and two bias entries are zero: exact-zero
    pre-activations occur beside both signs."""
    key = (shape, dtype)
    if key not in _CASES:
        Rr, H, W, Cin, Cout = shape
        g = torch.Generator().manual_seed(sum(p * s for p, s in zip((7, 5, 3, 2, 1), shape)))
        x = torch.randn(Rr, H, W, Cin, generator=g)
        w = torch.randn(Cin, Cout, 2, 2, generator=g) / Cin ** 0.5
        b = torch.randn(Cout, generator=g)
        gy = torch.randn(Rr, 2 * H, 2 * W, Cout, generator=g)
        if Rr:
            x[0, 0, 0] = 0
        w[:, 0] = 0
        b[0] = 0
        b[Cout - 1] = 0
        _CASES[key] = (R.round16(x, dtype), R.round16(w, dtype), b, R.round16(gy, dtype))
    return _CASES[key]


def on_gpu(guard, x, w, b, gy, dtype):
    """Guarded device copies with NaN bands around every input; activations as logical NCHW views of NHWC memory."""
    return (nchw(guard.guard_copy(x.to(dtype).cuda(), "x")), guard.guard_copy(w.cuda(), "weight"),
            guard.guard_copy(b.cuda(), "bias"), nchw(guard.guard_copy(gy.to(dtype).cuda(), "g")))


def wg_splits(splits, M):
    return min(splits, max(1, (M + 63) // 64))


SHAPES = [(1, 1, 1, 64, 64), (3, 5, 7, 128, 64), (5, 3, 9, 64, 192), (2, 14, 14, 256, 256), (0, 14, 14, 64, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_products_against_the_bound_under_the_guard(T, guard, dtype, shape):
    from torch_detection_amd import deconv_ops as D
    Rr, H, W, Cin, Cout = shape
    M = Rr * H * W
    x, w, b, gy = case(shape, dtype)
    x_, w_, b_, g_ = on_gpu(guard, x, w, b, gy, dtype)
    w_fwd, w_dgrad = D.pack_deconv_weight(w_, True, dtype)
    # the pack itself: exact
    assert tuple(w_fwd.shape) == (4 * Cout, Cin) and tuple(w_dgrad.shape) == (Cin, 4 * Cout)
    assert torch.equal(w_fwd.float().cpu(), R.w2d(w)) and torch.equal(w_dgrad.float().cpu(), R.w2d(w).T)
    only_fwd, none = D.pack_deconv_weight(w_, False, dtype)
    assert none is None and same_bits(only_fwd, w_fwd)
    ratios = {}
    for relu, bias in ((False, True), (True, True), (True, False)):
        y = D.deconv2x2_fwd(x_, w_fwd, b_ if bias else None, relu)
        assert tuple(y.shape) == (Rr, Cout, 2 * H, 2 * W) and y.dtype == dtype
        assert y.permute(0, 2, 3, 1).is_contiguous()
        if M:
            r = R.within(R.unshuffle(nhwc(y)), R.fwd_bound(x, w, b if bias else None, relu), dtype,
                         "fwd relu=%s bias=%s" % (relu, bias))
            ratios["fwd", relu, bias] = r["ratio"]
            if relu and bias:
                v = R.fwd(x, w, b, False)
                assert (v == 0).any() and (M == 1 or ((v > 0).any() and (v < 0).any()))
                assert (nhwc(y)[v == 0] == 0).all()
    dx = D.deconv2x2_dgrad(g_, w_dgrad)
    assert tuple(dx.shape) == (Rr, Cin, H, W) and dx.dtype == dtype and dx.permute(0, 2, 3, 1).is_contiguous()
    if M:
        ratios["dgrad"] = R.within(R.x2d(nhwc(dx)), R.dgrad_bound(gy, w), dtype, "dgrad")["ratio"]
    # weight and bias gradient: beta 0, then beta 1 into the same buffers (an exact doubling), then without dbias
    for splits in (0, 1, 3):
        ws = wg_splits(splits, M)
        dw, db = D.deconv2x2_wgrad(x_, g_, splits=ws)
        assert tuple(dw.shape) == (Cin, Cout, 2, 2) and tuple(db.shape) == (Cout,) and dw.dtype == db.dtype == torch.float32
        if splits and M:
            assert D.deconv2x2_plan(WGRAD, Rr, H, W, Cin, Cout, ws).slices == ws
        if M:
            ratios["wgrad", splits] = R.within(R.w2d(dw.cpu()), R.wgrad_bound(x, gy), torch.float32,
                                               "wgrad splits=%d" % splits)["ratio"]
            ratios["dbias", splits] = R.within(db, R.dbias_bound(gy), torch.float32, "dbias splits=%d" % splits)["ratio"]
        else:
            assert not dw.abs().sum().item() and not db.abs().sum().item()
        dw1, db1 = dw.clone(), db.clone()
        if not M:
            dw.fill_(1.5)
            db.fill_(-2.0)
            dw1, db1 = dw.clone(), db.clone()
        D.deconv2x2_wgrad(x_, g_, dw=dw, dbias=db, beta=1.0, splits=ws)
        if M:
            R.within(R.w2d(dw.cpu()), R.wgrad_bound(x, gy, mult=2.0), torch.float32, "wgrad beta=1")
            R.within(db, R.dbias_bound(gy, mult=2.0), torch.float32, "dbias beta=1")
        else:
            assert torch.equal(dw, dw1) and torch.equal(db, db1)          # beta * old
        dw2, none = D.deconv2x2_wgrad(x_, g_, want_dbias=False, splits=ws)
        assert none is None
        if M:
            assert same_bits(dw2, dw1)
    print("ratios", shape, dtype, {k: round(v, 4) for k, v in ratios.items()})
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log
    assert M == 0 or any(op == "deconv2x2_wgrad" for op, _, _ in guard.ws_log)


# ---- reproducibility --------------------------------------------------------------------------------------------------------
def _all_products(D, x, w, b, gy, dtype, splits):
    w_fwd, w_dgrad = D.pack_deconv_weight(w, True, dtype)
    y = D.deconv2x2_fwd(x, w_fwd, b, True)
    dx = D.deconv2x2_dgrad(gy, w_dgrad)
    dw, db = D.deconv2x2_wgrad(x, gy, splits=splits)
    return y, dx, dw, db


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("splits", [1, 3])
def test_twice_and_graph_replay_are_bit_identical(T, dtype, splits):
    from torch_detection_amd import deconv_ops as D
    shape = (3, 5, 7, 128, 64)
    splits = wg_splits(splits, 3 * 5 * 7)
    x, w, b, gy = case(shape, dtype)
    x, gy = nchw(x.to(dtype).cuda()), nchw(gy.to(dtype).cuda())
    w, b = w.cuda(), b.cuda()
    first = _all_products(D, x, w, b, gy, dtype, splits)
    second = _all_products(D, x, w, b, gy, dtype, splits)
    assert all(same_bits(a, c) for a, c in zip(first, second))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _all_products(D, x, w, b, gy, dtype, splits)        # the pack is a node: it reads the live fp32 weight
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    with torch.no_grad():
        w.mul_(-0.75)                                              # an in-place update between replays
        b.add_(0.5)
    graph.replay()
    eager = _all_products(D, x, w, b, gy, dtype, splits)
    assert all(same_bits(a, c) for a, c in zip(eager, held))
    assert not same_bits(first[0], held[0])


# ---- the autograd node --------------------------------------------------------------------------------------------------
def test_conv_transpose2x2_autograd_node_and_the_packed_cache(T):
    """``conv_transpose2x2``: a channels_last input is read in place, gradients come back in the input's layout; ReLU
    against the oracle with the mask applied; the packed copies follow the weight's version counter,
    ``invalidate_packed`` and the repack-in-capture rule."""
    from torch_detection_amd.deconv import _unit_for
    dtype, shape = BF16, (3, 5, 7, 128, 64)
    x, w, b, gy = case(shape, dtype)
    x_cl = nchw(x.to(dtype).cuda()).requires_grad_(True)
    assert x_cl.is_contiguous(memory_format=CL)
    x_nc = nchw(x.to(dtype).cuda()).contiguous().requires_grad_(True)
    wp, bp = torch.nn.Parameter(w.cuda()), torch.nn.Parameter(b.cuda())
    g_ = nchw(gy.to(dtype).cuda())
    outs = []
    for xi in (x_cl, x_nc):
        wp.grad = bp.grad = None
        y = T.conv_transpose2x2(xi, wp, bp, relu=True)
        if xi is x_cl:
            assert y.grad_fn.saved_tensors[0].data_ptr() == x_cl.data_ptr()      # no copy of the input
        y.backward(g_)
        outs.append((y.detach(), xi.grad, wp.grad, bp.grad))
    assert x_cl.grad.is_contiguous(memory_format=CL) and x_nc.grad.is_contiguous()
    assert tuple(outs[0][0].shape) == (3, 64, 10, 14) and outs[0][0].is_contiguous(memory_format=CL)
    for a, c in zip(outs[0], outs[1]):                                           # the layout of x changes no bit
        assert torch.equal(a.float().cpu(), c.float().cpu())
    yg = nhwc(outs[0][0])
    R.within(R.unshuffle(yg), R.fwd_bound(x, w, b, True), dtype, "conv_transpose2x2 fwd")
    yv = R.fwd(x, w, b, True)
    assert ((yv > 0) == (yg > 0)).float().mean() > 0.99
    ge = gy * (yg > 0)                                                           # the cotangent behind the GPU's own mask
    R.within(R.x2d(nhwc(outs[0][1])), R.dgrad_bound(ge, w), dtype, "conv_transpose2x2 dx")
    R.within(R.w2d(outs[0][2].cpu()), R.wgrad_bound(x, ge), torch.float32, "conv_transpose2x2 dw")
    R.within(outs[0][3], R.dbias_bound(ge), torch.float32, "conv_transpose2x2 dbias")
    # without ReLU and without bias
    y0 = T.conv_transpose2x2(x_cl, wp)
    R.within(R.unshuffle(nhwc(y0)), R.fwd_bound(x, w), dtype, "conv_transpose2x2 plain")
    # the cache: same version -> same packed tensors; an in-place update -> repacked; invalidate_packed reaches it
    u = _unit_for(wp, dtype)
    key, held = u.key, u.w_fwd
    T.conv_transpose2x2(x_cl, wp, bp)
    assert u.key == key and u.w_fwd is held
    with torch.no_grad():
        wp.mul_(2.0)
    y2 = T.conv_transpose2x2(x_cl, wp, bp)
    assert u.key != key and u.w_fwd is held                                      # repacked in place
    R.within(R.unshuffle(nhwc(y2)), R.fwd_bound(x, 2 * w, b), dtype, "conv_transpose2x2 after an update")
    m = torch.nn.Module()
    m.w = wp
    T.invalidate_packed(m)
    assert u.key is None
    # inside a capture the pack is enqueued again, so a replay after an update computes with the new weight
    T.conv_transpose2x2(x_cl, wp, bp)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        yc = T.conv_transpose2x2(x_cl, wp, bp)
    with torch.no_grad():
        wp.mul_(0.5)
    graph.replay()
    with torch.no_grad():
        assert same_bits(yc, T.conv_transpose2x2(x_cl, wp, bp))
    R.within(R.unshuffle(nhwc(yc)), R.fwd_bound(x, w, b), dtype, "conv_transpose2x2 replayed after an update")


# ---- FCNMaskHead ------------------------------------------------------------------------------------------------------------
def _small_head(T, seed=3, **kw):
    torch.manual_seed(seed)
    args = dict(num_convs=2, in_channels=64, conv_out_channels=64, num_classes=5)
    args.update(kw)
    head = T.FCNMaskHead(**args).cuda()
    with torch.no_grad():                                   # biases away from 0
        for p in (head.upsample.bias, head.conv_logits.bias):
            p.normal_(0, 0.1)
    return head


def _tail_by_hand(D, L, x, wu, bu, wl, bl, gz, dtype, chunks):
    """The tail through the public raw ops, the logits' rows cut at ``chunks``: -> (z2, y2, dx, dwu, dbu, dwl, dbl)"""
    ncls, Cout = wl.shape[0], wl.shape[1]
    uf, ud = D.pack_deconv_weight(wu, True, dtype)
    lf, ld = L.pack_linear_weight(wl.view(ncls, Cout), None, True, dtype)
    y = D.deconv2x2_fwd(x, uf, bu, True)
    Rr, _, H2, W2 = y.shape
    y2 = y.permute(0, 2, 3, 1).reshape(-1, Cout)
    z2 = torch.cat([L.linear_fwd(y2[s:e], lf, ncls, bl) for s, e in chunks])
    g2 = gz.permute(0, 2, 3, 1).reshape(-1, ncls)
    dwl = dbl = None
    gys = []
    for i, (s, e) in enumerate(chunks):
        dwl, dbl = L.linear_wgrad(y2[s:e], g2[s:e], dw=dwl, dbias=dbl, beta=1.0 if i else 0.0)
        gys.append(L.linear_dgrad(g2[s:e], ld, mask_src=y2[s:e]))
    gy = torch.cat(gys).view(Rr, H2, W2, Cout).permute(0, 3, 1, 2)
    dwu, dbu = D.deconv2x2_wgrad(x, gy)
    dx = D.deconv2x2_dgrad(gy, ud)
    return z2, y2, gy, dx, dwu, dbu, dwl.view(wl.shape), dbl


@pytest.mark.parametrize("agnostic", [False, True], ids=["classes", "agnostic"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_mask_head_is_the_chain_of_its_layers(T, guard, dtype, agnostic):
    from torch_detection_amd import deconv_ops as D, linear_ops as L
    Rr, S = 6, 14
    head = _small_head(T, class_agnostic=agnostic)
    ncls = 1 if agnostic else 5
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(Rr, 64, S, S, generator=g).cuda().to(dtype).contiguous(memory_format=CL)
    gz = torch.randn(Rr, ncls, 2 * S, 2 * S, generator=g).cuda().to(dtype).contiguous(memory_format=CL)
    x = x0.clone().requires_grad_(True)
    z = head(x)
    assert tuple(z.shape) == (Rr, ncls, 2 * S, 2 * S) and z.dtype == dtype
    assert z.is_contiguous(memory_format=CL) and z.permute(0, 2, 3, 1).is_contiguous()      # channels_last strides
    z.backward(gz)
    got = [z.detach(), x.grad] + [p.grad.clone() for p in head.parameters()]
    # by hand: the ConvModules as autograd nodes of their own, the tail through the raw ops
    convs = copy.deepcopy(head.convs)
    xh = x0.clone().requires_grad_(True)
    h = xh
    for conv in convs:
        h = conv(h)
    wu, bu = head.upsample.weight.detach(), head.upsample.bias.detach()
    wl, bl = head.conv_logits.weight.detach(), head.conv_logits.bias.detach()
    M2 = Rr * 4 * S * S
    z2, y2, gy, dh, dwu, dbu, dwl, dbl = _tail_by_hand(D, L, h.detach(), wu, bu, wl, bl, gz, dtype, [(0, M2)])
    h.backward(dh)
    want = [z2.view(Rr, 2 * S, 2 * S, ncls).permute(0, 3, 1, 2), xh.grad] + [p.grad for p in convs.parameters()] + \
           [dwu, dbu, dwl, dbl]
    assert len(got) == len(want)
    for i, (a, c) in enumerate(zip(got, want)):
        assert same_bits(a.contiguous(), c.contiguous()), "output %d of the head differs from the chain" % i
    assert x.grad.is_contiguous(memory_format=CL)
    # every launch of the tail within its bound, fed the GPU's own stored inputs
    f = lambda t: t.detach().float().cpu()
    WU, WL = R.round16(wu, dtype), R.round16(wl.view(ncls, 64), dtype)
    hx = nhwc(h)
    R.within(R.unshuffle(f(y2).view(Rr, 2 * S, 2 * S, 64)), R.fwd_bound(hx, WU, f(bu), True), dtype, "upsample")
    LR.within(z2, LR.fwd_bound(f(y2), WL, f(bl)), dtype, "conv_logits")
    g2 = f(gz.permute(0, 2, 3, 1).reshape(-1, ncls))
    LR.within(dwl.view(ncls, 64), LR.wgrad_bound(f(y2), g2), torch.float32, "conv_logits dw")
    LR.within(dbl, LR.dbias_bound(g2), torch.float32, "conv_logits dbias")
    LR.within(gy.permute(0, 2, 3, 1).reshape(-1, 64), LR.dgrad_bound(g2, WL, None, f(y2)), dtype, "conv_logits dx (masked)")
    gyc = nhwc(gy)
    assert (gyc[f(y2).view(Rr, 2 * S, 2 * S, 64) <= 0] == 0).all()
    R.within(R.w2d(dwu.cpu()), R.wgrad_bound(hx, gyc), torch.float32, "upsample dw")
    R.within(dbu, R.dbias_bound(gyc), torch.float32, "upsample dbias")
    R.within(R.x2d(nhwc(dh)), R.dgrad_bound(gyc, WU), dtype, "upsample dx")
    # mask_head_loss takes the logits in place
    labels = torch.arange(Rr, device="cuda") % max(ncls - 1, 1) + (0 if agnostic else 1)
    targets = (torch.rand(Rr, 2 * S, 2 * S, generator=g) > 0.5).to(torch.uint8).cuda()
    loss = T.mask_head_loss(z.detach(), targets, labels, torch.ones(Rr, device="cuda"))
    assert torch.isfinite(loss).all() and loss.item() > 0
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log


def test_mask_head_row_chunking(T):
    """84 RoIs of 28 x 28 give 84 * 56 * 56 = 263 424 logits rows, more than the linear kernels' 2^18: the head cuts the
    rows, bit-identically to two hand-made chunks, and stays within the oracle's (cheap) bound."""
    from torch_detection_amd import deconv_ops as D, linear_ops as L
    from torch_detection_amd.heads import row_chunks
    dtype, Rr, S, C, ncls = BF16, 84, 28, 64, 3
    M2 = Rr * 4 * S * S
    assert M2 == 263424 and row_chunks(M2) == [(0, 1 << 18), (1 << 18, M2)] and (1 << 18) % 128 == 0
    head = _small_head(T, num_convs=0, num_classes=ncls, roi_feat_size=S)
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(Rr, C, S, S, generator=g).cuda().to(dtype).contiguous(memory_format=CL)
    gz = torch.randn(Rr, ncls, 2 * S, 2 * S, generator=g).cuda().to(dtype).contiguous(memory_format=CL)
    x = x0.clone().requires_grad_(True)
    z = head(x)
    z.backward(gz)
    wu, bu = head.upsample.weight.detach(), head.upsample.bias.detach()
    wl, bl = head.conv_logits.weight.detach(), head.conv_logits.bias.detach()
    z2, y2, gy, dx, dwu, dbu, dwl, dbl = _tail_by_hand(D, L, x0, wu, bu, wl, bl, gz, dtype, row_chunks(M2))
    got = [z.detach().permute(0, 2, 3, 1).reshape(M2, ncls), x.grad] + [p.grad for p in head.parameters()]
    for i, (a, c) in enumerate(zip(got, [z2, dx, dwu, dbu, dwl, dbl])):
        assert same_bits(a.contiguous(), c.contiguous()), "output %d of the head differs from the two chunks" % i
    f = lambda t: t.detach().float().cpu()
    WU, WL = R.round16(wu, dtype), R.round16(wl.view(ncls, C), dtype)
    xc, g2 = nhwc(x0), f(gz.permute(0, 2, 3, 1).reshape(M2, ncls))
    R.within(R.unshuffle(f(y2).view(Rr, 2 * S, 2 * S, C)), R.fwd_bound(xc, WU, f(bu), True, cheap=True), dtype, "upsample")
    LR.within(z2, LR.fwd_bound(f(y2), WL, f(bl), cheap=True), dtype, "conv_logits (two chunks)")
    LR.within(dwl.view(ncls, C), LR.wgrad_bound(f(y2), g2, cheap=True), torch.float32, "conv_logits dw (two chunks)")
    LR.within(dbl, LR.dbias_bound(g2), torch.float32, "conv_logits dbias (two chunks)")
    LR.within(gy.permute(0, 2, 3, 1).reshape(M2, C), LR.dgrad_bound(g2, WL, None, f(y2), cheap=True), dtype,
              "conv_logits dx (two chunks)")
    gyc = nhwc(gy)
    R.within(R.w2d(dwu.cpu()), R.wgrad_bound(xc, gyc, cheap=True), torch.float32, "upsample dw")
    R.within(dbu, R.dbias_bound(gyc), torch.float32, "upsample dbias")
    R.within(R.x2d(nhwc(dx)), R.dgrad_bound(gyc, WU, cheap=True), dtype, "upsample dx")


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _problem(T):
    """Two images, three / two star-shaped instances, 64 proposals each, a four-level pyramid of 64 channels."""
    g = np.random.default_rng(9)
    gt = np.array([[[30, 40, 120, 140], [130, 20, 230, 100], [60, 150, 200, 240]],
                   [[20, 20, 110, 90], [140, 120, 240, 230], [0, 0, 0, 0]]], np.float32)
    gt_counts = np.array([3, 2], np.int32)
    gt_labels = np.array([[3, 1, 4], [2, 4, 0]], np.int64)
    polys = []
    for b in range(2):
        inst = []
        for j in range(gt_counts[b]):
            x1, y1, x2, y2 = gt[b, j]
            rx, ry = (x2 - x1) / 2, (y2 - y1) / 2
            s = MC.star(0, 0, 0.6, 1.0, 12, 50 + 3 * b + j)
            inst.append([MC.flat(s * np.array([rx, ry], np.float32) + np.array([x1 + rx, y1 + ry], np.float32))])
        polys.append(inst)
    props = np.zeros((2, 64, 5), np.float32)
    for b in range(2):
        for k in range(64):
            if k < 40:
                props[b, k, :4] = gt[b, k % gt_counts[b]] + g.integers(-8, 9, 4)
            else:
                xy = g.uniform(0, 180, 2)
                props[b, k, :4] = [xy[0], xy[1], xy[0] + g.uniform(20, 70), xy[1] + g.uniform(20, 70)]
            props[b, k, 4] = 1.0 - k / 64
    counts = np.array([64, 50], np.int32)
    import test_gpu_roi_align as RA
    feats = [f.requires_grad_(True) for f in RA.feats_of(2, 64, [(256 // s, 256 // s) for s in (4, 8, 16, 32)], BF16, 17, 0.5)]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return [cuda(a) for a in (props, counts, gt, gt_labels, gt_counts)], [t.cuda() for t in T.pack_polygons(polys, 3)], feats


def _forward_backward(T, head, sample_in, pg, feats):
    num, npos = 32, 8
    out = T.sample_rois(*sample_in, num=num, pos_fraction=npos / num, seed=3)
    rois = out[0].view(2, num, 5)[:, :npos].reshape(-1, 5)
    labels = out[1].view(2, num)[:, :npos].reshape(-1)
    inds = out[5].view(2, num)[:, :npos].reshape(-1)
    targets, weights = T.mask_target(rois, inds, *pg, mask_size=28)
    x = T.roi_align(feats, rois, out_size=14, featmap_strides=(4, 8, 16, 32))
    pred = head(x)
    loss = T.mask_head_loss(pred, targets, labels, weights)
    grads = torch.autograd.grad(loss, list(head.parameters()) + feats)
    return [weights, pred, loss] + list(grads)


def _end_to_end(T):
    sample_in, pg, feats = _problem(T)
    head = _small_head(T, seed=7)
    opt = T.SGD(head.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, modules=[head])
    out = _forward_backward(T, head, sample_in, pg, feats)
    n = len(list(head.parameters()))
    for p, gp in zip(head.parameters(), out[3:3 + n]):
        p.grad = gp.clone()
    opt.step()
    torch.cuda.synchronize()
    return head, out, [p.detach().clone() for p in head.parameters()]


def test_roi_align_mask_head_loss_backward_sgd_end_to_end(T):
    head, out, params = _end_to_end(T)
    weights, pred, loss = out[:3]
    n = len(params)
    assert tuple(pred.shape) == (16, 5, 28, 28) and pred.permute(0, 2, 3, 1).is_contiguous()
    assert int((weights > 0).sum()) >= 4
    assert torch.isfinite(loss).all() and loss.item() > 0
    for (name, p), gp in zip(head.named_parameters(), out[3:3 + n]):
        assert gp.dtype == torch.float32 and gp.shape == p.shape, name
        assert torch.isfinite(gp).all() and gp.abs().sum().item() > 0, name
    assert any(bool(t.float().abs().sum().item() > 0) for t in out[3 + n:])     # on through roi_align into the pyramid
    # a second identical run: identical bits
    _, again, params2 = _end_to_end(T)
    for a, c in zip(out + params, again + params2):
        assert same_bits(a, c)
    # the step moved every parameter
    fresh = _small_head(T, seed=7)
    assert all(not torch.equal(a, c.detach()) for a, c in zip(params, fresh.parameters()))
    # forward + backward captured in a graph: the replay matches eager bit for bit
    sample_in, pg, feats = _problem(T)
    head = _small_head(T, seed=7)
    step = lambda: _forward_backward(T, head, sample_in, pg, feats)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    with torch.no_grad():
        for t in captured:
            t.zero_()
    graph.replay()
    eager = step()
    torch.cuda.synchronize()
    for k, (a, c) in enumerate(zip(captured, eager)):
        assert same_bits(a, c), k
    for a, c in zip(captured, out):
        assert same_bits(a, c)
    # test time: the same head's logits go into mask_head_masks
    with torch.no_grad():
        dets = torch.tensor([[[30, 40, 120, 140, 0.9], [130, 20, 230, 100, 0.8]]], device="cuda")
        rois = T.rois_from_detections(dets, torch.tensor([2], dtype=torch.int32, device="cuda"))
        x = T.roi_align([f.detach()[:1] for f in feats], rois, out_size=14, featmap_strides=(4, 8, 16, 32))
        masks = T.mask_head_masks(head(x), dets, torch.tensor([[0, 2]], device="cuda"),
                                  torch.tensor([2], dtype=torch.int32, device="cuda"), (256, 256))
    assert tuple(masks.shape) == (2, 256, 256) and masks.dtype == torch.uint8


def _trainer(T):
    """The whole training step on static gradient buffers: forward, backward, gradients into ``p.grad``, ``SGD.step``."""
    sample_in, pg, feats = _problem(T)
    head = _small_head(T, seed=7)
    params = list(head.parameters())
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = T.SGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4, modules=[head])

    def step():
        out = _forward_backward(T, head, sample_in, pg, feats)
        with torch.no_grad():
            for p, gp in zip(params, out[3:3 + len(params)]):
                p.grad.copy_(gp)
        opt.step()
        return out

    return params, step


def test_whole_training_step_replayed_from_a_graph(T):
    """roi_align -> FCNMaskHead -> mask_head_loss -> backward -> SGD.step captured as ONE graph: a replay is the second
    training step, bit for bit what two eager steps give (the packed weights are re-derived inside the graph)."""
    params, step = _trainer(T)
    step()
    second = [t.clone() for t in step()]
    torch.cuda.synchronize()
    want = [p.detach().clone() for p in params]
    params, step = _trainer(T)
    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, c) in enumerate(zip(captured, second)):
        assert same_bits(a, c), k
    for a, c in zip(params, want):
        assert same_bits(a, c)
    assert not same_bits(second[1], _end_to_end(T)[1][1])            # the second step saw updated weights
