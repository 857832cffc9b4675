"""GPU: the fully connected layers (csrc/linear.hip) — every product through the wrappers of linear_ops.py
against the fp64 oracle of tests/linear_ref.py and the a-priori rounding bound of tests/bound_util.py, every case under
guard-banded, poisoned allocations with exact-size workspaces (tests/guard_util.py); bitwise reproducibility, eager and
graph-replayed; BBoxHead against the same layers chained by hand; and one tiny training step end to end."""
import pytest
import torch

import guard_util as G
import linear_ref as R

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
FWD, DGRAD, WGRAD = 0, 1, 2


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd as T
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need cuda:0")
    return T


@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import linear_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, linear_ops, g)
    return g


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


_CASES = {}


def case(M, K, O, dtype, C=None):
    """CPU operands of one shape, made once: x (memory order), w (logical order), bias, cotangent — fp32 containers of
    16-bit values.  Row 0 of x, row 0 of w and two bias entries are zero: exact-zero pre-activations occur beside both
    signs, and the mask (x > 0) sees zeros, negatives and positives."""
    key = (M, K, O, dtype, C)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * M + K + O)
        x = torch.randn(M, K, generator=g)
        w = torch.randn(O, K, generator=g) / K ** 0.5
        b = torch.randn(O, generator=g)
        gy = torch.randn(M, O, generator=g)
        if M:
            x[0] = 0
        if O > 1:
            w[0] = 0
        b[0] = 0
        b[O - 1] = 0
        _CASES[key] = (R.round16(x, dtype), R.round16(w, dtype), b, R.round16(gy, dtype))
    return _CASES[key]


def on_gpu(guard, x, w, b, gy, dtype):
    """Guarded device copies: NaN bands around every input, the 81-column cotangent among them."""
    return (guard.guard_copy(x.to(dtype).cuda(), "x"), guard.guard_copy(w.cuda(), "weight"),
            guard.guard_copy(b.cuda(), "bias"), guard.guard_copy(gy.to(dtype).cuda(), "g"))


def wg_splits(splits, M):
    return min(splits, max(1, (M + 63) // 64))


SHAPES = [((1, 64, 1), 0, None), ((130, 448, 81), 1, None), ((130, 448, 81), 3, None), ((130, 448, 81), 7, None),
          ((64, 1024, 324), 0, None), ((257, 3136, 64), 0, 64), ((0, 64, 81), 0, None),
          ((130, 448, 128), 0, None)]      # the last one: unsplit, O % 64 == 0 — forward and dgrad go to the conv GEMM


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("shape, splits, C", SHAPES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_products_against_the_bound_under_the_guard(T, guard, dtype, shape, splits, C):
    from torch_detection_amd import linear_ops as L
    M, K, O = shape
    x, w, b, gy = case(M, K, O, dtype, C)
    dx_, dw_, db_, dg_ = on_gpu(guard, x, w, b, gy, dtype)
    w_fwd, w_dgrad = L.pack_linear_weight(dw_, C, True, dtype)
    assert L.linear_plan(FWD, M, O, K, splits).conv == (1 if O == 128 else 0)
    # the pack itself: exact, pad rows zero
    wp = R.pack_w(w, C)
    assert torch.equal(w_fwd.float().cpu()[:O], wp) and not w_fwd[O:].float().abs().sum().item()
    assert torch.equal(w_dgrad.float().cpu()[:, :O], wp.T) and not w_dgrad[:, O:].float().abs().sum().item()
    ratios = {}
    # forward: ReLU on and off, with and without bias, 16-bit and fp32 output
    for relu, bias, f32 in ((False, True, False), (True, True, False), (True, False, False), (False, True, True)):
        y = L.linear_fwd(dx_, w_fwd, O, db_ if bias else None, relu, f32, splits)
        assert tuple(y.shape) == (M, O) and y.dtype == (torch.float32 if f32 else dtype)
        if M:
            r = R.within(y, R.fwd_bound(x, w, b if bias else None, relu, C), y.dtype, "fwd relu=%s bias=%s" % (relu, bias))
            ratios["fwd", relu, bias, f32] = r["ratio"]
            if relu and bias:
                v = R.fwd(x, w, b, False, C)
                assert (v == 0).any() and (M * O < 100 or ((v > 0).any() and (v < 0).any()))
                assert (y.float().cpu()[v == 0] == 0).all()
    # input gradient, with and without the mask
    for masked in (False, True):
        dx = L.linear_dgrad(dg_, w_dgrad, dx_ if masked else None, splits)
        assert tuple(dx.shape) == (M, K) and dx.dtype == dtype
        if M:
            r = R.within(dx, R.dgrad_bound(gy, w, C, x if masked else None), dtype, "dgrad masked=%s" % masked)
            ratios["dgrad", masked] = r["ratio"]
            if masked:
                assert (dx.float().cpu()[x <= 0] == 0).all()
    # weight and bias gradient: beta 0, then beta 1 into the same buffers (an exact doubling), then without dbias
    ws = wg_splits(splits, M)
    dw, db = L.linear_wgrad(dx_, dg_, C, splits=ws)
    assert tuple(dw.shape) == (O, K) and tuple(db.shape) == (O,) and dw.dtype == db.dtype == torch.float32
    if M:
        ratios["wgrad"] = R.within(R.pack_w(dw.cpu(), C), R.wgrad_bound(x, gy), torch.float32, "wgrad")["ratio"]
        ratios["dbias"] = R.within(db, R.dbias_bound(gy), torch.float32, "dbias")["ratio"]
    else:
        assert not dw.abs().sum().item() and not db.abs().sum().item()
    dw1, db1 = dw.clone(), db.clone()
    L.linear_wgrad(dx_, dg_, C, dw=dw, dbias=db, beta=1.0, splits=ws)
    if M:
        R.within(R.pack_w(dw.cpu(), C), R.wgrad_bound(x, gy, mult=2.0), torch.float32, "wgrad beta=1")
        R.within(db, R.dbias_bound(gy, mult=2.0), torch.float32, "dbias beta=1")
    else:
        assert torch.equal(dw, dw1) and torch.equal(db, db1)          # beta * old
    dw2, none = L.linear_wgrad(dx_, dg_, C, want_dbias=False, splits=ws)
    assert none is None and same_bits(dw2, dw1)
    print("ratios", shape, splits, C, dtype, {k: round(v, 4) for k, v in ratios.items()})
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("splits", [1, 3])
def test_wgrad_forced_row_splits(T, guard, dtype, splits):
    from torch_detection_amd import linear_ops as L
    M, K, O = 130, 448, 81
    x, w, b, gy = case(M, K, O, dtype)
    dx_, _, _, dg_ = on_gpu(guard, x, w, b, gy, dtype)
    assert L.linear_plan(WGRAD, M, O, K, splits).slices == splits
    dw, db = L.linear_wgrad(dx_, dg_, splits=splits)
    R.within(dw, R.wgrad_bound(x, gy), torch.float32, "wgrad splits=%d" % splits)
    R.within(db, R.dbias_bound(gy), torch.float32, "dbias splits=%d" % splits)
    found = guard.check()
    assert not found, "\n".join(found)


def test_fc6_at_the_workloads_own_shape(T, guard):
    """fc6 of one image, the library's own decomposition: (512, 12544, 1024), C = 256, bf16, against the cheap bound."""
    from torch_detection_amd import linear_ops as L
    M, K, O, C, dtype = 512, 12544, 1024, 256, BF16
    x, w, b, gy = case(M, K, O, dtype, C)
    assert L.linear_plan(FWD, M, O, K).slices > 1
    dx_, dw_, db_, dg_ = on_gpu(guard, x, w, b, gy, dtype)
    w_fwd, w_dgrad = L.pack_linear_weight(dw_, C, True, dtype)
    y = L.linear_fwd(dx_, w_fwd, O, db_, True)
    r0 = R.within(y, R.fwd_bound(x, w, b, True, C, cheap=True), dtype, "fc6 fwd")
    dx = L.linear_dgrad(dg_, w_dgrad, dx_)
    r1 = R.within(dx, R.dgrad_bound(gy, w, C, x, cheap=True), dtype, "fc6 dgrad")
    dw, db = L.linear_wgrad(dx_, dg_, C)
    r2 = R.within(R.pack_w(dw.cpu(), C), R.wgrad_bound(x, gy, cheap=True), torch.float32, "fc6 wgrad")
    R.within(db, R.dbias_bound(gy), torch.float32, "fc6 dbias")
    print("fc6 ratios", r0["ratio"], r1["ratio"], r2["ratio"])
    found = guard.check()
    assert not found, "\n".join(found)


# ---- reproducibility --------------------------------------------------------------------------------------------------------
def _all_products(L, x, w, b, gy, dtype, splits, C=None):
    w_fwd, w_dgrad = L.pack_linear_weight(w, C, True, dtype)
    y = L.linear_fwd(x, w_fwd, w.shape[0], b, True, False, splits)
    dx = L.linear_dgrad(gy, w_dgrad, x, splits)
    dw, db = L.linear_wgrad(x, gy, C, splits=wg_splits(splits, x.shape[0]))
    return y, dx, dw, db


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("splits", [1, 3])
def test_twice_and_graph_replay_are_bit_identical(T, dtype, splits):
    from torch_detection_amd import linear_ops as L
    M, K, O = 130, 448, 81
    x, w, b, gy = [t.cuda() for t in case(M, K, O, dtype)]
    x, gy = x.to(dtype), gy.to(dtype)
    first = _all_products(L, x, w, b, gy, dtype, splits)
    second = _all_products(L, x, w, b, gy, dtype, splits)
    assert all(same_bits(a, c) for a, c in zip(first, second))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _all_products(L, x, w, b, gy, dtype, splits)        # the pack is a node: it reads the live fp32 weight
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    with torch.no_grad():
        w.mul_(-0.75)                                              # an in-place update between replays
        b.add_(0.5)
    graph.replay()
    eager = _all_products(L, x, w, b, gy, dtype, splits)
    assert all(same_bits(a, c) for a, c in zip(eager, held))
    assert not same_bits(first[0], held[0])


def test_linear_autograd_node_and_the_packed_cache(T):
    """``linear``: channels_last input read in place, gradients in the input's layout; the packed copies follow the
    weight's version counter, ``invalidate_packed`` and the repack-in-capture rule."""
    from torch_detection_amd.linear import _unit_for
    dtype, Rr, C, S, O = BF16, 70, 64, 7, 81
    K = C * S * S
    g = torch.Generator().manual_seed(5)
    xl = R.round16(torch.randn(Rr, C, S, S, generator=g), dtype)
    w = R.round16(torch.randn(O, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(O, generator=g)
    gy = R.round16(torch.randn(Rr, O, generator=g), dtype)
    x_cl = xl.cuda().to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    x_nc = xl.cuda().to(dtype).contiguous().requires_grad_(True)
    wp = torch.nn.Parameter(w.cuda())
    bp = torch.nn.Parameter(b.cuda())
    outs = []
    for xi in (x_cl, x_nc):
        wp.grad = bp.grad = None
        y = T.linear(xi, wp, bp, relu=True)
        y.backward(gy.cuda().to(dtype))
        outs.append((y.detach(), xi.grad, wp.grad, bp.grad))
    assert x_cl.grad.is_contiguous(memory_format=torch.channels_last) and x_nc.grad.is_contiguous()
    x_mem = xl.permute(0, 2, 3, 1).reshape(Rr, K)
    yv = R.fwd(x_mem, w, b, True, C)
    R.within(outs[0][0], R.fwd_bound(x_mem, w, b, True, C), dtype, "linear fwd (channels_last)")
    R.within(outs[1][0], R.fwd_bound(xl.reshape(Rr, K), w, b, True), dtype, "linear fwd (contiguous)")
    ge = gy * (outs[0][0].float().cpu() > 0)                      # the cotangent behind the GPU's own ReLU mask
    assert ((yv > 0) == (outs[0][0].float().cpu() > 0)).float().mean() > 0.99
    R.within(outs[0][1].permute(0, 2, 3, 1).reshape(Rr, K), R.dgrad_bound(ge, w, C), dtype, "linear dx")
    R.within(R.pack_w(outs[0][2].cpu(), C), R.wgrad_bound(x_mem, ge), torch.float32, "linear dw")
    R.within(outs[0][3], R.dbias_bound(ge), torch.float32, "linear dbias")
    # the cache: same version -> same packed tensors; an in-place update -> repacked; invalidate_packed reaches it
    u = _unit_for(wp, dtype, C)
    key = u.key
    T.linear(x_cl, wp, bp)
    assert u.key == key
    with torch.no_grad():
        wp.mul_(2.0)
    y2 = T.linear(x_cl, wp, bp)
    assert u.key != key
    R.within(y2, R.fwd_bound(x_mem, 2 * w, b, False, C), dtype, "linear fwd after an update")
    m = torch.nn.Module()
    m.w = wp
    T.invalidate_packed(m)
    assert u.key is None


# ---- BBoxHead ---------------------------------------------------------------------------------------------------------------
def _small_head(T, dtype, seed=3):
    torch.manual_seed(seed)
    head = T.BBoxHead(num_fcs=2, in_channels=64, fc_out_channels=128, roi_feat_size=7, num_classes=5).cuda()
    with torch.no_grad():                                   # biases away from 0, predictors large enough to matter
        for fc in list(head.shared_fcs) + [head.fc_cls, head.fc_reg]:
            fc.bias.normal_(0, 0.1)
        head.fc_cls.weight.mul_(10)
        head.fc_reg.weight.mul_(100)
    return head


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_bbox_head_is_the_chain_of_linears(T, dtype):
    Rr = 64
    head = _small_head(T, dtype)
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(Rr, 64, 7, 7, generator=g).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
    gc = torch.randn(Rr, 5, generator=g).cuda().to(dtype)
    gr = torch.randn(Rr, 20, generator=g).cuda().to(dtype)
    x = x0.clone().requires_grad_(True)
    cls, reg = head(x)
    assert cls.is_contiguous() and reg.is_contiguous() and cls.dtype == reg.dtype == dtype
    assert tuple(cls.shape) == (Rr, 5) and tuple(reg.shape) == (Rr, 20)
    torch.autograd.backward([cls, reg], [gc, gr])
    got = [cls.detach(), reg.detach(), x.grad] + [p.grad.clone() for p in head.parameters()]
    # by hand: three linear() nodes, the predictors stacked (one product: their input gradients add in fp32)
    ps = [p.detach().clone().requires_grad_(True) for p in head.parameters()]
    w0, b0, w1, b1, wc, bc, wr, br = ps
    xh = x0.clone().requires_grad_(True)
    h1 = T.linear(xh, w0, b0, relu=True)
    h2 = T.linear(h1, w1, b1, relu=True)
    h1.retain_grad()
    h2.retain_grad()
    y = T.linear(h2, torch.cat([wc, wr]), torch.cat([bc, br]))
    torch.autograd.backward([y[:, :5], y[:, 5:]], [gc, gr])
    want = [y[:, :5].detach(), y[:, 5:].detach(), xh.grad] + [p.grad for p in ps]
    for i, (a, c) in enumerate(zip(got, want)):
        assert same_bits(a, c), "output %d of the head differs from the chain" % i
    assert x.grad.is_contiguous(memory_format=torch.channels_last)
    # every layer of the chain within its bound, fed the GPU's own stored inputs
    f = lambda t: t.detach().float().cpu()
    W0, W1, WP = R.round16(w0, dtype), R.round16(w1, dtype), R.round16(torch.cat([wc, wr]), dtype)
    x_mem = f(x0.permute(0, 2, 3, 1).reshape(Rr, -1))
    R.within(h1, R.fwd_bound(x_mem, W0, f(b0), True, 64), dtype, "fc6")
    R.within(h2, R.fwd_bound(f(h1), W1, f(b1), True), dtype, "fc7")
    R.within(y, R.fwd_bound(f(h2), WP, f(torch.cat([bc, br]))), dtype, "predictors")
    gp = torch.cat([f(gc), f(gr)], 1)
    # dx of the predictors: the fp32 sum of fc_cls's and fc_reg's input gradients, rounded once
    R.within(h2.grad, R.dgrad_bound(gp, WP), dtype, "predictors' dx")
    exact = f(gc).double() @ R.round16(wc, dtype).double() + f(gr).double() @ R.round16(wr, dtype).double()
    assert torch.allclose(R.dgrad(gp, WP), exact, rtol=0, atol=1e-9)
    g2 = f(h2.grad) * (f(h2) > 0)
    R.within(h1.grad, R.dgrad_bound(g2, W1), dtype, "fc7 dx")
    g1 = f(h1.grad) * (f(h1) > 0)
    R.within(xh.grad.permute(0, 2, 3, 1).reshape(Rr, -1), R.dgrad_bound(g1, W0, 64), dtype, "fc6 dx")
    R.within(torch.cat([wc.grad, wr.grad]), R.wgrad_bound(f(h2), gp), torch.float32, "predictors' dw")
    R.within(torch.cat([bc.grad, br.grad]), R.dbias_bound(gp), torch.float32, "predictors' dbias")
    R.within(w1.grad, R.wgrad_bound(f(h1), g2), torch.float32, "fc7 dw")
    R.within(b1.grad, R.dbias_bound(g2), torch.float32, "fc7 dbias")
    R.within(R.pack_w(f(w0.grad), 64), R.wgrad_bound(x_mem, g1), torch.float32, "fc6 dw")
    R.within(b0.grad, R.dbias_bound(g1), torch.float32, "fc6 dbias")


def _end_to_end(T, seed):
    dtype, B, C, ncls, Rr = BF16, 2, 64, 5, 64
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, C, h, w, generator=g).cuda().to(dtype).contiguous(memory_format=torch.channels_last)
             .requires_grad_(True) for h, w in ((32, 48), (16, 24))]
    xy = torch.rand(Rr, 2, generator=g) * torch.tensor([120.0, 80.0])
    wh = torch.rand(Rr, 2, generator=g) * 60 + 4
    wh[::2] += 80                                            # large boxes: both levels are used
    rois = torch.cat([torch.arange(Rr).view(-1, 1).float() % B, xy, xy + wh], 1).contiguous().cuda()
    labels = torch.where(torch.rand(Rr, generator=g) < 0.4, torch.randint(1, ncls, (Rr,), generator=g), 0).cuda()
    lw = torch.ones(Rr).cuda()
    bt = torch.randn(Rr, 4, generator=g).cuda()
    bw = (labels > 0).float().view(-1, 1).expand(Rr, 4).contiguous()
    head = _small_head(T, dtype, seed=7)
    opt = T.SGD(head.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, modules=[head])
    x = T.roi_align(feats, rois, 7, (4, 8))
    cls, reg = head(x)
    losses = T.bbox_head_loss(cls, reg, labels, lw, bt, bw)
    losses.sum().backward()
    grads = [p.grad.clone() for p in head.parameters()]
    fgrads = [f.grad.clone() for f in feats]
    opt.step()
    torch.cuda.synchronize()
    return head, rois, losses.detach(), grads, fgrads, [p.detach().clone() for p in head.parameters()]


def test_roi_align_head_loss_backward_sgd_end_to_end(T):
    head, rois, losses, grads, fgrads, params = _end_to_end(T, 21)
    assert torch.isfinite(losses).all() and (losses > 0).all()
    for (name, p), gp in zip(head.named_parameters(), grads):
        assert gp.dtype == torch.float32 and gp.shape == p.shape, name
        assert torch.isfinite(gp).all() and gp.abs().sum().item() > 0, name
    for fg in fgrads:
        assert torch.isfinite(fg.float()).all() and fg.float().abs().sum().item() > 0
    again = _end_to_end(T, 21)
    assert same_bits(losses, again[2])
    for a, c in zip(grads + fgrads + params, again[3] + again[4] + again[5]):
        assert same_bits(a, c)
    # the step moved every parameter
    torch.manual_seed(7)
    fresh = _small_head(T, BF16, seed=7)
    assert all(not torch.equal(a, c.detach()) for a, c in zip(params, fresh.parameters()))
    # test time: the same head's outputs go into bbox_head_detections
    head.eval()
    with torch.no_grad():
        x = T.roi_align([torch.randn(2, 64, 32, 48).cuda().to(BF16).contiguous(memory_format=torch.channels_last),
                         torch.randn(2, 64, 16, 24).cuda().to(BF16).contiguous(memory_format=torch.channels_last)],
                        rois, 7, (4, 8))
        cls, reg = head(x)
        dets, labels, row_idx, counts = T.bbox_head_detections(
            rois, cls, reg, torch.tensor([[128, 192], [128, 192]], dtype=torch.int32).cuda(), score_thr=0.0)
    assert dets.shape[-1] == 5 and int(counts.sum()) > 0 and torch.isfinite(dets.float()).all()
