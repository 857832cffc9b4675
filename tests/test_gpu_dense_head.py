"""GPU: the dense head predictors (csrc/dense_head.hip) — every product through the wrappers of
dense_ops.py against the fp64 oracle of tests/dense_head_ref.py and the a-priori rounding bound of tests/bound_util.py,
every case under guard-banded, poisoned allocations with exact-size workspaces (tests/guard_util.py); bitwise
reproducibility, eager and graph-replayed; ``RPNHead`` against the same layers called one by one; one tiny training step
from the pyramid through ``loss`` to ``SGD.step``, and ``get_proposals`` on the same outputs."""
import numpy as np
import pytest
import torch

import dense_head_ref as R
import guard_util as G

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
    from torch_detection_amd import dense_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, dense_ops, g)
    return g


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def nhwc(t):
    """logical (B, C, H, W) channels_last tensor -> its NHWC memory as an fp32 CPU tensor"""
    v = t.detach().permute(0, 2, 3, 1)
    assert v.is_contiguous()
    return v.float().cpu()


def nchw(t):
    return t.permute(0, 3, 1, 2)


def row_tile():
    from torch_detection_amd import dense_ops as D
    return D.pred_plan(FWD, [1], 64, 3).rows_per_workgroup


# (B, [(H, W)]): odd sizes over several workgroups, a single row, eight levels several of them 1x1, row counts one
# below, at and one above the kernel's row tile (filled in from pred_plan), an empty batch; "long": 16,412 rows, more than
# the wgrad planner's 64 slices x 128 rows, so that a slice is three 128-row steps (the last slice's third holds 16 rows)
PYRAMIDS = {
    "four": (2, [(9, 8), (5, 4), (3, 2), (1, 1)]),
    "one": (1, [(1, 1)]),
    "eight": (1, [(5, 5), (1, 1), (3, 3), (1, 1), (2, 2), (1, 1), (1, 2), (1, 1)]),
    "tile": None,
    "empty": (0, [(4, 4), (2, 2)]),
    "long": (2, [(82, 100), (3, 2)]),
}
CASES = [("four", 3, 64), ("four", 1, 256), ("four", 4, 64), ("four", 9, 64), ("four", 12, 512), ("one", 3, 256),
         ("one", 12, 64), ("eight", 3, 64), ("eight", 9, 256), ("tile", 3, 256), ("tile", 4, 512), ("tile", 12, 64),
         ("empty", 3, 64), ("long", 3, 64), ("long", 12, 64)]


def pyramid(name):
    if name == "tile":
        rt = row_tile()
        assert rt == 128
        return 1, [(rt - 1, 1), (rt // 8, 8), ((rt + 1) // 3, 3)]          # 127, 128 and 129 rows
    return PYRAMIDS[name]


_CASES = {}


def case(name, A, C, dtype):
    """CPU operands of one case, made once: hidden maps NHWC with exact zeros and both signs, the two weights with a
    zero row, biases with two zero entries, cotangents NHWC — fp32 containers of 16-bit values."""
    key = (name, A, C, dtype)
    if key not in _CASES:
        B, sizes = pyramid(name)
        g = torch.Generator().manual_seed(1000 * A + C + len(sizes))
        hs = [torch.randn(B, H, W, C, generator=g) for H, W in sizes]
        for h in hs:
            h[torch.rand(h.shape, generator=g) < 0.25] = 0
        wc = torch.randn(A, C, generator=g) / C ** 0.5
        wr = torch.randn(4 * A, C, generator=g) / C ** 0.5
        wc[0] = 0
        bc, br = torch.randn(A, generator=g), torch.randn(4 * A, generator=g)
        bc[A - 1] = 0
        br[1] = 0
        gc = [torch.randn(B, H, W, A, generator=g) for H, W in sizes]
        gr = [torch.randn(B, H, W, 4 * A, generator=g) for H, W in sizes]
        r = lambda ts: [R.round16(t, dtype) for t in ts]
        _CASES[key] = (B, sizes, r(hs), R.round16(wc, dtype), bc, R.round16(wr, dtype), br, r(gc), r(gr))
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name,A,C", CASES, ids=["%s-A%d-C%d" % c for c in CASES])
def test_products_against_the_bound_under_the_guard(T, guard, name, A, C, dtype):
    from torch_detection_amd import dense_ops as D
    B, sizes, hs, wc, bc, wr, br, gc, gr = case(name, A, C, dtype)
    M = sum(B * H * W for H, W in sizes)
    dev = lambda ts, what: [nchw(guard.guard_copy(t.to(dtype).cuda(), "%s[%d]" % (what, l))) for l, t in enumerate(ts)]
    hs_, gc_, gr_ = dev(hs, "h"), dev(gc, "g_cls"), dev(gr, "g_reg")
    wc_, wr_ = guard.guard_copy(wc.cuda().view(A, C, 1, 1), "w_cls"), guard.guard_copy(wr.cuda().view(4 * A, C, 1, 1), "w_reg")
    bc_, br_ = guard.guard_copy(bc.cuda(), "bias_cls"), guard.guard_copy(br.cuda(), "bias_reg")
    # the pack: exact, zero padded; strided 2-D views of the parameters give the same bytes
    w_fwd, w_dgrad = D.pack_pred_weight(wc_, wr_, True, dtype)
    Op, Kp = -(-5 * A // 16) * 16, -(-5 * A // 32) * 32
    assert tuple(w_fwd.shape) == (Op, C) and tuple(w_dgrad.shape) == (C, Kp) and w_fwd.dtype == w_dgrad.dtype == dtype
    W = R.stack(wc, wr)
    assert torch.equal(w_fwd.float().cpu(), torch.cat([W, torch.zeros(Op - 5 * A, C)]))
    assert torch.equal(w_dgrad.float().cpu(), torch.cat([W, torch.zeros(Kp - 5 * A, C)]).T)
    wide_c, wide_r = torch.zeros(A, 2 * C, device="cuda"), torch.zeros(2 * C, 4 * A, device="cuda")
    wide_c[:, ::2] = wc_.view(A, C)
    wide_r[::2] = wr_.view(4 * A, C).T
    only_fwd, none = D.pack_pred_weight(wide_c[:, ::2], wide_r[::2].T, False, dtype)
    assert none is None and same_bits(only_fwd, w_fwd)
    ratios = {}
    # forward
    cls, reg = D.pred_fwd(hs_, w_fwd, bc_, br_)
    assert len(cls) == len(reg) == len(sizes)
    for (H, Wd), c, r in zip(sizes, cls, reg):
        assert tuple(c.shape) == (B, A, H, Wd) and tuple(r.shape) == (B, 4 * A, H, Wd) and c.dtype == r.dtype == dtype
        assert c.permute(0, 2, 3, 1).is_contiguous() and r.permute(0, 2, 3, 1).is_contiguous()      # dense, channels_last
    if M:
        got = R.stack_g([nhwc(c) for c in cls], [nhwc(r) for r in reg])
        ratios["fwd"] = R.within(got, R.fwd_bound(hs, wc, bc, wr, br), dtype, "pred_fwd")["ratio"]
    # dgrad: masked by the hidden map; exact zeros where h <= 0
    dhs = D.pred_dgrad(gc_, gr_, w_dgrad, hs_)
    for (H, Wd), d in zip(sizes, dhs):
        assert tuple(d.shape) == (B, C, H, Wd) and d.dtype == dtype and d.permute(0, 2, 3, 1).is_contiguous()
    if M:
        got = R.rows([nhwc(d) for d in dhs])
        ratios["dgrad"] = R.within(got, R.dgrad_bound(gc, gr, wc, wr, hs), dtype, "pred_dgrad")["ratio"]
        hrows = R.rows(hs)
        assert (hrows == 0).any() and (hrows < 0).any() and (hrows > 0).any()
        assert (got[hrows <= 0] == 0).all() and (got[hrows > 0] != 0).any()
    # a cotangent in another layout or dtype (NCHW float32 handed to .backward) is copied once: same bits
    dhs2 = D.pred_dgrad([t.float().contiguous() for t in gc_], [t.contiguous() for t in gr_], w_dgrad, hs_)
    assert all(same_bits(a, c) for a, c in zip(dhs, dhs2))
    # wgrad: the parameters' logical shapes, fp32
    dwc, dbc, dwr, dbr = D.pred_wgrad(hs_, gc_, gr_)
    assert tuple(dwc.shape) == (A, C, 1, 1) and tuple(dwr.shape) == (4 * A, C, 1, 1)
    assert tuple(dbc.shape) == (A,) and tuple(dbr.shape) == (4 * A,)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (dwc, dbc, dwr, dbr))
    if M:
        ratios["wgrad"] = R.within(R.stack(dwc.cpu(), dwr.cpu()), R.wgrad_bound(hs, gc, gr), torch.float32, "pred_wgrad")["ratio"]
        ratios["dbias"] = R.within(torch.cat([dbc, dbr]), R.dbias_bound(gc, gr), torch.float32, "pred_wgrad dbias")["ratio"]
        pl = D.pred_plan(WGRAD, [B * H * Wd for H, Wd in sizes], C, A)
        assert pl.slices == sum(-(-B * H * Wd // pl.rows_per_slice) for H, Wd in sizes)
        assert name != "long" or pl.rows_per_slice > pl.rows_per_workgroup     # several steps per wgrad workgroup
    else:
        assert all(not t.abs().sum().item() for t in (dwc, dbc, dwr, dbr))      # zeros, not poison
        assert all(t.numel() == 0 for t in cls + reg + dhs)
    print("ratios", name, A, C, dtype, {k: round(v, 4) for k, v in ratios.items()})
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log
    assert M == 0 or any(op == "pred_wgrad" for op, _, _ in guard.ws_log)


# ---- reproducibility ----------------------------------------------------------------------------------------------------
def _all_products(D, hs, wc, bc, wr, br, gc, gr, dtype):
    w_fwd, w_dgrad = D.pack_pred_weight(wc, wr, True, dtype)
    cls, reg = D.pred_fwd(hs, w_fwd, bc, br)
    dhs = D.pred_dgrad(gc, gr, w_dgrad, hs)
    return cls + reg + dhs + list(D.pred_wgrad(hs, gc, gr))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_twice_and_graph_replay_are_bit_identical(T, dtype):
    from torch_detection_amd import dense_ops as D
    B, sizes, hs, wc, bc, wr, br, gc, gr = case("four", 3, 64, dtype)
    cu = lambda ts: [nchw(t.to(dtype).cuda()) for t in ts]
    hs, gc, gr = cu(hs), cu(gc), cu(gr)
    wc, wr, bc, br = wc.cuda(), wr.cuda(), bc.cuda(), br.cuda()
    assert D.pred_plan(WGRAD, [B * H * W for H, W in sizes], 64, 3).slices > 1
    first = _all_products(D, hs, wc, bc, wr, br, gc, gr, dtype)
    second = _all_products(D, hs, wc, bc, wr, br, gc, gr, dtype)
    assert all(same_bits(a, c) for a, c in zip(first, second))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _all_products(D, hs, wc, bc, wr, br, gc, gr, dtype)     # the pack is a node: it reads the live fp32 weights
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    with torch.no_grad():
        wc.mul_(-0.75)                                                 # an in-place update between replays
        wr.add_(0.125)
        bc.add_(0.5)
    graph.replay()
    eager = _all_products(D, hs, wc, bc, wr, br, gc, gr, dtype)
    assert all(same_bits(a, c) for a, c in zip(eager, held))
    assert not same_bits(first[0], held[0])


# ---- RPNHead --------------------------------------------------------------------------------------------------------------
def _small_head(T, seed=3, **kw):
    torch.manual_seed(seed)
    args = dict(in_channels=64, feat_channels=64, anchor_strides=(4, 8, 16, 32))
    args.update(kw)
    head = T.RPNHead(**args).cuda()
    with torch.no_grad():                                   # weights large enough to matter, biases away from 0
        for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
            m.weight.mul_(8.0)
            m.bias.normal_(0, 0.1)
    return head


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_rpn_head_is_the_chain_of_its_layers(T, guard, dtype):
    from torch_detection_amd import dense_ops as D
    B, C, A = 2, 64, 3
    sizes = [(9, 8), (5, 4), (3, 2)]
    head = _small_head(T)
    g = torch.Generator().manual_seed(11)
    x0 = [torch.randn(B, C, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL) for H, W in sizes]
    x0[1] = x0[1].contiguous()                                           # one level in plain NCHW memory
    gcl = [torch.randn(B, A, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL) for H, W in sizes]
    grg = [torch.randn(B, 4 * A, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL) for H, W in sizes]
    grg[2] = grg[2].float().contiguous()                                 # an NCHW float32 cotangent: one copy
    xs = [x.clone().requires_grad_(True) for x in x0]
    xs[1] = x0[1].clone(memory_format=torch.contiguous_format).requires_grad_(True)
    cls, reg = head(xs)
    for (H, W), c, r in zip(sizes, cls, reg):
        assert tuple(c.shape) == (B, A, H, W) and tuple(r.shape) == (B, 4 * A, H, W) and c.dtype == r.dtype == dtype
        assert c.permute(0, 2, 3, 1).is_contiguous() and r.permute(0, 2, 3, 1).is_contiguous()
    # one autograd node; a channels_last input is not copied
    assert all(t.grad_fn is cls[0].grad_fn for t in cls + reg)
    saved = cls[0].grad_fn.saved_tensors
    assert saved[0].data_ptr() == xs[0].data_ptr() and saved[2].data_ptr() == xs[2].data_ptr()
    assert saved[1].data_ptr() != xs[1].data_ptr()
    torch.autograd.backward(cls + reg, gcl + grg)
    got = [t.detach() for t in cls + reg] + [x.grad for x in xs] + [p.grad.clone() for p in head.parameters()]
    # input gradients keep the input's layout
    assert xs[0].grad.is_contiguous(memory_format=CL) and xs[2].grad.is_contiguous(memory_format=CL)
    assert xs[1].grad.is_contiguous() and xs[1].grad.dtype == dtype
    # by hand: a ConvModule holding the same weights applied per level, then the raw ops
    conv = T.ConvModule(C, C, 3, padding=1, bias=True, activation='relu').cuda()
    with torch.no_grad():
        conv.conv.weight.copy_(head.rpn_conv.weight)
        conv.conv.bias.copy_(head.rpn_conv.bias)
    xh = [x.clone().requires_grad_(True) for x in x0]
    hs = [conv(x) for x in xh]
    hd = [h.detach() for h in hs]
    w_fwd, w_dgrad = D.pack_pred_weight(head.rpn_cls.weight.detach(), head.rpn_reg.weight.detach(), True, dtype)
    cls2, reg2 = D.pred_fwd(hd, w_fwd, head.rpn_cls.bias.detach(), head.rpn_reg.bias.detach())
    dwc, dbc, dwr, dbr = D.pred_wgrad(hd, gcl, grg)
    dhs = D.pred_dgrad(gcl, grg, w_dgrad, hd)
    # the module's own backward level by level; rpn_conv's gradients are the fp32 sum of its per-level gradients in
    # level order, finest first: ((g0 + g1) + g2)
    per_level = [torch.autograd.grad(h, [x, conv.conv.weight, conv.conv.bias], dh) for h, x, dh in zip(hs, xh, dhs)]
    dw3 = (per_level[0][1] + per_level[1][1]) + per_level[2][1]
    db3 = (per_level[0][2] + per_level[1][2]) + per_level[2][2]
    want = list(cls2) + list(reg2) + [g[0] for g in per_level] + [dw3, db3, dwc, dbc, dwr, dbr]
    assert len(got) == len(want) == 6 + 3 + 6
    for i, (a, c) in enumerate(zip(got, want)):
        assert same_bits(a.contiguous(), c.contiguous()), "output %d of the head differs from the chain" % i
    # every launch of the predictors within its bound, fed the GPU's own stored hidden maps
    f = lambda t: t.detach().float().cpu()
    hn = [nhwc(h) for h in hd]
    WC, WR = R.round16(head.rpn_cls.weight.view(A, C), dtype), R.round16(head.rpn_reg.weight.view(4 * A, C), dtype)
    gcn = [nhwc(t) for t in gcl]
    grn = [R.round16(t.permute(0, 2, 3, 1), dtype) for t in grg]
    R.within(R.stack_g([nhwc(t) for t in cls], [nhwc(t) for t in reg]),
             R.fwd_bound(hn, WC, f(head.rpn_cls.bias), WR, f(head.rpn_reg.bias)), dtype, "head fwd")
    R.within(R.rows([nhwc(d) for d in dhs]), R.dgrad_bound(gcn, grn, WC, WR, hn), dtype, "head dh")
    R.within(R.stack(f(dwc), f(dwr)), R.wgrad_bound(hn, gcn, grn), torch.float32, "head dw")
    assert all((nhwc(d)[h <= 0] == 0).all() for d, h in zip(dhs, hn)) and all((h == 0).any() for h in hn)
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log


def test_packed_predictor_weights_follow_the_version_counter(T):
    head = _small_head(T)
    x = [torch.randn(1, 64, 4, 4).cuda().to(BF16).contiguous(memory_format=CL)]
    with torch.no_grad():
        y0 = head(x)[0][0].clone()
        u = head._pred_unit(BF16)
        key, held = u.key, u.w_fwd
        head(x)
        assert u.key == key and u.w_fwd is held
        head.rpn_cls.weight.mul_(2.0)
        y1 = head(x)[0][0].clone()
        assert u.key != key and u.w_fwd is held and not same_bits(y0, y1)          # repacked in place
        T.invalidate_packed(head)
        assert u.key is None
        # inside a capture the pack is enqueued again: a replay after an update computes with the new weight
        head(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yc = head(x)[0][0]
        head.rpn_cls.weight.mul_(0.5)
        head.rpn_cls.bias.add_(0.25)
        graph.replay()
        assert same_bits(yc, head(x)[0][0])


# ---- end to end -------------------------------------------------------------------------------------------------------------
STRIDES = (4, 8, 16, 32)


def _problem(T, dtype=BF16):
    """Two 256 x 256 images, three / two ground truths — one of them large enough for the 256-pixel anchors of the
    coarsest level, which only take part without the image-border filter —, a four-level pyramid of 64 channels."""
    import test_gpu_roi_align as RA
    gt = np.array([[[30, 40, 120, 140], [130, 20, 230, 100], [8, 8, 247, 247]],
                   [[20, 20, 110, 90], [4, 12, 235, 250], [0, 0, 0, 0]]], np.float32)
    gt_counts = np.array([3, 2], np.int32)
    img_shapes = np.array([[256, 256], [256, 240]], np.int32)
    sizes = [(256 // s, 256 // s) for s in STRIDES]
    feats = [f.requires_grad_(True) for f in RA.feats_of(2, 64, sizes, dtype, 17, 0.5)]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return cuda(gt), cuda(gt_counts), cuda(img_shapes), sizes, feats


def _forward_backward(T, head, problem):
    gt, gt_counts, img_shapes, sizes, feats = problem
    cls, reg = head(feats)
    anchors, flags = head.get_anchors(sizes)
    losses = head.loss(cls, reg, anchors, flags, gt, gt_counts, img_shapes, num=256, allowed_border=-1, seed=3)
    grads = torch.autograd.grad(losses.sum(), list(head.parameters()) + feats)
    return list(cls) + list(reg) + [losses] + list(grads)


def _end_to_end(T, dtype=BF16):
    problem = _problem(T, dtype)
    head = _small_head(T, seed=7)
    opt = T.SGD(head.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, modules=[head])
    out = _forward_backward(T, head, problem)
    for p, gp in zip(head.parameters(), out[9:15]):
        p.grad = gp.clone()
    opt.step()
    torch.cuda.synchronize()
    return head, problem, out, [p.detach().clone() for p in head.parameters()]


def test_pyramid_rpn_head_loss_backward_sgd_end_to_end(T):
    head, problem, out, params = _end_to_end(T)
    sizes = problem[3]
    cls, reg, losses = out[:4], out[4:8], out[8]
    for (H, W), c, r in zip(sizes, cls, reg):
        assert tuple(c.shape) == (2, 3, H, W) and tuple(r.shape) == (2, 12, H, W)
        assert c.permute(0, 2, 3, 1).is_contiguous() and r.permute(0, 2, 3, 1).is_contiguous()
    assert tuple(losses.shape) == (2,) and torch.isfinite(losses).all() and (losses > 0).all()
    for (name, p), gp in zip(head.named_parameters(), out[9:15]):
        assert gp.dtype == torch.float32 and gp.shape == p.shape, name
        assert torch.isfinite(gp).all() and gp.abs().sum().item() > 0, name
    for f, gf in zip(problem[4], out[15:]):
        assert gf.shape == f.shape and gf.dtype == f.dtype and gf.is_contiguous(memory_format=CL)
        assert torch.isfinite(gf.float()).all() and gf.float().abs().sum().item() > 0
    # a second identical run: identical bits
    _, _, again, params2 = _end_to_end(T)
    for a, c in zip(out + params, again + params2):
        assert same_bits(a, c)
    # the step moved every parameter
    fresh = _small_head(T, seed=7)
    assert all(not torch.equal(a, c.detach()) for a, c in zip(params, fresh.parameters()))
    # forward + backward captured in one graph: the replay matches eager bit for bit
    problem = _problem(T)
    head = _small_head(T, seed=7)
    step = lambda: _forward_backward(T, head, problem)
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
    # test time: get_proposals takes the same outputs in place
    anchors, _ = head.get_anchors(sizes)
    with torch.no_grad():
        cls, reg = head([f.detach() for f in problem[4]])
        props, idx, counts = head.get_proposals(cls, reg, anchors, problem[2], nms_pre=200, nms_post=100, max_num=100)
    assert tuple(props.shape) == (2, 100, 5) and (counts > 0).all() and torch.isfinite(props).all()


def test_fp16_head_outputs_go_through_loss_and_proposals(T):
    """fp16 compute: the loss takes the outputs in place; ``get_proposals`` casts them to float32 (``rpn_proposals``
    takes float32 or bfloat16 only)."""
    head, problem, out, _ = _end_to_end(T, F16)
    assert out[0].dtype == F16 and torch.isfinite(out[8]).all() and (out[8] > 0).all()
    anchors, _ = head.get_anchors(problem[3])
    with torch.no_grad():
        cls, reg = head([f.detach() for f in problem[4]])
        props, idx, counts = head.get_proposals(cls, reg, anchors, problem[2], nms_pre=200, nms_post=100, max_num=100)
    assert (counts > 0).all() and torch.isfinite(props).all()
