"""GPU: the shared-weight 3x3 conv over a pyramid (csrc/pyramid_conv.hip) — every product through the
wrappers of pyramid_ops.py against the fp64 oracle of tests/pyramid_conv_ref.py and the a-priori rounding bound of
tests/bound_util.py, every case under guard-banded, poisoned allocations with exact-size workspaces
(tests/guard_util.py); bitwise reproducibility, eager and graph-replayed; one launch over a pyramid against single-level
launches; ``RetinaHead`` against its default route called op by op and, on the composed route, against the same oracle;
one tiny training step from the pyramid through ``loss`` to ``SGD.step``, ``get_bboxes`` on the same outputs, and a
captured forward + backward."""
import numpy as np
import pytest
import torch

import guard_util as G
import pyramid_conv_ref as R

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
    from torch_detection_amd import pyramid_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, pyramid_ops, g)
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


def tiles():
    from torch_detection_amd import pyramid_ops as P
    pl = P.pyramid_conv_plan(FWD, 1, [(1, 1)], 64, 1)
    return pl.pixels_per_workgroup, pl.cols_per_workgroup


# (B, [(H, W)]): odd sizes over several workgroups; a single pixel; maps one pixel wide or high, where every off-centre tap
# of a row or column is padding; eight levels, several of them 1x1; per-image pixel counts one below, at and one above the
# kernel's pixel tile (from the plan) with two images, so that a tile straddles rows and images, the widths 127 and 43 not
# dividing the tile; an empty batch; "long": 16,412 pixels, more than the wgrad planner's slice count x 128, so that a slice
# is three 128-pixel steps (the last slice's third holds 16 pixels)
PYRAMIDS = {
    "four": (2, [(9, 8), (5, 4), (3, 2), (1, 1)]),
    "one": (1, [(1, 1)]),
    "thin": (1, [(1, 7), (7, 1), (2, 2)]),
    "eight": (1, [(5, 5), (1, 1), (3, 3), (1, 1), (2, 2), (1, 1), (1, 2), (1, 1)]),
    "tile": None,
    "empty": (0, [(4, 4), (2, 2)]),
    "long": (2, [(82, 100), (3, 2)]),
}
# (pyramid, Cout, Cin): Cout 1, 9 (odd: 18-byte rows), 36, 80, one below / at / one above the column tile (64, asserted
# against the plan), 720 and 1024 once with Cin = 64; Cin 64, 256, 512
CASES = [("four", 1, 64), ("four", 9, 64), ("four", 36, 256), ("four", 80, 64), ("four", 63, 64), ("four", 64, 64),
         ("four", 65, 64), ("four", 9, 512), ("four", 720, 64), ("four", 1024, 64), ("one", 36, 256), ("one", 9, 64),
         ("thin", 9, 64), ("thin", 65, 256), ("eight", 36, 64), ("eight", 80, 512), ("tile", 9, 64), ("tile", 64, 256),
         ("tile", 65, 64), ("empty", 36, 64), ("long", 9, 64), ("long", 65, 64)]


def pyramid(name):
    if name == "tile":
        pt, ct = tiles()
        assert (pt, ct) == (128, 64)
        return 2, [(1, pt - 1), (8, pt // 8), (3, (pt + 1) // 3)]           # 127, 128 and 129 pixels per image
    return PYRAMIDS[name]


_CASES = {}


def case(name, Cout, Cin, dtype):
    """CPU operands of one case, made once: NHWC inputs with exact zeros and both signs, the weight with a zero row and
    a bias with zero entries (where there is more than one row), cotangents, mask sources (zeros, both signs) and addends — fp32 containers of 16-bit
    values."""
    key = (name, Cout, Cin, dtype)
    if key not in _CASES:
        B, sizes = pyramid(name)
        g = torch.Generator().manual_seed(1000 * Cout + Cin + len(sizes))
        mk = lambda ch: [torch.randn(B, H, W, ch, generator=g) for H, W in sizes]
        xs, gs, ms, ad = mk(Cin), mk(Cout), mk(Cin), mk(Cin)
        for t in xs + ms:
            t[torch.rand(t.shape, generator=g) < 0.25] = 0
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        b = torch.randn(Cout, generator=g)
        if Cout > 1:
            w[Cout // 2] = 0
            b[0] = 0
            b[Cout - 1] = 0
        r = lambda ts: [R.round16(t, dtype) for t in ts]
        _CASES[key] = (B, sizes, r(xs), R.round16(w, dtype), b, r(gs), r(ms), r(ad))
    return _CASES[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name,Cout,Cin", CASES, ids=["%s-O%d-C%d" % c for c in CASES])
def test_products_against_the_bound_under_the_guard(T, guard, name, Cout, Cin, dtype):
    from torch_detection_amd import pyramid_ops as P
    B, sizes, xs, w, b, gs, ms, ad = case(name, Cout, Cin, dtype)
    M = sum(B * H * W for H, W in sizes)
    dev = lambda ts, what: [nchw(guard.guard_copy(t.to(dtype).cuda(), "%s[%d]" % (what, l))) for l, t in enumerate(ts)]
    xs_, gs_, ms_, ad_ = dev(xs, "x"), dev(gs, "g"), dev(ms, "mask_src"), dev(ad, "addend")
    # the parameter as the modules keep it: channels_last memory
    w_ = nchw(guard.guard_copy(w.permute(0, 2, 3, 1).contiguous().cuda(), "w"))
    b_ = guard.guard_copy(b.cuda(), "bias")
    # the pack: exact, zero padded; a contiguous parameter and a strided view of a wider one give the same bytes
    w_fwd, w_dgrad = P.pack_pyramid_weight(w_, True, dtype)
    Cp = -(-Cout // 64) * 64
    assert tuple(w_fwd.shape) == (Cp, 3, 3, Cin) and tuple(w_dgrad.shape) == (Cin, 3, 3, Cp)
    assert w_fwd.dtype == w_dgrad.dtype == dtype and w_fwd.is_contiguous() and w_dgrad.is_contiguous()
    want_f = torch.zeros(Cp, 3, 3, Cin)
    want_f[:Cout] = w.permute(0, 2, 3, 1)
    want_d = torch.zeros(Cin, 3, 3, Cp)
    want_d[..., :Cout] = w.flip(2, 3).permute(1, 2, 3, 0)
    assert torch.equal(w_fwd.float().cpu(), want_f) and torch.equal(w_dgrad.float().cpu(), want_d)
    wide = torch.zeros(Cout, 2 * Cin, 3, 3, device="cuda")
    wide[:, 1::2] = w_
    only_fwd, none = P.pack_pyramid_weight(wide[:, 1::2], False, dtype)
    assert none is None and same_bits(only_fwd, w_fwd)
    both = P.pack_pyramid_weight(w_.contiguous(), True, dtype)
    assert same_bits(both[0], w_fwd) and same_bits(both[1], w_dgrad)
    ratios = {}
    worst = lambda recs: max([r["ratio"] for r in recs] or [0.0])
    # forward, ReLU off and on: exactly Cout channels per pixel, dense channels_last
    for relu in (False, True):
        ys = P.pyramid_conv_fwd(xs_, w_fwd, b_, Cout, relu)
        assert len(ys) == len(sizes)
        for (H, Wd), y in zip(sizes, ys):
            assert tuple(y.shape) == (B, Cout, H, Wd) and y.dtype == dtype and y.permute(0, 2, 3, 1).is_contiguous()
        if M:
            ratios["fwd%d" % relu] = worst([R.within(y, bd, dtype, "pyramid_conv_fwd relu=%d level %d" % (relu, l))
                                            for l, (y, bd) in enumerate(zip(ys, R.fwd_bounds(xs, w, b, relu)))])
            if relu:
                assert all((nhwc(y) >= 0).all() for y in ys) and any((nhwc(y) == 0).any() for y in ys)
    nobias = P.pyramid_conv_fwd(xs_, w_fwd, None, Cout)
    if M:
        [R.within(y, bd, dtype, "pyramid_conv_fwd without bias") for y, bd in zip(nobias, R.fwd_bounds(xs, w, None))]
    # dgrad: masked by the mask source, with and without the addend; exact zeros where the mask source is <= 0
    for tag, masks, adds, masks_, adds_ in (("dgrad+", ms, ad, ms_, ad_), ("dgrad", ms, None, ms_, None),
                                           ("dgrad0", None, None, None, None)):
        dxs = P.pyramid_conv_dgrad(gs_, w_dgrad, masks_, adds_)
        for (H, Wd), d in zip(sizes, dxs):
            assert tuple(d.shape) == (B, Cin, H, Wd) and d.dtype == dtype and d.permute(0, 2, 3, 1).is_contiguous()
        if M:
            ratios[tag] = worst([R.within(d, bd, dtype, "pyramid_conv_%s level %d" % (tag, l))
                                 for l, (d, bd) in enumerate(zip(dxs, R.dgrad_bounds(gs, w, masks, adds)))])
            if masks is not None:
                got, src = R.rows([nhwc(d) for d in dxs]), R.rows(ms)
                assert (src == 0).any() and (src < 0).any() and (src > 0).any()
                assert (got[src <= 0] == 0).all() and (got[src > 0] != 0).any()
    # a cotangent in another layout or dtype (NCHW float32 handed to .backward) is copied once: same bits
    dxs2 = P.pyramid_conv_dgrad([t.float().contiguous() for t in gs_], w_dgrad)
    assert all(same_bits(a, c) for a, c in zip(dxs, dxs2))
    # wgrad: the parameter's logical shape and, for a channels_last parameter, its memory layout; fp32
    dw, db = P.pyramid_conv_wgrad(xs_, gs_)
    assert tuple(dw.shape) == (Cout, Cin, 3, 3) and dw.stride() == w_.stride() and tuple(db.shape) == (Cout,)
    assert dw.dtype == db.dtype == torch.float32
    dw2, db2 = P.pyramid_conv_wgrad(xs_, gs_, channels_last=False)
    assert dw2.is_contiguous() and torch.equal(dw2, dw) and torch.equal(db2, db)
    if M:
        ratios["wgrad"] = R.within(dw, R.wgrad_bound(xs, gs), torch.float32, "pyramid_conv_wgrad")["ratio"]
        ratios["dbias"] = R.within(db, R.dbias_bound(gs), torch.float32, "pyramid_conv_wgrad dbias")["ratio"]
        pl = P.pyramid_conv_plan(WGRAD, B, sizes, Cin, Cout)
        assert pl.slices == sum(-(-B * H * Wd // pl.pixels_per_slice) for H, Wd in sizes)
        assert name != "long" or pl.pixels_per_slice > pl.pixels_per_workgroup   # several steps per wgrad workgroup
    else:
        assert not dw.abs().sum().item() and not db.abs().sum().item()         # zeros, not poison
        assert all(t.numel() == 0 for t in ys + dxs)
    print("ratios", name, Cout, Cin, dtype, {k: round(v, 4) for k, v in ratios.items()})
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log
    assert M == 0 or any(op == "pyramid_conv_wgrad" for op, _, _ in guard.ws_log)


# ---- reproducibility ----------------------------------------------------------------------------------------------------
def _all_products(P, xs, w, b, gs, ms, ad, dtype, Cout):
    w_fwd, w_dgrad = P.pack_pyramid_weight(w, True, dtype)
    ys = P.pyramid_conv_fwd(xs, w_fwd, b, Cout, True)
    dxs = P.pyramid_conv_dgrad(gs, w_dgrad, ms, ad)
    return ys + dxs + list(P.pyramid_conv_wgrad(xs, gs))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_twice_and_graph_replay_are_bit_identical(T, dtype):
    from torch_detection_amd import pyramid_ops as P
    B, sizes, xs, w, b, gs, ms, ad = case("tile", 9, 64, dtype)
    cu = lambda ts: [nchw(t.to(dtype).cuda()) for t in ts]
    xs, gs, ms, ad = cu(xs), cu(gs), cu(ms), cu(ad)
    w, b = w.cuda().contiguous(memory_format=CL), b.cuda()
    assert P.pyramid_conv_plan(WGRAD, B, sizes, 64, 9).slices > 1
    first = _all_products(P, xs, w, b, gs, ms, ad, dtype, 9)
    second = _all_products(P, xs, w, b, gs, ms, ad, dtype, 9)
    assert all(same_bits(a, c) for a, c in zip(first, second))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = _all_products(P, xs, w, b, gs, ms, ad, dtype, 9)        # the pack is a node: it reads the live fp32 weights
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    with torch.no_grad():
        w.mul_(-0.75)                                                  # an in-place update between replays
        b.add_(0.5)
    graph.replay()
    eager = _all_products(P, xs, w, b, gs, ms, ad, dtype, 9)
    assert all(same_bits(a, c) for a, c in zip(eager, held))
    assert not same_bits(first[0], held[0])


@pytest.mark.parametrize("name,Cout,Cin", [("four", 9, 64), ("tile", 65, 64), ("eight", 36, 64)])
def test_one_launch_over_the_pyramid_equals_single_level_launches(T, name, Cout, Cin):
    """Level boundaries do not leak: forward and input gradient of the pyramid are, bit for bit, those of every level
    given on its own."""
    from torch_detection_amd import pyramid_ops as P
    dtype = BF16
    B, sizes, xs, w, b, gs, ms, ad = case(name, Cout, Cin, dtype)
    cu = lambda ts: [nchw(t.to(dtype).cuda()) for t in ts]
    xs, gs, ms, ad = cu(xs), cu(gs), cu(ms), cu(ad)
    w_fwd, w_dgrad = P.pack_pyramid_weight(w.cuda(), True, dtype)
    b = b.cuda()
    ys = P.pyramid_conv_fwd(xs, w_fwd, b, Cout, True)
    dxs = P.pyramid_conv_dgrad(gs, w_dgrad, ms, ad)
    for l in range(len(sizes)):
        assert same_bits(ys[l], P.pyramid_conv_fwd([xs[l]], w_fwd, b, Cout, True)[0]), l
        assert same_bits(dxs[l], P.pyramid_conv_dgrad([gs[l]], w_dgrad, [ms[l]], [ad[l]])[0]), l


# ---- RetinaHead -----------------------------------------------------------------------------------------------------------
SIZES = [(9, 8), (5, 4), (3, 2)]


def _small_head(T, seed=3, **kw):
    torch.manual_seed(seed)
    args = dict(num_classes=4, in_channels=64, feat_channels=64, stacked_convs=2, scales_per_octave=3,
                anchor_strides=(8, 16, 32))
    args.update(kw)
    head = T.RetinaHead(**args).cuda()
    with torch.no_grad():                                   # weights large enough to matter, biases away from 0
        for p in head.parameters():
            if p.dim() == 4:
                p.mul_(6.0)
            else:
                p.normal_(0, 0.1)
    return head


def _inputs(dtype, seed=11, B=2, C=64, sizes=SIZES, A=9, ncls=3):
    g = torch.Generator().manual_seed(seed)
    x0 = [torch.randn(B, C, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL) for H, W in sizes]
    gcl = [torch.randn(B, A * ncls, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL) for H, W in sizes]
    grg = [torch.randn(B, 4 * A, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL) for H, W in sizes]
    return x0, gcl, grg


class _ByHand(object):
    """One shared 3x3 layer called op by op on the route ``routes`` names for its products: the pyramid kernels through
    ``pyramid_ops``, or the conv units level by level (a predictor: zero padded to 64 output channels, its outputs sliced
    and its cotangents padded by copies; the shared weight's gradient the fp32 level sum, finest level first)."""

    def __init__(self, T, conv, routes, relu, dtype):
        from torch_detection_amd import functional as HF
        from torch_detection_amd import pyramid_ops as P
        self.P, self.HF, self.routes, self.relu, self.dtype = P, HF, routes, relu, dtype
        self.w, self.b = conv.weight.detach(), conv.bias.detach()
        self.Cout = self.w.shape[0]
        self.Cp = -(-self.Cout // 64) * 64
        self.w_fwd, self.w_dgrad = P.pack_pyramid_weight(self.w, True, dtype)
        pc = torch.nn.Conv2d(self.w.shape[1], self.Cp, 3, padding=1).cuda()
        with torch.no_grad():
            pc.weight.zero_()
            pc.bias.zero_()
            pc.weight.data = pc.weight.data.contiguous(memory_format=CL)
            pc.weight[:self.Cout].copy_(self.w)
            pc.bias[:self.Cout].copy_(self.b)
        self.unit = HF.ConvUnit(pc, None, relu, dtype).refresh()

    def pad(self, gs):
        out = []
        for g in gs:
            p = torch.zeros(g.shape[0], g.shape[2], g.shape[3], self.Cp, dtype=g.dtype, device=g.device)
            p[..., :self.Cout] = g.permute(0, 2, 3, 1)
            out.append(p)
        return out

    def levels(self, route, maps):
        """(levels run level by level, levels of the one pyramid launch) — 'split': by ``heads.SPLIT_PIXELS``"""
        from torch_detection_amd import heads
        every = list(range(len(maps)))
        if route != "split":
            return (every, []) if route == "composed" else ([], every)
        big = [l for l in every if maps[l].shape[0] * maps[l].shape[2] * maps[l].shape[3] >= heads.SPLIT_PIXELS]
        return big, [l for l in every if l not in big]

    def fwd(self, xs):
        big, tail = self.levels(self.routes["fwd"], xs)
        out = [None] * len(xs)
        if tail:
            for l, y in zip(tail, self.P.pyramid_conv_fwd([xs[l] for l in tail], self.w_fwd, self.b, self.Cout, self.relu)):
                out[l] = y
        for l in big:
            y = self.HF.unit_fwd(self.unit, xs[l].permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
            out[l] = y[:, :self.Cout].contiguous(memory_format=CL) if self.Cp != self.Cout else y
        return out

    def dgrad(self, gs, mask_src=None, addend=None):
        big, tail = self.levels(self.routes["dgrad"], gs)
        pick = lambda ts, idx: None if ts is None else [ts[l] for l in idx]
        out = [None] * len(gs)
        if tail:
            for l, d in zip(tail, self.P.pyramid_conv_dgrad(pick(gs, tail), self.w_dgrad, pick(mask_src, tail),
                                                           pick(addend, tail))):
                out[l] = d
        for l, g in zip(big, self.pad(pick(gs, big))):
            a = addend[l].permute(0, 2, 3, 1) if addend is not None else None
            m = mask_src[l].permute(0, 2, 3, 1) if mask_src is not None else None
            out[l] = self.HF.unit_dgrad(self.unit, g, (g.shape[1], g.shape[2]), a, 1 if a is not None else 0,
                                        m).permute(0, 3, 1, 2)
        return out

    def wgrad(self, xs, gs):
        if self.routes["wgrad"] == "pyramid":
            return self.P.pyramid_conv_wgrad(xs, gs)
        per = [self.HF.unit_wgrad(self.unit, x.permute(0, 2, 3, 1), g) for x, g in zip(xs, self.pad(gs))]
        self.HF.join_side_stream(xs[0].device)
        dw, db = per[0]
        for gw, gb in per[1:]:
            dw, db = dw + gw, db + gb
        return dw[:self.Cout], db[:self.Cout]


def _chain_by_hand(T, head, routes, x0, gcl, grg, dtype):
    """-> (outputs, dfeats, parameter gradients in ``head.parameters()`` order, the saved maps of both chains)"""
    chains = []
    for tower, pred, kind in ((head.cls_convs, head.retina_cls, "cls"), (head.reg_convs, head.retina_reg, "reg")):
        chains.append([_ByHand(T, m.conv, routes["tower"], True, dtype) for m in tower] +
                      [_ByHand(T, pred, routes[kind], False, dtype)])
    acts = []
    for chain in chains:
        maps = [x0]
        for layer in chain:
            maps.append(layer.fwd(maps[-1]))
        acts.append(maps)
    grads, first = [], None
    for chain, maps, g in zip(chains, acts, (gcl, grg)):
        mine = []
        for i in reversed(range(len(chain))):
            mine.append(chain[i].wgrad(maps[i], g))
            g = chain[i].dgrad(g, mask_src=maps[i]) if i else chain[i].dgrad(g, addend=first)
        first = g
        grads.append(mine[::-1])
    params = []
    for mine in (grads[0][:-1], grads[1][:-1], grads[0][-1:], grads[1][-1:]):
        for dw, db in mine:
            params += [dw, db]
    return acts[0][-1] + acts[1][-1], first, params, acts


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_retina_head_is_its_default_route_called_op_by_op(T, guard, dtype):
    from torch_detection_amd import heads
    B, C, A = 2, 64, 9
    head = _small_head(T)
    assert head._routes is heads.RETINA_ROUTES
    x0, gcl, grg = _inputs(dtype)
    grg[2] = grg[2].float().contiguous()                                 # an NCHW float32 cotangent: one copy
    xs = [x.clone().requires_grad_(True) for x in x0]
    xs[1] = x0[1].float().contiguous().requires_grad_(True)              # one level as float32 NCHW
    if dtype == F16:
        head.compute_dtype = F16
    cls, reg = head(xs)
    for (H, W), c, r in zip(SIZES, cls, reg):
        assert tuple(c.shape) == (B, 3 * A, H, W) and tuple(r.shape) == (B, 4 * A, H, W) and c.dtype == r.dtype == dtype
        assert c.permute(0, 2, 3, 1).is_contiguous() and r.permute(0, 2, 3, 1).is_contiguous()
    assert all(t.grad_fn is cls[0].grad_fn for t in cls + reg)           # one autograd node
    torch.autograd.backward(cls + reg, gcl + grg)
    got = [t.detach() for t in cls + reg] + [x.grad for x in xs] + [p.grad for p in head.parameters()]
    # input gradients come back in the input's own dtype and layout
    assert xs[0].grad.is_contiguous(memory_format=CL) and xs[0].grad.dtype == dtype
    assert xs[1].grad.is_contiguous() and xs[1].grad.dtype == torch.float32
    for p in head.parameters():
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32
    # the chain by hand takes the cotangent as the head's one copy leaves it: compute dtype, channels_last
    grg[2] = grg[2].to(dtype).contiguous(memory_format=CL)
    outs, dfeats, params, _ = _chain_by_hand(T, head, heads.RETINA_ROUTES, x0, gcl, grg, dtype)
    dfeats = list(dfeats)
    dfeats[1] = dfeats[1].float().contiguous()
    want = outs + dfeats + params
    assert len(got) == len(want) == 6 + 3 + 12
    for i, (a, c) in enumerate(zip(got, want)):
        assert same_bits(a.contiguous(), c.contiguous()), "output %d of the head differs from the chain" % i
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log


@pytest.mark.parametrize("route", ["composed", "pyramid", "split"])
def test_retina_head_routes_stay_within_the_oracle_bounds(T, monkeypatch, route):
    """Every launch of a whole-route head within the a-priori bound of the same oracle, fed the GPU's own stored maps.
    'split' (forward and input gradient; the weight gradient composed) with the threshold lowered so that the finest
    level (144 pixels) runs level by level and the other two in one pyramid launch."""
    from torch_detection_amd import heads
    dtype = BF16
    routes = {k: {p: route for p in ("fwd", "dgrad", "wgrad")} for k in ("tower", "cls", "reg")}
    assert routes == heads.RETINA_COMPOSED or route != "composed"
    if route == "split":
        monkeypatch.setattr(heads, "SPLIT_PIXELS", 100)
        for k in routes:
            routes[k]["wgrad"] = "composed"
    head = _small_head(T)
    head._routes = routes
    x0, gcl, grg = _inputs(dtype)
    xs = [x.clone().requires_grad_(True) for x in x0]
    cls, reg = head(xs)
    torch.autograd.backward(cls + reg, gcl + grg)
    outs, dfeats, params, acts = _chain_by_hand(T, head, routes, x0, gcl, grg, dtype)
    for a, c in zip(list(cls) + list(reg) + [x.grad for x in xs] + [p.grad for p in head.parameters()],
                    outs + list(dfeats) + params):
        assert same_bits(a.contiguous(), c.contiguous())
    names = [n for n, _ in head.named_parameters()]
    grads = dict(zip(names, params))
    for ci, (tower, pred, pname, g) in enumerate(((head.cls_convs, head.retina_cls, "retina_cls", gcl),
                                                  (head.reg_convs, head.retina_reg, "retina_reg", grg))):
        tname = "cls_convs" if ci == 0 else "reg_convs"
        layers = [("%s.%d.conv" % (tname, i), m.conv, True) for i, m in enumerate(tower)] + [(pname, pred, False)]
        maps = [[nhwc(t) for t in level] for level in acts[ci]]
        g = [nhwc(t) for t in g]
        for i in reversed(range(len(layers))):
            lname, conv, relu = layers[i]
            w, b = R.round16(conv.weight, dtype), conv.bias.detach().float().cpu()
            for l, bd in enumerate(R.fwd_bounds(maps[i], w, b, relu)):
                R.within(nchw(maps[i + 1][l]), bd, dtype, "%s forward level %d" % (lname, l))
            R.within(grads[lname + ".weight"], R.wgrad_bound(maps[i], g), torch.float32, lname + " dw")
            R.within(grads[lname + ".bias"], R.dbias_bound(g), torch.float32, lname + " dbias")
            if i:
                # the next cotangent is the GPU's own: recompute it with the ops, then bound it
                layer = _ByHand(T, conv, routes["tower" if relu else ("cls" if ci == 0 else "reg")], relu, dtype)
                gn = layer.dgrad([nchw(t).to(dtype).cuda().contiguous(memory_format=CL) for t in g],
                                 mask_src=[nchw(t).to(dtype).cuda().contiguous(memory_format=CL) for t in maps[i]])
                for l, bd in enumerate(R.dgrad_bounds(g, w, maps[i])):
                    R.within(gn[l], bd, dtype, "%s dgrad level %d" % (lname, l))
                    assert (nhwc(gn[l])[maps[i][l] <= 0] == 0).all()
                g = [nhwc(t) for t in gn]


def test_packed_weights_follow_the_version_counter(T):
    from torch_detection_amd import heads
    head = _small_head(T)
    head._routes = {k: {p: "pyramid" for p in ("fwd", "dgrad", "wgrad")} for k in ("tower", "cls", "reg")}
    x = [torch.randn(1, 64, 4, 4).cuda().to(BF16).contiguous(memory_format=CL)]
    with torch.no_grad():
        y0 = head(x)[0][0].clone()
        u = head._pyr_unit("retina_cls", head.retina_cls.weight, BF16)
        assert isinstance(u, heads.PyrUnit)
        key, held = u.key, u.w_fwd
        head(x)
        assert u.key == key and u.w_fwd is held
        head.retina_cls.weight.mul_(2.0)
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
        head.retina_cls.weight.mul_(0.5)
        head.cls_convs[0].conv.weight.mul_(1.5)
        head.retina_cls.bias.add_(0.25)
        graph.replay()
        assert same_bits(yc, head(x)[0][0])


# ---- end to end -------------------------------------------------------------------------------------------------------------
STRIDES = (8, 16, 32)


def _problem(T, dtype=BF16):
    """Two 128 x 128 images, two ground truths each, a three-level pyramid of 64 channels."""
    import test_gpu_roi_align as RA
    gt = np.array([[[10, 20, 70, 90], [60, 8, 120, 60]], [[16, 16, 100, 80], [4, 40, 60, 124]]], np.float32)
    gt_labels = np.array([[1, 3], [2, 1]], np.int64)
    gt_counts = np.array([2, 2], np.int32)
    img_shapes = np.array([[128, 128], [128, 120]], np.int32)
    sizes = [(128 // s, 128 // s) for s in STRIDES]
    feats = [f.requires_grad_(True) for f in RA.feats_of(2, 64, sizes, dtype, 17, 0.5)]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return cuda(gt), cuda(gt_labels), cuda(gt_counts), cuda(img_shapes), sizes, feats


def _forward_backward(T, head, problem):
    gt, gt_labels, gt_counts, img_shapes, sizes, feats = problem
    cls, reg = head(feats)
    anchors, flags = head.get_anchors(sizes)
    losses = head.loss(cls, reg, anchors, flags, gt, gt_labels, gt_counts, img_shapes)
    grads = torch.autograd.grad(losses.sum(), list(head.parameters()) + feats)
    return list(cls) + list(reg) + [losses] + list(grads)


def _end_to_end(T, dtype=BF16):
    problem = _problem(T, dtype)
    head = _small_head(T, seed=7)
    opt = T.SGD(head.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, modules=[head])
    out = _forward_backward(T, head, problem)
    for p, gp in zip(head.parameters(), out[7:19]):
        p.grad = gp.clone()
    opt.step()
    torch.cuda.synchronize()
    return head, problem, out, [p.detach().clone() for p in head.parameters()]


def test_pyramid_retina_head_loss_backward_sgd_end_to_end(T):
    head, problem, out, params = _end_to_end(T)
    sizes = problem[4]
    cls, reg, losses = out[:3], out[3:6], out[6]
    for (H, W), c, r in zip(sizes, cls, reg):
        assert tuple(c.shape) == (2, 27, H, W) and tuple(r.shape) == (2, 36, H, W)
        assert c.permute(0, 2, 3, 1).is_contiguous() and r.permute(0, 2, 3, 1).is_contiguous()
    assert tuple(losses.shape) == (2,) and torch.isfinite(losses).all() and (losses > 0).all()
    for (name, p), gp in zip(head.named_parameters(), out[7:19]):
        assert gp.dtype == torch.float32 and gp.shape == p.shape, name
        assert torch.isfinite(gp).all() and gp.abs().sum().item() > 0, name
    for f, gf in zip(problem[5], out[19:]):
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
    # test time: get_bboxes takes the same outputs in place
    anchors, _ = head.get_anchors(sizes)
    with torch.no_grad():
        cls, reg = head([f.detach() for f in problem[5]])
        dets, labels, idx, counts = head.get_bboxes(cls, reg, anchors, problem[3], max_per_img=50)
    assert tuple(dets.shape) == (2, 50, 5) and tuple(labels.shape) == (2, 50) and tuple(idx.shape) == (2, 50)
    assert tuple(counts.shape) == (2,) and (counts > 0).all() and torch.isfinite(dets).all()
    assert dets.dtype == torch.float32 and labels.dtype == torch.int64 and counts.dtype == torch.int32
