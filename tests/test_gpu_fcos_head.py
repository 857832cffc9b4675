"""GPU: ``FCOSHead`` — the module against its own products called op by op, bit for bit; every launch of
the default and the composed routes within the a-priori bounds of the conv oracle (tests/pyramid_conv_ref.py) and the
GroupNorm criteria of tests/test_gpu_gn.py against a float64 ``nn.GroupNorm`` restatement, each fed the GPU's own stored
maps; ``norm_cfg=None``; a frozen affine; the packed weights and the version counter; and one tiny training step from
``fcos_target`` through the head and ``fcos_loss`` to ``SGD.step``, with ``get_bboxes`` on the same outputs."""
import types

import numpy as np
import pytest
import torch

import guard_util as G
import pyramid_conv_ref as R
import test_gpu_gn as GN
import test_gpu_pyramid_conv as PC
from test_gpu_pyramid_conv import BF16, CL, F16, nhwc, same_bits

pytestmark = pytest.mark.gpu

SIZES = [(9, 8), (5, 4), (3, 2)]
STRIDES = (8, 16, 32)
RANGES = ((-1, 32), (32, 64), (64, 1e8))                 # 128-pixel images: every level gets positives (_problem)
B, C, NCLS = 2, 64, 3


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


def _small_head(T, seed=3, **kw):
    torch.manual_seed(seed)
    args = dict(num_classes=NCLS + 1, in_channels=C, feat_channels=C, stacked_convs=2, strides=STRIDES,
                regress_ranges=RANGES, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True))
    args.update(kw)
    head = T.FCOSHead(**args).cuda()
    with torch.no_grad():                                   # weights large enough to matter, biases away from 0
        for name, p in head.named_parameters():
            if p.dim() == 4:
                p.mul_(6.0)
            elif name.endswith("norm.weight"):
                p.add_(torch.randn_like(p) * 0.1)
            elif p.dim() == 1:
                p.normal_(0, 0.1)
    return head


def _inputs(dtype, seed=11):
    g = torch.Generator().manual_seed(seed)
    mk = lambda ch: [torch.randn(B, ch, H, W, generator=g).cuda().to(dtype).contiguous(memory_format=CL) for H, W in SIZES]
    return mk(C), mk(NCLS), mk(4), mk(1)


class _Gn(object):
    """The GroupNorm + ReLU of a tower layer called op by op on the route named"""

    def __init__(self, norm, route):
        self.n, self.route = norm, route

    def fwd(self, zs):
        from torch_detection_amd import ops, pyramid_ops as P
        n = self.n
        if self.route == "pyramid":
            ys, st = P.pyramid_gn_fwd(zs, n.weight.detach(), n.bias.detach(), n.num_groups, n.eps, True)
            return ys, [st]
        out = [ops.gn_fwd(z.permute(0, 2, 3, 1), n.weight.detach(), n.bias.detach(), n.num_groups, n.eps, None, True)
               for z in zs]
        return [y.permute(0, 3, 1, 2) for y, _ in out], [s for _, s in out]

    def bwd(self, gs, ys, zs, stats):
        from torch_detection_amd import ops, pyramid_ops as P
        n = self.n
        if self.route == "pyramid":
            return P.pyramid_gn_bwd(gs, ys, zs, stats[0], n.weight.detach(), n.num_groups, True)
        dzs, dg, db = [], None, None
        for g, y, z, st in zip(gs, ys, zs, stats):
            gm = ops.act_mask(g.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1))
            dz, dg, db = ops.gn_bwd(gm, z.permute(0, 2, 3, 1), st, n.weight.detach(), n.num_groups, dg, db, dg is not None)
            dzs.append(dz.permute(0, 3, 1, 2))
        return dzs, dg, db


def _conv_by_hand(T, conv, routes, relu, dtype):
    """``_ByHand`` of the RetinaHead tests; a bias-free conv is handed a zero bias (x + 0.0 == x in fp32) and its bias
    gradient is dropped by the caller."""
    if conv.bias is None:
        conv = types.SimpleNamespace(weight=conv.weight, bias=torch.zeros(conv.weight.shape[0], device="cuda"))
    return PC._ByHand(T, conv, routes, relu, dtype)


def _chain_by_hand(T, head, routes, x0, gcl, grg, gct, dtype):
    """-> (outputs, dfeats, parameter gradients in ``head._params()`` order, the record of every product for the bounds)"""
    gn = head.norm_cfg is not None
    towers = []
    for convs in (head.cls_convs, head.reg_convs):
        towers.append([(_conv_by_hand(T, m.conv, routes["tower"], not gn, dtype),
                        _Gn(m.norm, routes["gn"]["fwd"]) if gn else None, m) for m in convs])
    preds = [_conv_by_hand(T, m, routes[k], False, dtype) for m, k in
             ((head.fcos_cls, "cls"), (head.fcos_reg, "reg"), (head.fcos_centerness, "ctr"))]
    acts, tops = [], []
    for tower in towers:
        cur, rows = x0, []
        for conv, g, _ in tower:
            zs = conv.fwd(cur)
            if g is None:
                rows.append((None, zs, None))
                cur = zs
            else:
                ys, stats = g.fwd(zs)
                rows.append((zs, ys, stats))
                cur = ys
        acts.append(rows)
        tops.append(cur)
    outs = preds[0].fwd(tops[0]) + preds[1].fwd(tops[1]) + preds[2].fwd(tops[0])
    rec, tower_grads, first = [], [], None
    pg = [preds[0].wgrad(tops[0], gcl), preds[1].wgrad(tops[1], grg), preds[2].wgrad(tops[0], gct)]
    for ti, (tower, rows) in enumerate(zip(towers, acts)):
        mask = tops[ti] if not gn else None
        if ti == 0:
            g1 = preds[0].dgrad(gcl, mask_src=mask)
            g = preds[2].dgrad(gct, mask_src=mask, addend=g1)
            rec.append(("pred", "fcos_cls", head.fcos_cls, tops[0], gcl, g1, mask, None))
            rec.append(("pred", "fcos_centerness", head.fcos_centerness, tops[0], gct, g, mask, g1))
        else:
            g = preds[1].dgrad(grg, mask_src=mask)
            rec.append(("pred", "fcos_reg", head.fcos_reg, tops[1], grg, g, mask, None))
        mine = []
        for i in reversed(range(len(tower))):
            conv, gnl, m = tower[i]
            zs, ys, stats = rows[i]
            x_in = rows[i - 1][1] if i else x0
            name = "%s.%d" % ("cls_convs" if ti == 0 else "reg_convs", i)
            aff = []
            if gnl is not None:
                g_in = g
                g, dgam, dbet = gnl.bwd(g, ys, zs, stats)
                aff = [dgam, dbet]
                rec.append(("gn", name, m.norm, zs, ys, g_in, g, dgam, dbet))
            dwb = conv.wgrad(x_in, g)
            if i:
                msk = x_in if not gn else None
                dx = conv.dgrad(g, mask_src=msk)
                add = None
            else:
                msk, add = None, first
                dx = conv.dgrad(g, addend=first)
            rec.append(("conv", name, m.conv, x_in, zs if gn else ys, g, dx, msk, add, dwb))
            mine.append([dwb[0]] + ([dwb[1]] if m.conv.bias is not None else []) + aff)
            g = dx
        first = g
        tower_grads.append(mine[::-1])
    params = [t for mine in tower_grads for grp in mine for t in grp] + [t for dwb in pg for t in dwb]
    rec += [("predw", n, c, tops[i], g_, dwb) for n, c, i, g_, dwb in (
        ("fcos_cls", head.fcos_cls, 0, gcl, pg[0]), ("fcos_reg", head.fcos_reg, 1, grg, pg[1]),
        ("fcos_centerness", head.fcos_centerness, 0, gct, pg[2]))]
    return outs, first, params, rec


def _run_head(head, x0, gcl, grg, gct):
    xs = [x.clone().requires_grad_(True) for x in x0]
    cls, reg, ctr = head(xs)
    torch.autograd.backward(cls + reg + ctr, gcl + grg + gct)
    return xs, cls, reg, ctr


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_fcos_head_is_its_default_route_called_op_by_op(T, guard, dtype):
    from torch_detection_amd import heads
    head = _small_head(T)
    assert head._routes is heads.FCOS_ROUTES
    x0, gcl, grg, gct = _inputs(dtype)
    grg[2] = grg[2].float().contiguous()                                 # an NCHW float32 cotangent: one copy
    xs = [x.clone().requires_grad_(True) for x in x0]
    xs[1] = x0[1].float().contiguous().requires_grad_(True)              # one level as float32 NCHW
    if dtype == F16:
        head.compute_dtype = F16
    cls, reg, ctr = head(xs)
    for (H, W), c, r, t in zip(SIZES, cls, reg, ctr):
        assert tuple(c.shape) == (B, NCLS, H, W) and tuple(r.shape) == (B, 4, H, W) and tuple(t.shape) == (B, 1, H, W)
        assert c.dtype == r.dtype == t.dtype == dtype
        assert all(v.permute(0, 2, 3, 1).is_contiguous() for v in (c, r, t))
    assert all(t.grad_fn is cls[0].grad_fn for t in cls + reg + ctr)     # one autograd node
    torch.autograd.backward(cls + reg + ctr, gcl + grg + gct)
    assert xs[0].grad.is_contiguous(memory_format=CL) and xs[0].grad.dtype == dtype
    assert xs[1].grad.is_contiguous() and xs[1].grad.dtype == torch.float32
    for p in head._params():
        assert p.grad.shape == p.shape and p.grad.dtype == torch.float32
    assert all(s.scale.grad is None for s in head.scales)                # the scales are fcos_loss's business
    got = [t.detach() for t in cls + reg + ctr] + [x.grad for x in xs] + [p.grad for p in head._params()]
    grg[2] = grg[2].to(dtype).contiguous(memory_format=CL)
    outs, dfeats, params, _ = _chain_by_hand(T, head, heads.FCOS_ROUTES, x0, gcl, grg, gct, dtype)
    dfeats = list(dfeats)
    dfeats[1] = dfeats[1].float().contiguous()
    want = outs + dfeats + params
    assert len(got) == len(want) == 9 + 3 + 18
    for i, (a, c) in enumerate(zip(got, want)):
        assert same_bits(a.contiguous(), c.contiguous()), "output %d of the head differs from the chain" % i
    found = guard.check()
    assert not found, "\n".join(found)
    assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log


def _f64(t):
    return t.detach().double().cpu()


def _check_gn(norm, zs, ys, g_in, dzs, dgam, dbet, dtype, tag):
    """One GroupNorm + ReLU product against float64 nn.GroupNorm on the GPU's own stored z and cotangent; the ReLU mask
    is the stored y's, as the backward is specified."""
    ulp = GN.ULP[dtype]
    ref = torch.nn.GroupNorm(norm.num_groups, norm.num_channels, norm.eps).double()
    with torch.no_grad():
        ref.weight.copy_(_f64(norm.weight))
        ref.bias.copy_(_f64(norm.bias))
    zr = [_f64(z).contiguous().requires_grad_(True) for z in zs]
    pre = [ref(z) for z in zr]
    gm = [_f64(g) * (_f64(y) > 0) for g, y in zip(g_in, ys)]
    torch.autograd.backward(pre, gm)
    Gr, cpg = norm.num_groups, norm.num_channels // norm.num_groups
    for l, (z, y) in enumerate(zip(zr, ys)):
        GN._check_y(_f64(y).numpy(), torch.relu(pre[l]).detach().numpy(), ulp, "%s y level %d" % (tag, l))
        den = float(z.grad.abs().max())
        mr = float((_f64(dzs[l]) - z.grad).abs().max()) / (den if den > 0 else 1.0)
        assert mr <= 2 * ulp, "%s dz level %d: %.3g" % (tag, l, mr)
    flat = lambda ts: np.concatenate([t.detach().numpy().reshape(t.shape[0], t.shape[1], -1, 1) for t in ts], axis=2)
    xhat = [torch.from_numpy(GN.R.gn_xhat(z.detach().numpy(), Gr, norm.eps)) for z in zr]
    GN._check_bwd(flat([_f64(d) for d in dzs]), _f64(dgam).numpy(), _f64(dbet).numpy(),
                  (flat([z.grad for z in zr]), ref.weight.grad.numpy(), ref.bias.grad.numpy()), flat(gm), flat(xhat), ulp, tag)


@pytest.mark.parametrize("route", ["default", "composed"])
def test_fcos_head_routes_stay_within_the_oracle_bounds(T, route):
    """Every launch of the head within its bound, fed the GPU's own stored maps: the convs within the a-priori bounds of
    the fp64 conv oracle on the 16-bit-rounded weights, the GroupNorms within the criteria of the single-map kernels
    against float64 ``nn.GroupNorm``; and the module equals the chain bit for bit on this route too."""
    from torch_detection_amd import heads
    dtype = BF16
    routes = heads.FCOS_ROUTES if route == "default" else heads.FCOS_COMPOSED
    head = _small_head(T)
    head._routes = routes
    x0, gcl, grg, gct = _inputs(dtype)
    xs, cls, reg, ctr = _run_head(head, x0, gcl, grg, gct)
    outs, dfeats, params, rec = _chain_by_hand(T, head, routes, x0, gcl, grg, gct, dtype)
    for a, c in zip(list(cls) + list(reg) + list(ctr) + [x.grad for x in xs] + [p.grad for p in head._params()],
                    outs + list(dfeats) + params):
        assert same_bits(a.contiguous(), c.contiguous())
    h = lambda ts: None if ts is None else [nhwc(t) for t in ts]
    seen = 0
    for r in rec:
        if r[0] == "gn":
            _, name, norm, zs, ys, g_in, dzs, dgam, dbet = r
            _check_gn(norm, zs, ys, g_in, dzs, dgam, dbet, dtype, name + ".norm")
        elif r[0] == "conv":
            _, name, conv, x_in, out, g, dx, msk, add, dwb = r
            w = R.round16(conv.weight, dtype)
            for l, bd in enumerate(R.fwd_bounds(h(x_in), w, None, False)):
                R.within(out[l], bd, dtype, "%s forward level %d" % (name, l))
            for l, bd in enumerate(R.dgrad_bounds(h(g), w, h(msk), h(add))):
                R.within(dx[l], bd, dtype, "%s dgrad level %d" % (name, l))
            R.within(dwb[0], R.wgrad_bound(h(x_in), h(g)), torch.float32, name + " dw")
        elif r[0] == "pred":
            _, name, conv, x_in, g, dx, msk, add = r
            w = R.round16(conv.weight, dtype)
            for l, bd in enumerate(R.dgrad_bounds(h(g), w, h(msk), h(add))):
                R.within(dx[l], bd, dtype, "%s dgrad level %d" % (name, l))
        else:
            _, name, conv, x_in, g, dwb = r
            R.within(dwb[0], R.wgrad_bound(h(x_in), h(g)), torch.float32, name + " dw")
            R.within(dwb[1], R.dbias_bound(h(g)), torch.float32, name + " dbias")
        seen += 1
    assert seen == 4 + 4 + 3 + 3
    # the predictors' forwards
    n = len(SIZES)
    tops = {"fcos_cls": rec[0][3], "fcos_centerness": rec[1][3], "fcos_reg": [r for r in rec if r[1] == "fcos_reg"][0][3]}
    for name, conv, got in (("fcos_cls", head.fcos_cls, outs[:n]), ("fcos_reg", head.fcos_reg, outs[n:2 * n]),
                            ("fcos_centerness", head.fcos_centerness, outs[2 * n:])):
        w, b = R.round16(conv.weight, dtype), conv.bias.detach().float().cpu()
        for l, bd in enumerate(R.fwd_bounds(h(tops[name]), w, b, False)):
            R.within(got[l], bd, dtype, "%s forward level %d" % (name, l))


def test_fcos_head_without_norm_cfg(T):
    from torch_detection_amd import heads
    dtype = BF16
    head = _small_head(T, norm_cfg=None)
    assert [n for n, _ in head.named_parameters()][:2] == ["cls_convs.0.conv.weight", "cls_convs.0.conv.bias"]
    x0, gcl, grg, gct = _inputs(dtype)
    xs, cls, reg, ctr = _run_head(head, x0, gcl, grg, gct)
    outs, dfeats, params, _ = _chain_by_hand(T, head, heads.FCOS_ROUTES, x0, gcl, grg, gct, dtype)
    got = list(cls) + list(reg) + list(ctr) + [x.grad for x in xs] + [p.grad for p in head._params()]
    assert len(got) == 9 + 3 + 14
    for i, (a, c) in enumerate(zip(got, outs + list(dfeats) + params)):
        assert same_bits(a.contiguous(), c.contiguous()), i
    for (n_, p) in head.named_parameters():
        if not n_.startswith("scales"):
            assert torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, n_


def test_frozen_gn_affine_gets_no_gradient(T):
    dtype = BF16
    head = _small_head(T, norm_cfg=dict(type='GN', num_groups=32, requires_grad=False))
    x0, gcl, grg, gct = _inputs(dtype)
    xs, cls, reg, ctr = _run_head(head, x0, gcl, grg, gct)
    free = _small_head(T)
    xs2, cls2, _, _ = _run_head(free, x0, gcl, grg, gct)
    for (n_, p), (_, q) in zip(head.named_parameters(), free.named_parameters()):
        if ".norm." in n_:
            assert p.grad is None and not p.requires_grad and q.grad is not None, n_
        elif not n_.startswith("scales"):
            assert same_bits(p.grad, q.grad), n_                          # freezing changes nothing else
    assert all(same_bits(a.grad, c.grad) for a, c in zip(xs, xs2)) and same_bits(cls[0], cls2[0])


def test_packed_weights_follow_the_version_counter(T):
    from torch_detection_amd import heads
    head = _small_head(T)
    x = [torch.randn(1, 64, 4, 4).cuda().to(BF16).contiguous(memory_format=CL)]
    with torch.no_grad():
        y0 = head(x)[0][0].clone()
        u = head._pyr_unit("fcos_cls", head.fcos_cls.weight, BF16)
        assert isinstance(u, heads.PyrUnit)
        key, held = u.key, u.w_fwd
        head(x)
        assert u.key == key and u.w_fwd is held
        head.fcos_cls.weight.mul_(2.0)
        y1 = head(x)[0][0].clone()
        assert u.key != key and u.w_fwd is held and not same_bits(y0, y1)          # repacked in place
        T.invalidate_packed(head)
        assert u.key is None
        # inside a capture the pack is enqueued again, and gamma / beta are read at launch time
        head(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            yc = head(x)[0][0]
        head.fcos_cls.weight.mul_(0.5)
        head.cls_convs[0].conv.weight.mul_(1.5)
        head.cls_convs[1].norm.weight.mul_(1.25)
        head.cls_convs[0].norm.bias.add_(0.25)
        graph.replay()
        assert same_bits(yc, head(x)[0][0])


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _problem(T, dtype=BF16):
    """Two 128 x 128 images, three ground truths each — small, medium and large against RANGES, so that every level
    has positive points (8 + 6, 18 + 22 and 0 + 5 by the assignment rule) —, a three-level pyramid of 64 channels."""
    import test_gpu_roi_align as RA
    gt = np.array([[[10, 20, 70, 90], [60, 8, 120, 60], [30, 30, 50, 54]],
                   [[16, 16, 100, 80], [4, 40, 60, 124], [70, 90, 90, 110]]], np.float32)
    gt_labels = np.array([[1, 3, 2], [2, 1, 3]], np.int64)
    gt_counts = np.array([3, 3], np.int32)
    img_shapes = np.array([[128, 128], [128, 120]], np.int32)
    sizes = [(128 // s, 128 // s) for s in STRIDES]
    feats = [f.requires_grad_(True) for f in RA.feats_of(2, 64, sizes, dtype, 17, 0.5)]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return cuda(gt), cuda(gt_labels), cuda(gt_counts), cuda(img_shapes), sizes, feats


def _end_to_end(T, dtype=BF16):
    gt, gt_labels, gt_counts, img_shapes, sizes, feats = _problem(T, dtype)
    head = _small_head(T, seed=7)
    with torch.no_grad():
        for l, s in enumerate(head.scales):
            s.scale.fill_(1.0 + 0.25 * l)
    opt = T.SGD(head.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, modules=[head])
    cls, reg, ctr = head(feats)
    losses = head.loss(cls, reg, ctr, gt, gt_labels, gt_counts)
    plist = list(head.parameters())
    grads = torch.autograd.grad(losses.sum(), plist + feats)
    for p, gp in zip(plist, grads):
        p.grad = gp.clone()
    before = [p.detach().clone() for p in plist]
    opt.step()
    torch.cuda.synchronize()
    out = list(cls) + list(reg) + list(ctr) + [losses] + list(grads)
    return head, (img_shapes, sizes, feats), out, before, [p.detach().clone() for p in plist]


def test_fcos_target_head_loss_backward_sgd_end_to_end(T):
    head, (img_shapes, sizes, feats), out, before, after = _end_to_end(T)
    n = len(sizes)
    cls, reg, ctr, losses = out[:n], out[n:2 * n], out[2 * n:3 * n], out[3 * n]
    for (H, W), c, r, t in zip(sizes, cls, reg, ctr):
        assert tuple(c.shape) == (2, NCLS, H, W) and tuple(r.shape) == (2, 4, H, W) and tuple(t.shape) == (2, 1, H, W)
    assert losses.dim() == 1 and torch.isfinite(losses).all() and (losses > 0).all()
    names = [n_ for n_, _ in head.named_parameters()]
    grads = out[3 * n + 1:]
    assert len(names) == 21 and names[-3:] == ["scales.0.scale", "scales.1.scale", "scales.2.scale"]
    for name, p, gp in zip(names, head.parameters(), grads):
        assert gp.dtype == torch.float32 and gp.shape == p.shape, name
        assert torch.isfinite(gp).all() and gp.abs().sum().item() > 0, name
    for f, gf in zip(feats, grads[len(names):]):
        assert gf.shape == f.shape and gf.dtype == f.dtype and gf.is_contiguous(memory_format=CL)
        assert torch.isfinite(gf.float()).all() and gf.float().abs().sum().item() > 0
    assert all(not torch.equal(a, c) for a, c in zip(before, after))     # the step moved every parameter
    # a second identical run: identical bits
    _, _, again, _, after2 = _end_to_end(T)
    for a, c in zip(out + after, again + after2):
        assert same_bits(a, c)
    # detections on the same outputs
    with torch.no_grad():
        dets, labels, point_idx, counts = head.get_bboxes(cls, reg, ctr, img_shapes, max_per_img=20)
    assert tuple(dets.shape) == (2, 20, 5) and dets.dtype == torch.float32
    assert tuple(labels.shape) == (2, 20) and labels.dtype == torch.int64
    assert tuple(point_idx.shape) == (2, 20) and tuple(counts.shape) == (2,) and counts.dtype == torch.int32
    assert tuple(head.get_points(sizes).shape) == (sum(H * W for H, W in sizes), 4)
