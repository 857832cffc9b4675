"""GPU tests of the gradient-harmonised losses (ghm_head_loss / GHMC / GHMR, csrc/ghm.hip) against the CPU oracle
tests/ghm_ref.py: small shapes over every layout and dtype, a level of many workgroups, unaligned heads,
the boundary inputs of every bin edge, NaN / Inf / poison, both scopes, the extreme bin counts, graph replay, every entry
point of ghm_ops.py under guard-banded, poisoned outputs with exact-size workspaces (tests/guard_util.py), and the chain
through RetinaHead.

What is compared as bit patterns: the whole table (beta, the counts, tot, the number of non-empty bins, the number of
valid elements in no bin), the running averages, both gradients (16-bit: the oracle's float32 value rounded to nearest
even).  loss_bbox is the fp64 sum of float32 summands that equal the oracle's bit for bit, in another order: the sums
differ by at most n 2^-53 relative, so the float32 results agree to half a spacing (+ that); with one summand per row
they are the same bits.  loss_cls goes through the device's log1pf: |got - ref64| <= K u mag + spacing(ref), K = 8."""
import inspect

import numpy as np
import pytest
import torch

import ghm_cases as GC
import ghm_ref as R
import guard_util as G

pytestmark = pytest.mark.gpu

f32 = np.float32
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CFG = dict(num_classes=None, bins_cls=30, bins_reg=10, momentum_cls=0.75, momentum_reg=0.7, mu=0.02, scope="level")
ENTERED, WS_SEEN = set(), {}        # what ran under the guard in this run (checked by the last test of the file)


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _layout(t, nhwc):
    return t.contiguous(memory_format=torch.channels_last) if nhwc else t.contiguous()


def put(case, dtype, layout):
    """numpy case -> (the case as the storage type holds it, float32 numpy; the CUDA heads; the CUDA targets)."""
    cls, reg = [], []
    for l, (c, r) in enumerate(zip(case[0], case[1])):
        nhwc = {"nchw": (False, False), "nhwc": (True, True), "mixed": (l % 2 == 0, l % 2 == 1)}[layout]
        cls.append(_layout(torch.from_numpy(c).to(dtype).cuda(), nhwc[0]))
        reg.append(_layout(torch.from_numpy(r).to(dtype).cuda(), nhwc[1]))
    stored = ([t.float().cpu().numpy() for t in cls], [t.float().cpu().numpy() for t in reg]) + tuple(case[2:])
    return stored, cls + reg, [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in case[2:]]


def _same_bits(got, want32, dtype, what):
    """got (CUDA, dtype) == the float32 oracle value rounded to nearest even into dtype; NaNs wherever the oracle has them"""
    want = torch.from_numpy(np.ascontiguousarray(want32)).to(dtype)
    got = got.detach().cpu()
    assert got.shape == want.shape, what
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what + ": NaN pattern differs"
    bad = (_bits(got) != _bits(want)) & ~nan.contiguous()
    assert not bad.any(), "%s: bits differ at %d of %d" % (what, int(bad.sum()), bad.numel())


def check(ref, losses, table, dcls, dreg, dtype, what):
    """Everything one forward + backward returned against the oracle's ``ref``."""
    tab = table.cpu().numpy()
    want = R.table(ref)
    assert np.array_equal(tab.view(np.uint32), want.view(np.uint32)), "%s: table differs at %s" % (
        what, np.argwhere(tab.view(np.uint32) != want.view(np.uint32))[:5].tolist())
    got = losses.detach().cpu().numpy().astype(np.float64)
    for k in range(2):
        r64 = ref["losses64"][k]
        if np.isnan(r64):
            assert np.isnan(got[k]), what
            continue
        sp = float(np.spacing(f32(abs(r64))))
        tol = R.K * R.U * ref["mag"][0] + sp if k == 0 else 0.5 * sp * (1 + 2.0 ** -20)
        print("%s: loss %d got %r ref %r error %.3g (allowed %.3g)" % (what, k, got[k], r64, abs(got[k] - r64), tol))
        assert abs(got[k] - r64) <= tol, (what, k, got[k], r64, tol)
    for l in range(len(dcls)):
        _same_bits(dcls[l], ref["dcls"][l], dtype, "%s: dcls[%d]" % (what, l))
        _same_bits(dreg[l], ref["dreg"][l], dtype, "%s: dreg[%d]" % (what, l))


def raw(heads, targets, acc, g, cfg):
    """One forward + backward through ghm_ops.py -> (losses, table, dcls, dreg); the gradients keep the heads' strides."""
    from torch_detection_amd import ghm_ops
    L = len(heads) // 2
    order = ("num_classes", "bins_cls", "bins_reg", "momentum_cls", "momentum_reg", "mu", "scope")
    meta = [cfg[k] for k in order]
    losses, table = ghm_ops.ghm_head_loss_fwd(heads[:L], heads[L:], *targets, acc[0], acc[1], *meta)
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    dcls, dreg = ghm_ops.ghm_head_loss_bwd(heads[:L], heads[L:], *targets, gt, table, *meta)
    for d, h in zip(dcls + dreg, heads):
        assert d.shape == h.shape and d.dtype == h.dtype and d.stride() == h.stride()
    return losses, table, dcls, dreg


def steps(case_of, dtype, layout, cfg, g, what, n=3):
    """n successive calls on new inputs with the running averages carried over, each against the oracle; then acc."""
    acc = [torch.zeros(cfg["bins_cls"], device="cuda") if cfg["momentum_cls"] > 0 else None,
           torch.zeros(cfg["bins_reg"], device="cuda") if cfg["momentum_reg"] > 0 else None]
    acc_ref = [None if a is None else np.zeros(a.numel(), f32) for a in acc]
    for step in range(n):
        stored, heads, targets = put(case_of(step), dtype, layout)
        out = raw(heads, targets, acc, g, cfg)
        ref = R.ghm_head_loss(*stored, acc_ref[0], acc_ref[1], g=g, **cfg)
        check(ref, *out, dtype, "%s step %d" % (what, step))
    for a, r in zip(acc, acc_ref):
        if a is not None:
            assert np.array_equal(a.cpu().numpy().view(np.uint32), r.view(np.uint32)), what + ": acc"
    return ref


# ---- small shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "mixed"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("A,C", [(3, 1), (2, 5), (9, 20)])
def test_small_vs_oracle(T, A, C, B, dt, layout):
    """Five levels 13 x 17 .. 1 x 1 (the last leaves most bins empty: the n_r path), NaN / Inf / poison under every zero
    weight; three calls with momentum, then one with momentum 0 and acc=None (the counts are the table's)."""
    g = (768.0, 320.0) if dt == "f16" else (1.5, 0.75)
    cfg = dict(CFG, num_classes=C)
    ref = steps(lambda s: GC.case(B, A, C, GC.LEVELS, 1000 * A + 10 * B + s), DTYPES[dt], layout, cfg, g,
                "A%d C%d B%d %s %s" % (A, C, B, dt, layout))
    assert (ref["n"] < np.array([[30], [10]])).any() and ref["cnt"][0].sum() > 0 and ref["cnt"][1].sum() > 0
    cfg0 = dict(cfg, momentum_cls=0.0, momentum_reg=0.0)
    steps(lambda s: GC.case(B, A, C, GC.LEVELS, 77 + A), DTYPES[dt], layout, cfg0, g, "momentum 0", n=1)


@pytest.mark.parametrize("dt,B,layout", [("f32", 1, "nchw"), ("bf16", 2, "nhwc")])
def test_many_workgroups(T, dt, B, layout):
    """One 64 x 100 level, A = 9, C = 20: 288 000 chunks, the full 256 workgroups and more than one grid pass."""
    cfg = dict(CFG, num_classes=20)
    steps(lambda s: GC.case(B, 9, 20, [(64, 100)], 5 + s, valid=0.5), DTYPES[dt], layout, cfg, (1.0, 1.0),
          "64x100 %s" % dt, n=1)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_heads_four_bytes_off_alignment(T, dt):
    dtype = DTYPES[dt]
    cfg = dict(CFG, num_classes=5)
    stored, heads, targets = put(GC.case(2, 2, 5, GC.LEVELS[:3], 31), dtype, "mixed")
    skew = 4 // heads[0].element_size()
    off = []
    for h in heads:
        flat = torch.empty(h.numel() + 16, dtype=dtype, device="cuda")
        v = flat[skew:skew + h.numel()].as_strided(tuple(h.shape), tuple(h.stride()))
        v.copy_(h)
        assert v.data_ptr() % 16 == 4 and v.stride() == h.stride()
        off.append(v)
    acc = [torch.zeros(30, device="cuda"), torch.zeros(10, device="cuda")]
    acc_ref = [np.zeros(30, f32), np.zeros(10, f32)]
    out = raw(off, targets, acc, (1.5, 0.75), cfg)
    check(R.ghm_head_loss(*stored, *acc_ref, g=(1.5, 0.75), **cfg), *out, dtype, "unaligned " + dt)


# ---- the bin edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_both_sides_of_every_edge_land_in_the_oracles_bins(T, dt):
    """Every interior edge of bins = 30 (GHM-C, both targets) and bins = 10 (GHM-R, both signs): the two adjacent
    representable inputs between which the oracle's bin changes (bisection, tests/ghm_cases.py); x = 0 (bin bins / 2) and
    g = 1.0 exactly (|d| = 8192 >> mu: the last bin).  The counts of the table show every element's bin."""
    dtype = DTYPES[dt]
    x0, x1 = GC.cls_crossings(30, dt, False).ravel(), GC.cls_crossings(30, dt, True).ravel()
    x = np.concatenate([x0, [0.0], x1, [0.0, -0.0]]).astype(f32)
    n = x.size
    labels = np.concatenate([np.zeros(x0.size + 1), np.ones(x1.size + 2)]).astype(np.int64)[None]
    d = np.concatenate([GC.reg_crossings(10, dt, 0.02, 1).ravel(), GC.reg_crossings(10, dt, 0.02, -1).ravel(),
                        [8192.0, -8192.0, 0.0]]).astype(f32)
    reg = np.zeros(4 * n, f32)
    reg[:d.size] = d
    bw = np.zeros(4 * n, f32)
    bw[:d.size] = 1
    case = ([x.reshape(1, 1, 1, n)], [reg.reshape(n, 4).T.reshape(1, 4, 1, n).copy()], labels, np.ones((1, n), f32),
            np.zeros((1, n, 4), f32), bw.reshape(1, n, 4))
    cfg = dict(CFG, num_classes=1, momentum_cls=0.0, momentum_reg=0.0)
    stored, heads, targets = put(case, dtype, "nchw")
    assert np.array_equal(stored[0][0].view(np.uint32), case[0][0].view(np.uint32))       # the inputs are representable
    out = raw(heads, targets, [None, None], (1.0, 1.0), cfg)
    ref = R.ghm_head_loss(*stored, None, None, g=(1.0, 1.0), **cfg)
    want_c = np.full(30, 4)                                  # per target and edge one input on either side
    want_c[[0, 29]] = 2
    want_c[15] += 3                                          # the three zeros
    want_r = np.full(10, 4)
    want_r[[0, 9]] = 2
    want_r[0] += 1                                           # d = 0
    want_r[9] += 2                                           # g = 1.0
    assert np.array_equal(ref["cnt"][0, 0, :30], want_c) and np.array_equal(ref["cnt"][1, 0, :10], want_r)
    check(ref, *out, dtype, "edges " + dt)


# ---- NaN, scopes, bin counts ---------------------------------------------------------------------------------------------
def test_nan_under_a_positive_weight_spreads_and_counts(T):
    case = GC.case(2, 2, 5, GC.LEVELS[:3], 41)
    cfg = dict(CFG, num_classes=5)
    A, C = 2, 5
    n = int(np.flatnonzero(case[3][0] > 0)[3])               # a valid anchor of image 0 on level 0
    h, w = GC.LEVELS[0]
    p, a = divmod(n, A)
    case[0][0][0, a * C + 1, p // w, p % w] = np.nan
    m = int(np.flatnonzero(case[5][0, :h * w * A, 0] > 0)[0])
    p, a = divmod(m, A)
    case[1][0][0, a * 4 + 0, p // w, p % w] = np.nan
    stored, heads, targets = put(case, torch.float32, "mixed")
    acc = [torch.zeros(30, device="cuda"), torch.zeros(10, device="cuda")]
    out = raw(heads, targets, acc, (1.0, 1.0), cfg)
    ref = R.ghm_head_loss(*stored, np.zeros(30, f32), np.zeros(10, f32), **cfg)
    assert ref["nan"][0, 0] == 1 and ref["nan"][1, 0] == 1 and np.isnan(ref["losses64"]).all()
    check(ref, *out, torch.float32, "NaN under weight > 0")
    assert torch.isnan(out[0]).all() and torch.isfinite(acc[0]).all() and torch.isfinite(acc[1]).all()


def test_all_weights_zero(T):
    case = list(GC.case(1, 2, 5, GC.LEVELS[2:], 43))
    case[3] = np.zeros_like(case[3])
    case[5] = np.zeros_like(case[5])
    for c in case[0] + case[1]:
        c[...] = np.nan
    stored, heads, targets = put(case, torch.bfloat16, "nhwc")
    acc = [torch.full((30,), 3.0, device="cuda"), torch.full((10,), 2.0, device="cuda")]
    losses, table, dcls, dreg = raw(heads, targets, acc, (1.0, 1.0), dict(CFG, num_classes=5))
    assert losses.tolist() == [0.0, 0.0] and table[:, :, 128].eq(1).all() and table[:, :, :128].eq(0).all()
    assert all(not d.float().abs().sum().item() for d in dcls + dreg)
    assert acc[0].eq(3).all() and acc[1].eq(2).all()         # every bin is empty: acc is untouched


@pytest.mark.parametrize("scope", ["level", "batch"])
@pytest.mark.parametrize("bins", [1, 30, 64])
def test_scopes_and_extreme_bin_counts(T, scope, bins):
    cfg = dict(CFG, num_classes=5, bins_cls=bins, bins_reg=64 if bins == 64 else min(bins, 10), scope=scope)
    ref = steps(lambda s: GC.case(3, 2, 5, GC.LEVELS, 50 + s, bins_cls=bins, bins_reg=cfg["bins_reg"]), torch.bfloat16,
                "mixed", cfg, (1.5, 0.75), "%s bins %d" % (scope, bins))
    assert ref["tot"].shape == (2, 1 if scope == "batch" else 5)


def test_one_summand_per_row_gives_the_oracles_bits(T):
    """One valid box element per level: every row's fp64 sum is its one float32 summand, so loss_bbox has the oracle's bits."""
    case = list(GC.case(1, 2, 5, GC.LEVELS, 61, poison=False))
    bw = np.zeros_like(case[5])
    n0 = 0
    for h, w in GC.LEVELS:
        bw[0, n0 + (h * w * 2) // 2, 1] = 1
        n0 += h * w * 2
    case[5] = bw
    cfg = dict(CFG, num_classes=5, momentum_reg=0.0)
    stored, heads, targets = put(case, torch.float32, "nchw")
    losses = raw(heads, targets, [torch.zeros(30, device="cuda"), None], (1.0, 1.0), cfg)[0]
    ref = R.ghm_head_loss(*stored, np.zeros(30, f32), None, **cfg)
    terms = [float(t.astype(np.float64).sum()) for t in ref["terms_reg"]]
    assert all(np.count_nonzero(t) == 1 for t in ref["terms_reg"])
    total = 0.0
    for t in terms:
        total += t / 1.0
    assert f32(total).view(np.uint32) == losses.cpu().numpy()[1].view(np.uint32)


# ---- the public function, eager and replayed -------------------------------------------------------------------------
def test_autograd_function_run_to_run_and_graph_replay(T):
    """ghm_head_loss through autograd: two runs from the same state agree bit for bit; forward + backward captured once
    and replayed three times on new logits and targets agrees with eager, with the oracle, and leaves the oracle's acc:
    a host synchronisation or an allocation inside the library would break the capture."""
    cfg = dict(CFG, num_classes=5)
    kw = {k: v for k, v in cfg.items() if k != "num_classes"}
    new = lambda seed: put(GC.case(2, 2, 5, GC.LEVELS, seed), torch.bfloat16, "nhwc")
    stored, heads, targets = new(70)
    heads = [h.requires_grad_(True) for h in heads]
    acc = [torch.zeros(30, device="cuda"), torch.zeros(10, device="cuda")]
    cot = torch.tensor([1.5, 0.75], device="cuda")

    def step(acc):
        losses = T.ghm_head_loss(heads[:5], heads[5:], *targets, acc[0], acc[1], 5, **kw)
        return [losses] + list(torch.autograd.grad(losses, heads, cot))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = step([a.clone() for a in acc])
        again = step([a.clone() for a in acc])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(_bits(a), _bits(b))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(acc)
    acc_ref = [np.zeros(30, f32), np.zeros(10, f32)]
    seen = []
    for seed in (71, 72, 73):
        stored, h2, t2 = new(seed)
        with torch.no_grad():
            for dst, src in zip(heads + targets, h2 + t2):
                dst.copy_(src)
        before = [a.clone() for a in acc]
        graph.replay()
        eager = step(before)
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(_bits(a), _bits(b))
        ref = R.ghm_head_loss(*stored, *acc_ref, g=(1.5, 0.75), **cfg)
        for l in range(5):
            _same_bits(captured[1 + l], ref["dcls"][l], torch.bfloat16, "replay dcls[%d]" % l)
            _same_bits(captured[6 + l], ref["dreg"][l], torch.bfloat16, "replay dreg[%d]" % l)
        for a, b, r in zip(acc, before, acc_ref):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), r.view(np.uint32))
            assert torch.equal(a, b)
        seen.append(captured[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- under the guard ---------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import ghm_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, ghm_ops, g)
    yield g
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt,layout", [("f32", "mixed"), ("bf16", "nhwc"), ("f16", "nchw")])
def test_guarded(T, guard, dt, layout):
    g = (768.0, 320.0) if dt == "f16" else (1.5, 0.75)
    for B, A, C, scope in ((3, 9, 20, "level"), (1, 3, 1, "batch")):
        cfg = dict(CFG, num_classes=C, scope=scope)
        stored, heads, targets = put(GC.case(B, A, C, GC.LEVELS, 80 + A), DTYPES[dt], layout)
        acc = [torch.zeros(30, device="cuda"), torch.zeros(10, device="cuda")]
        out = raw(heads, targets, acc, g, cfg)
        log = list(guard.ws_log)
        found = guard.check()
        assert not found, "\n".join(found)
        check(R.ghm_head_loss(*stored, np.zeros(30, f32), np.zeros(10, f32), g=g, **cfg), *out, DTYPES[dt],
              "guarded %s %s" % (dt, layout))
        ENTERED.update(["ghm_head_loss_fwd", "ghm_head_loss_bwd"])
        for op, asked, given in log:
            WS_SEEN.setdefault(op, (asked, given))


def test_every_ghm_entry_point_ran_under_the_guard():
    """Counts what the guarded tests above did IN THIS RUN (run the file as a whole): every public wrapper of ghm_ops.py
    returned under the guard, and the workspace query was answered at its exact size (rounded up only to the 256-byte
    alignment the header asks for)."""
    from torch_detection_amd import ghm_ops
    public = sorted(n for n, v in vars(ghm_ops).items()
                    if inspect.isfunction(v) and v.__module__ == ghm_ops.__name__ and not n.startswith("_"))
    assert public == ["ghm_head_loss_bwd", "ghm_head_loss_fwd"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    asked, given = WS_SEEN["ghm_head_loss_fwd"]
    assert 0 <= given - asked < 256 and asked > 0, (asked, given)


# ---- RetinaHead ----------------------------------------------------------------------------------------------------------
def _retina(T, **kw):
    torch.manual_seed(7)
    head = T.RetinaHead(num_classes=5, in_channels=64, feat_channels=64, stacked_convs=2, anchor_strides=(8, 16),
                        **kw).cuda()
    with torch.no_grad():                                   # weights large enough to matter, biases away from 0
        for p in head.parameters():
            if p.dim() == 4:
                p.mul_(6.0)
            else:
                p.normal_(0, 0.1)
    return head


def _problem():
    g = torch.Generator().manual_seed(17)
    sizes = [(8, 8), (4, 4)]
    feats = [(torch.randn(2, 64, h, w, generator=g) * 0.5).to(torch.bfloat16).cuda().contiguous(
        memory_format=torch.channels_last).requires_grad_(True) for h, w in sizes]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    gt = np.array([[[4, 8, 40, 50], [30, 4, 60, 30]], [[8, 8, 50, 40], [2, 20, 30, 62]]], f32)
    return (sizes, feats, cuda(gt), cuda(np.array([[1, 3], [2, 4]], np.int64)), cuda(np.array([2, 2], np.int32)),
            cuda(np.array([[64, 64], [64, 60]], np.int32)))


def test_retina_head_with_ghm_losses_forward_loss_backward(T):
    sizes, feats, gt, gt_labels, gt_counts, img_shapes = _problem()
    head = _retina(T, loss_cls=dict(type='GHMC', bins=30, momentum=0.75),
                   loss_bbox=T.GHMR(mu=0.02, bins=10, momentum=0.7, loss_weight=2.0))
    assert head.loss_cls.acc_sum.is_cuda and not head.loss_cls.acc_sum.any()
    cls, reg = head(feats)
    anchors, flags = head.get_anchors(sizes)
    losses = head.loss(cls, reg, anchors, flags, gt, gt_labels, gt_counts, img_shapes)
    cot = torch.tensor([1.0, 0.5], device="cuda")
    grads = torch.autograd.grad(losses, list(cls) + list(reg) + list(head.parameters()) + feats, cot)
    torch.cuda.synchronize()
    targets = T.anchor_target_all(torch.cat(anchors), torch.cat(flags), gt, gt_labels, gt_counts, img_shapes,
                                  pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, target_means=head.target_means,
                                  target_stds=head.target_stds)[:4]
    acc_ref = [np.zeros(30, f32), np.zeros(10, f32)]
    ref = R.ghm_head_loss([c.detach().float().cpu().numpy() for c in cls], [r.detach().float().cpu().numpy() for r in reg],
                          *[t.cpu().numpy() for t in targets], *acc_ref, g=(1.0, 1.0), **dict(CFG, num_classes=4))
    assert ref["cnt"][1].sum() > 0, "the problem has positives"
    got = losses.detach().cpu().numpy().astype(np.float64)
    want = ref["losses64"] * np.array([1.0, 2.0])
    assert abs(got[0] - want[0]) <= R.K * R.U * ref["mag"][0] + np.spacing(f32(want[0]))
    assert abs(got[1] - want[1]) <= 0.5 * np.spacing(f32(want[1])) * (1 + 2.0 ** -20)
    for l in range(2):                                       # loss_bbox's weight 2 doubles the cotangent 0.5: exact
        _same_bits(grads[l], ref["dcls"][l], torch.bfloat16, "head dcls[%d]" % l)
        _same_bits(grads[2 + l], ref["dreg"][l], torch.bfloat16, "head dreg[%d]" % l)
    for a, r in zip((head.loss_cls.acc_sum, head.loss_bbox.acc_sum), acc_ref):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), r.view(np.uint32))
    for gp in grads[4:]:
        assert torch.isfinite(gp.float()).all() and gp.float().abs().sum().item() > 0


def test_retina_head_without_the_keywords_is_unchanged(T):
    sizes, feats, gt, gt_labels, gt_counts, img_shapes = _problem()
    head = _retina(T)
    cls, reg = head(feats)
    anchors, flags = head.get_anchors(sizes)
    losses = head.loss(cls, reg, anchors, flags, gt, gt_labels, gt_counts, img_shapes)
    labels, lw, bt, bw, num_pos = T.anchor_target_all(
        torch.cat(anchors), torch.cat(flags), gt, gt_labels, gt_counts, img_shapes, pos_iou_thr=0.5, neg_iou_thr=0.4,
        min_pos_iou=0, target_means=head.target_means, target_stds=head.target_stds)[:5]
    direct = T.anchor_head_loss(cls, reg, labels, lw, bt, bw, avg_factor=num_pos, num_classes=4, beta=1.0 / 9.0,
                                gamma=2.0, alpha=0.25)
    assert torch.equal(_bits(losses), _bits(direct)) and (losses > 0).all()
    ga = torch.autograd.grad(losses.sum(), list(cls) + list(reg), retain_graph=True)
    gb = torch.autograd.grad(direct.sum(), list(cls) + list(reg))
    for a, b in zip(ga, gb):
        assert torch.equal(_bits(a), _bits(b))
