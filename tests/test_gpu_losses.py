"""GPU tests of the loss kernels (anchor_head_loss / rpn_loss / bbox_head_loss, csrc/loss.hip) against the CPU oracle
tests/loss_ref.py: small shapes over every layout, dtype and loss; the chain from anchor_target and
sample_rois at full size; graph replay; and every entry point under guard-banded, poisoned outputs with exact-size
workspaces (tests/guard_util.py).

Bounds (DESIGN.md §4e derives K): smooth-L1 gradients equal the float32 oracle as bit patterns (16-bit: that value
rounded to nearest even); the other gradients |got - ref64| <= K * 2^-24 * |w * s| * D (+ one ulp16 of ref for a 16-bit
output); losses |got - ref64| <= K * 2^-24 * mag + spacing(ref)."""
import inspect

import numpy as np
import pytest
import torch

import guard_util as G
import loss_ref as R
import target_cases as C4

pytestmark = pytest.mark.gpu

K = 16
U = 2.0 ** -24
LEVELS = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 1)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT = {torch.bfloat16: 7, torch.float16: 10}
ENTERED, WS_SEEN = set(), {}        # what ran under the guard in this run (checked by the last test of the file)


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _ulp16(ref, dtype):
    """Spacing of the 16-bit type at |ref| (its smallest subnormal below the normal range)."""
    if dtype == torch.float32:
        return np.zeros_like(ref)
    emin = -14 if dtype == torch.float16 else -126
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref), where=ref != 0, out=np.full(ref.shape, float(emin))))
    return 2.0 ** (np.maximum(e, emin) - MANT[dtype])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _np64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _check_elementwise(got, ref, scale, D, dtype, what):
    got = _np64(got)
    assert got.shape == ref.shape, what
    assert np.array_equal(got == 0, ref == 0), "%s: zero pattern differs at %d elements" % (
        what, int(((got == 0) != (ref == 0)).sum()))
    assert np.all(np.isfinite(got)), what
    tol = K * U * scale * D + _ulp16(ref, dtype)
    err = np.abs(got - ref)
    unit = U * scale * D
    worst = float((err[unit > 0] / unit[unit > 0]).max()) if np.any(unit > 0) else 0.0
    assert np.all(err <= tol), "%s: %d beyond the bound, worst %.2f x 2^-24 |w s| D" % (what, int((err > tol).sum()), worst)
    return worst


def _check_smooth_l1(got, ref32, dtype, what):
    want = torch.from_numpy(np.ascontiguousarray(ref32)).to(dtype)
    assert torch.equal(_bits(got.detach().cpu().contiguous()), _bits(want)), "%s: smooth-L1 gradient bits differ at %d" % (
        what, int((_bits(got.detach().cpu().contiguous()) != _bits(want)).sum()))


def _check_losses(got, ref, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    worst = []
    for k in range(2):
        tol = K * U * ref["mag"][k] + float(np.spacing(np.float32(abs(ref["losses"][k]))))
        err = abs(got[k] - ref["losses"][k])
        worst.append(err / (U * ref["mag"][k]) if ref["mag"][k] > 0 else 0.0)
        assert err <= tol, "%s: loss %d: got %r, ref %r, error %g > %g" % (what, k, got[k], ref["losses"][k], err, tol)
    return worst


def _stored(a, dtype):
    """a rounded to the storage dtype, as float32: a 16-bit prediction can then equal its target, which gives d = 0
    exactly and not a rounding residue whose gradient lies below the 16-bit type's smallest subnormal."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


def _layout(t, nhwc):
    return t.contiguous(memory_format=torch.channels_last) if nhwc else t.contiguous()


def dense_case(B, A, Cn, levels, dtype, layout, seed, pos=0.01):
    """Random head outputs (stored values) and targets; NaN / Inf planted wherever the weight is 0."""
    g = np.random.default_rng(seed)
    N = sum(h * w for h, w in levels) * A
    labels = np.where(g.random((B, N)) < pos, g.integers(1, Cn + 1, (B, N)), 0).astype(np.int64)
    labels[:, ::97] = g.integers(1, Cn + 1, labels[:, ::97].shape)             # positives on every level
    lw = g.choice(np.array([0, 1, 0.5], np.float32), (B, N), p=[0.3, 0.5, 0.2])
    bt = g.normal(0, 0.3, (B, N, 4)).astype(np.float32)
    bt[..., 0] = _stored(bt[..., 0], dtype)             # representable, so that "d = 0" below is exact in 16-bit too
    bw = np.where((labels > 0)[..., None], g.choice(np.array([1, 0.5], np.float32), (B, N, 4)), 0).astype(np.float32)
    cls, reg, n0 = [], [], 0
    for l, (h, w) in enumerate(levels):
        n1 = n0 + h * w * A
        c = np.clip(g.normal(0, 1.5, (B, A * Cn, h, w)), -4, 4).astype(np.float32)
        r = g.normal(0, 0.3, (B, 4 * A, h, w)).astype(np.float32)
        r[:, ::4] = R.unflatten_head(bt[:, n0:n1], A, 4, h, w)[:, ::4] + \
            g.choice(np.array([0, 0.05, -0.05, 1.0], np.float32), (B, A, h, w))   # d = 0, inside and outside beta
        w0 = R.unflatten_head(np.broadcast_to(lw[:, n0:n1, None], (B, h * w * A, Cn)), A, Cn, h, w) == 0
        c[w0] = g.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(w0.sum()))
        b0 = R.unflatten_head(bw[:, n0:n1], A, 4, h, w) == 0
        r[b0 & (g.random(b0.shape) < 0.5)] = np.nan
        nhwc = {"nchw": (False, False), "nhwc": (True, True), "mixed": (l % 2 == 0, l % 2 == 1)}[layout]
        cls.append(_layout(torch.from_numpy(c).to(dtype).cuda(), nhwc[0]))
        reg.append(_layout(torch.from_numpy(r).to(dtype).cuda(), nhwc[1]))
        n0 = n1
    return cls, reg, labels, lw, bt, bw


def run_dense(T, cls, reg, labels, lw, bt, bw, avg_gpu, avg_ref, Cn, beta, gamma, alpha, g, what, targets_gpu=None):
    """forward + backward twice (bitwise equal), then everything against the oracle.  Returns the worst errors."""
    dtype = cls[0].dtype
    tg = targets_gpu or [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):
        heads = [t.detach().requires_grad_(True) for t in cls + reg]
        L = len(cls)
        losses = T.anchor_head_loss(heads[:L], heads[L:], *tg, avg_gpu, num_classes=Cn, beta=beta, gamma=gamma,
                                    alpha=alpha)
        grads = torch.autograd.grad(losses, heads, gt)
        runs.append((losses, grads))
    torch.cuda.synchronize()
    (losses, grads), (losses2, grads2) = runs
    assert losses.shape == (2,) and losses.dtype == torch.float32
    assert torch.equal(_bits(losses), _bits(losses2)), what + ": losses differ run to run"
    for a, b, h in zip(grads, grads2, cls + reg):
        assert a.shape == h.shape and a.dtype == h.dtype and a.stride() == h.stride(), (what, a.stride(), h.stride())
        assert torch.equal(_bits(a), _bits(b)), what + ": gradients differ run to run"
    ref = R.anchor_head_loss([t.float().cpu().numpy() for t in cls], [t.float().cpu().numpy() for t in reg],
                             labels, lw, bt, bw, avg_ref, Cn, beta, gamma, alpha, g)
    wl = _check_losses(losses, ref, what)
    L = len(cls)
    wg = 0.0
    for l in range(L):
        wg = max(wg, _check_elementwise(grads[l], ref["dcls"][l], ref["scale_cls"][l], ref["D"][l], dtype,
                                        "%s: dcls[%d]" % (what, l)))
        _check_smooth_l1(grads[L + l], ref["dreg32"][l], dtype, "%s: dreg[%d]" % (what, l))
        assert np.array_equal(_np64(grads[L + l]) == 0, ref["dreg"][l] == 0), what
    print("%s: losses %s, worst loss error %.2f / %.2f, worst gradient error %.2f (x 2^-24 of the bound's unit)" % (
        what, losses.detach().cpu().numpy(), wl[0], wl[1], wg))
    return ref


LOSSES = {"bce": (None, 0.25), "focal2": (2.0, 0.25), "focal0": (0.0, 0.25)}


@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("A,Cn", [(3, 1), (2, 5), (9, 20)])
def test_dense_small_vs_oracle(T, A, Cn, dt, loss):
    gamma, alpha = LOSSES[loss]
    dtype = DTYPES[dt]
    g = (768.0, 320.0) if dt == "f16" else (1.5, 0.75)             # an fp16 loss scale arrives as the cotangent
    seed = 0
    for B in (1, 3):
        for layout in ("nchw", "nhwc", "mixed"):
            seed += 1
            case = dense_case(B, A, Cn, LEVELS, dtype, layout, seed)
            run_dense(T, *case, 23.0, 23.0, Cn, 1.0 / 9.0, gamma, alpha, g,
                      "A%d C%d %s %s B%d %s" % (A, Cn, dt, loss, B, layout))


@pytest.mark.parametrize("dt,layout,loss", [("f32", "nchw", "focal2"), ("bf16", "nhwc", "focal2"),
                                            ("f16", "nhwc", "bce"), ("f32", "nhwc", "bce")])
def test_dense_many_workgroups(T, dt, layout, loss):
    """64 x 100, A = 9, C = 20: 2.3 M logits, more chunks than one grid pass and 256 partials."""
    gamma, alpha = LOSSES[loss]
    g = (768.0, 320.0) if dt == "f16" else (1.5, 0.75)
    case = dense_case(2, 9, 20, [(64, 100)], DTYPES[dt], layout, 77)
    num_pos = torch.tensor([311, 5], dtype=torch.int32, device="cuda")
    run_dense(T, *case, num_pos, np.array([311, 5]), 20, 0.5, gamma, alpha, g, "64x100 %s %s %s" % (dt, layout, loss))


def test_avg_factor_forms_and_unaligned_views(T):
    """A number, a tensor, a tuple, a sum of zero; head tensors that start 4 bytes into an allocation (no 16-byte
    loads or stores there)."""
    cls, reg, labels, lw, bt, bw = dense_case(2, 3, 1, LEVELS[:3], torch.float32, "nchw", 5)
    a = torch.tensor([3, 4], dtype=torch.int32, device="cuda")
    b = torch.tensor([10, 0, 2], dtype=torch.int32, device="cuda")
    z = torch.zeros(2, dtype=torch.int32, device="cuda")
    for gpu, ref in ((19.0, 19.0), (a, np.array([3, 4])), ((a, b), (np.array([3, 4]), np.array([10, 0, 2]))),
                     ((z, z), (np.zeros(2, int), np.zeros(2, int)))):
        out = run_dense(T, cls, reg, labels, lw, bt, bw, gpu, ref, 1, 1.0 / 9.0, None, 0.25, (1.0, 1.0), "avg forms")
        assert out["avg"] == R.divisor(ref)
    shifted = []
    for t in cls + reg:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        shifted.append(v)
    run_dense(T, shifted[:3], shifted[3:], labels, lw, bt, bw, 19.0, 19.0, 1, 1.0 / 9.0, None, 0.25, (1.0, 1.0),
              "unaligned views")


# ---- RoI head ---------------------------------------------------------------------------------------------------
def roi_case(Rn, Cn, specific, dtype, seed, all_zero=False):
    g = np.random.default_rng(seed)
    cols = 4 * Cn if specific else 4
    cls = np.clip(g.normal(0, 2, (Rn, Cn)), -6, 6).astype(np.float32)
    reg = g.normal(0, 0.5, (Rn, cols)).astype(np.float32)
    labels = np.where(g.random(Rn) < 0.3, g.integers(1, Cn, Rn) if Cn > 1 else 0, 0).astype(np.int64)
    lw = g.choice(np.array([0, 1, 0.5], np.float32), Rn, p=[0.25, 0.6, 0.15])
    if all_zero:
        lw[:] = 0
    pad = lw == 0                                                   # sample_rois' padding rows: weight 0, label 0
    labels[pad] = 0
    cls[pad] = np.nan
    bt = g.normal(0, 0.5, (Rn, 4)).astype(np.float32)
    bt[:, 0] = _stored(bt[:, 0], dtype)
    bw = np.where(((labels > 0) & ~pad)[:, None], np.float32(1), np.float32(0)) * np.ones((1, 4), np.float32)
    reg[pad] = np.inf
    rows = np.arange(Rn)
    col = (4 * labels if specific else np.zeros(Rn, np.int64))
    reg[rows[~pad], col[~pad]] = bt[~pad, 0] + g.choice(np.array([0, 0.3, -0.3, 2.0], np.float32), int((~pad).sum()))
    return (torch.from_numpy(cls).to(dtype).cuda(), torch.from_numpy(reg).to(dtype).cuda(), labels, lw, bt,
            bw.astype(np.float32))


def run_roi(T, cls, reg, labels, lw, bt, bw, avg_gpu, avg_ref, beta, g, what, targets_gpu=None):
    dtype = cls.dtype
    tg = targets_gpu or [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):
        x, r = cls.detach().requires_grad_(True), reg.detach().requires_grad_(True)
        losses = T.bbox_head_loss(x, r, *tg, avg_factor=avg_gpu, beta=beta)
        runs.append((losses, torch.autograd.grad(losses, [x, r], gt)))
    torch.cuda.synchronize()
    (losses, (dc, dr)), (losses2, (dc2, dr2)) = runs
    assert torch.equal(_bits(losses), _bits(losses2)) and torch.equal(_bits(dc), _bits(dc2)) and \
        torch.equal(_bits(dr), _bits(dr2)), what + ": run to run"
    assert dc.shape == cls.shape and dr.shape == reg.shape and dc.dtype == dtype and dr.dtype == dtype
    ref = R.bbox_head_loss(cls.float().cpu().numpy(), reg.float().cpu().numpy(), labels, lw, bt, bw, avg_ref, beta, g)
    wl = _check_losses(losses, ref, what)
    wg = _check_elementwise(dc, ref["dcls"], ref["scale_cls"], ref["D"], dtype, what + ": dcls")
    _check_smooth_l1(dr, ref["dreg32"], dtype, what + ": dreg")
    assert np.array_equal(_np64(dr) == 0, ref["dreg"] == 0), what
    print("%s: losses %s avg %g, worst loss error %.2f / %.2f, worst gradient error %.2f" % (
        what, losses.detach().cpu().numpy(), float(ref["avg"]), wl[0], wl[1], wg))
    return ref, losses


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("Cn", [2, 81, 1024])
def test_roi_vs_oracle(T, Cn, dt):
    g = (512.0, 256.0) if dt == "f16" else (1.25, 0.5)
    seed = 0
    for Rn in (1, 7, 512, 1031):
        for specific in (True, False):
            seed += 1
            case = roi_case(Rn, Cn, specific, DTYPES[dt], seed)
            n = torch.tensor([Rn // 2, 3], dtype=torch.int32, device="cuda")
            forms = {0: (None, None), 1: (37.0, 37.0), 2: (n, np.array([Rn // 2, 3])),
                     3: ((n, n[:1]), (np.array([Rn // 2, 3]), np.array([Rn // 2])))}
            gpu, ref = forms[seed % 4]
            run_roi(T, *case, gpu, ref, 1.0, g, "R%d C%d %s specific=%s avg form %d" % (Rn, Cn, dt, specific, seed % 4))


def test_roi_all_rows_weight_zero_and_bad_labels(T):
    case = roi_case(33, 81, True, torch.float32, 3, all_zero=True)
    ref, losses = run_roi(T, *case, None, None, 1.0, (1.0, 1.0), "all rows weight 0")
    assert ref["avg"] == 1 and np.all(losses.detach().cpu().numpy() == 0)
    # a label outside [0, C) on a CUDA tensor: the row counts as weight 0 on the device (no fault, no assert), but
    # still counts toward avg_factor=None, which is the number of rows with label_weights > 0
    cls, reg, labels, lw, bt, bw = roi_case(40, 9, True, torch.float32, 4)
    labels[5], lw[5], bw[5] = 9, 1.0, 1.0
    labels[6], lw[6], bw[6] = -3, 1.0, 1.0
    labels[7], lw[7] = 1 << 40, 0.5
    run_roi(T, cls, reg, labels, lw, bt, bw, None, None, 1.0, (1.0, 1.0), "labels out of range")


# ---- the chain at full size --------------------------------------------------------------------------------------
def test_chain_anchor_target_rpn_loss_backward(T):
    case = C4.anchor_case(**C4.CASES["b2"])
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in case.items()}
    labels, lw, bt, bw, num_pos, num_neg, _ = T.anchor_target(**d, seed=3, target_stds=(0.5, 0.5, 0.5, 0.5))
    g = torch.Generator().manual_seed(5)
    cls = [(torch.randn(2, 3, h, w, generator=g) * 2).to(torch.bfloat16).cuda().contiguous(
        memory_format=torch.channels_last) for (h, w), _ in C4.LEVELS]
    reg = [(torch.randn(2, 12, h, w, generator=g) * 0.5).to(torch.bfloat16).cuda().contiguous(
        memory_format=torch.channels_last) for (h, w), _ in C4.LEVELS]
    heads = [t.requires_grad_(True) for t in cls + reg]
    losses = T.rpn_loss(heads[:5], heads[5:], labels, lw, bt, bw, avg_factor=(num_pos, num_neg))
    losses.backward(torch.tensor([1.0, 1.0], device="cuda"))
    torch.cuda.synchronize()
    tn = [t.cpu().numpy() for t in (labels, lw, bt, bw)]
    assert int((tn[1] > 0).sum()) == int(num_pos.sum() + num_neg.sum()) > 0 and int((tn[3] > 0).sum()) > 0
    ref = R.anchor_head_loss([t.detach().float().cpu().numpy() for t in cls],
                             [t.detach().float().cpu().numpy() for t in reg], *tn,
                             (num_pos.cpu().numpy(), num_neg.cpu().numpy()), 1, 1.0 / 9.0, None)
    wl = _check_losses(losses, ref, "chain")
    wg = 0.0
    for l in range(5):
        assert heads[l].grad.stride() == heads[l].stride() and heads[l].grad.dtype == torch.bfloat16
        wg = max(wg, _check_elementwise(heads[l].grad, ref["dcls"][l], ref["scale_cls"][l], ref["D"][l],
                                        torch.bfloat16, "chain dcls[%d]" % l))
        _check_smooth_l1(heads[5 + l].grad, ref["dreg32"][l], torch.bfloat16, "chain dreg[%d]" % l)
    print("chain: losses %s avg %g, worst loss error %.2f / %.2f, worst gradient error %.2f" % (
        losses.detach().cpu().numpy(), float(ref["avg"]), wl[0], wl[1], wg))


def _sampled_rois(T):
    import test_gpu_targets as TT
    props, counts = TT._rpn_output(T, 2)
    gt, glab = TT._roi_gts(props.cpu().numpy(), counts.cpu().numpy(), 40, (40, 3), 3)
    out = T.sample_rois(props, counts, torch.from_numpy(gt).cuda(), torch.from_numpy(glab).cuda(),
                        torch.tensor([40, 3], dtype=torch.int32).cuda(), num=512, seed=5, neg_pos_ub=2, pos_fraction=0.1)
    return out[1:5]


def test_chain_sample_rois_bbox_head_loss(T):
    tg = list(_sampled_rois(T))
    tn = [t.cpu().numpy() for t in tg]
    Rn = tn[0].shape[0]
    assert (tn[1] == 0).sum() > 0 and (tn[0] > 0).sum() > 0                 # padding rows and positives
    g = torch.Generator().manual_seed(6)
    cls = torch.randn(Rn, 81, generator=g).mul(2).cuda()
    reg = torch.randn(Rn, 324, generator=g).mul(0.3).cuda()
    cls[tg[1] == 0] = float("nan")
    run_roi(T, cls, reg, *tn, None, None, 1.0, (1.0, 1.0), "sample_rois chain", targets_gpu=tg)


# ---- graph -------------------------------------------------------------------------------------------------------
def test_graph_replay_matches_eager(T):
    """Forward + backward of rpn_loss and of bbox_head_loss captured once, replayed on new logits, targets and
    num_pos / num_neg: a host synchronisation or an allocation inside the library would break the capture."""
    def new(seed):
        c = dense_case(2, 3, 1, LEVELS, torch.bfloat16, "nhwc", seed)
        r = roi_case(200, 21, True, torch.float32, seed)
        n = np.random.default_rng(seed).integers(1, 200, (2, 2)).astype(np.int32)
        return c, r, n
    c, r, n = new(1)
    heads = [t.clone().requires_grad_(True) for t in c[0] + c[1]]
    dt = [torch.from_numpy(a).cuda() for a in c[2:]]
    rx, rr = r[0].clone().requires_grad_(True), r[1].clone().requires_grad_(True)
    rt = [torch.from_numpy(a).cuda() for a in r[2:]]
    npos, nneg = torch.from_numpy(n[0]).cuda(), torch.from_numpy(n[1]).cuda()
    cot = torch.tensor([2.0, 0.5], device="cuda")

    def step():
        l1 = T.rpn_loss(heads[:5], heads[5:], *dt, avg_factor=(npos, nneg))
        l2 = T.bbox_head_loss(rx, rr, *rt, avg_factor=npos)
        g1 = torch.autograd.grad(l1, heads, cot)
        g2 = torch.autograd.grad(l2, [rx, rr], cot)
        return [l1, l2] + list(g1) + list(g2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    seen = []
    for seed in (2, 3):
        c, r, n = new(seed)
        with torch.no_grad():
            for dst, src in zip(heads, c[0] + c[1]):
                dst.copy_(src)
            for dst, src in zip(dt + rt, list(c[2:]) + list(r[2:])):
                dst.copy_(torch.from_numpy(src))
            rx.copy_(r[0])
            rr.copy_(r[1])
            npos.copy_(torch.from_numpy(n[0]))
            nneg.copy_(torch.from_numpy(n[1]))
        graph.replay()
        eager = step()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager):
            assert torch.equal(_bits(a), _bits(b))
        seen.append(captured[0].clone())
    assert not torch.equal(seen[0], seen[1])


# ---- under the guard ---------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import loss_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, loss_ops, g)
    yield g
    torch.cuda.synchronize()


def _clean(g, names):
    log = list(g.ws_log)
    found = g.check()
    assert not found, "\n".join(found)
    ENTERED.update(names)
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


@pytest.mark.parametrize("dt,layout", [("f32", "mixed"), ("bf16", "nhwc"), ("f16", "nchw")])
def test_guarded_dense(T, guard, dt, layout):
    g = (768.0, 320.0) if dt == "f16" else (1.5, 0.75)
    case = dense_case(3, 9, 20, LEVELS, DTYPES[dt], layout, 11)
    run_dense(T, *case, 23.0, 23.0, 20, 1.0 / 9.0, 2.0, 0.25, g, "guarded %s %s" % (dt, layout))
    _clean(guard, ["anchor_head_loss_fwd", "anchor_head_loss_bwd"])
    case = dense_case(1, 3, 1, LEVELS, DTYPES[dt], layout, 12)
    run_dense(T, *case, 23.0, 23.0, 1, 1.0 / 9.0, None, 0.25, g, "guarded rpn %s %s" % (dt, layout))
    _clean(guard, [])


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_guarded_roi(T, guard, dt):
    g = (512.0, 256.0) if dt == "f16" else (1.25, 0.5)
    for Rn, Cn, specific in ((1031, 81, True), (7, 1024, True), (512, 2, False), (1, 81, True)):
        run_roi(T, *roi_case(Rn, Cn, specific, DTYPES[dt], Rn), None, None, 1.0, g, "guarded R%d C%d" % (Rn, Cn))
        _clean(guard, ["bbox_head_loss_fwd", "bbox_head_loss_bwd"])


def test_guarded_roi_no_rows(T, guard):
    """R = 0 still runs one workgroup and the last launch: losses of 0, a divisor of 1."""
    from torch_detection_amd import loss_ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    losses, avg = loss_ops.bbox_head_loss_fwd(z(0, 5), z(0, 20), z(0, dt=torch.int64), z(0), z(0, 4), z(0, 4), None, 1.0)
    _clean(guard, [])
    assert losses.tolist() == [0.0, 0.0] and avg.tolist() == [1.0]


def test_every_loss_entry_point_ran_under_the_guard():
    """Counts what the guarded tests above did IN THIS RUN (run the file as a whole): every public wrapper of
    loss_ops.py returned under the guard, and every tdn_loss*_workspace_bytes query was answered at its exact size
    (rounded up only to the 256-byte alignment the header asks for)."""
    from torch_detection_amd import loss_ops
    public = sorted(n for n, v in vars(loss_ops).items()
                    if inspect.isfunction(v) and v.__module__ == loss_ops.__name__ and not n.startswith("_"))
    assert public == ["anchor_head_loss_bwd", "anchor_head_loss_fwd", "bbox_head_loss_bwd", "bbox_head_loss_fwd"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in ("anchor_head_loss_fwd", "bbox_head_loss_fwd"):
        assert op in WS_SEEN, op
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)
