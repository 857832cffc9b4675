"""GPU: the Libra R-CNN pieces beside the BFP neck against tests/libra_ref.py: IoU-balanced negative
sampling (``sample_assigned_iou_balanced``, ``sample_rois(neg_sampler='iou_balanced')``: masks, counts and rows equal to
the oracle's, ``'random'`` equal to today's outputs) and balanced L1 in the RoI box loss,
``bbox_head_loss(reg_loss='balanced_l1')``; the smooth-L1 path with the new keywords left at their defaults must give
today's bits.  Every call runs twice and must give the same bits.

Bounds, those of tests/test_gpu_losses.py (K = 16, u = 2^-24): losses |got - ref64| <= K u mag + spacing(ref); the
classification gradients |got - ref64| <= K u |w s| (+ one ulp16); box gradients on the OUTER branch and every exact zero
equal the float32 oracle as bit patterns (16-bit: that value rounded to nearest even); box gradients on the inner branch,
which go through ``log1pf``, |got - ref64| <= K u |w s| Dmax (+ one ulp16), Dmax = gamma + alpha |1 - beta| / beta the
largest |dl| there."""
import inspect

import numpy as np
import pytest
import torch

import guard_util as G
import libra_ref as R
import loss_ref as L
import target_cases as TC
import target_ref as TR
import test_gpu_losses as TL
import test_gpu_targets as TT
from test_gpu_losses import DTYPES, K, U, _bits, _np64, _ulp16

pytestmark = pytest.mark.gpu

ENTERED, WS_SEEN = set(), {}
PARAMS = [(1.0, 0.5, 1.5), (1.0 / 9.0, 0.5, 1.5)]                      # (beta, alpha, gamma)


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def run_balanced(T, cls, reg, labels, lw, bt, bw, avg_gpu, avg_ref, beta, alpha, gamma, g, what):
    dtype = cls.dtype
    tg = [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    gt = torch.tensor(g, dtype=torch.float32, device="cuda")
    runs = []
    for _ in range(2):
        x, r = cls.detach().requires_grad_(True), reg.detach().requires_grad_(True)
        losses = T.bbox_head_loss(x, r, *tg, avg_factor=avg_gpu, beta=beta, reg_loss="balanced_l1", reg_alpha=alpha,
                                  reg_gamma=gamma)
        runs.append((losses, torch.autograd.grad(losses, [x, r], gt)))
    torch.cuda.synchronize()
    (losses, (dc, dr)), (losses2, (dc2, dr2)) = runs
    assert torch.equal(_bits(losses), _bits(losses2)) and torch.equal(_bits(dc), _bits(dc2)) and \
        torch.equal(_bits(dr), _bits(dr2)), what + ": run to run"
    assert dc.shape == cls.shape and dr.shape == reg.shape and dc.dtype == dtype and dr.dtype == dtype
    ref = R.bbox_head_loss_balanced(cls.float().cpu().numpy(), reg.float().cpu().numpy(), labels, lw, bt, bw, avg_ref,
                                    beta, alpha, gamma, g)
    wl = TL._check_losses(losses, ref, what)
    wg = TL._check_elementwise(dc, ref["dcls"], ref["scale_cls"], ref["D"], dtype, what + ": dcls")
    got = _np64(dr)
    assert np.all(np.isfinite(got)), what
    assert np.array_equal(got == 0, ref["dreg"] == 0), what + ": zero pattern of dreg"
    # outer branch and zeros: bits of the float32 oracle
    want = torch.from_numpy(np.ascontiguousarray(ref["dreg32"])).to(dtype)
    exact = torch.from_numpy(ref["outer"] | (ref["dreg"] == 0))
    same = _bits(dr.detach().cpu().contiguous()) == _bits(want)
    assert bool(same[exact].all()), "%s: %d outer-branch / zero gradients differ in bits" % (what, int((~same[exact]).sum()))
    # inner branch: the bound
    dmax = float(np.float32(gamma)) + float(np.float32(alpha)) * abs(1 - float(np.float32(beta))) / float(np.float32(beta))
    unit = U * ref["scale_reg"] * dmax
    err = np.abs(got - ref["dreg"])
    tol = K * unit + _ulp16(ref["dreg"], dtype)
    inner = ~ref["outer"] & (ref["dreg"] != 0)
    assert (inner.any() and ref["outer"].any()) or cls.shape[0] < 1000, what
    worst = float((err[inner] / unit[inner]).max()) if inner.any() else 0.0
    assert np.all(err <= tol), "%s: %d box gradients beyond the bound, worst %.2f" % (what, int((err > tol).sum()), worst)
    print("%s: losses %s avg %g, worst loss error %.2f / %.2f, worst gradient error cls %.2f box %.2f "
          "(x 2^-24 of the bound's unit; bound %d)" % (what, losses.detach().cpu().numpy(), float(ref["avg"]), wl[0], wl[1],
                                                        wg, worst, K))
    return ref, losses


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("Cn", [2, 81])
def test_balanced_l1_vs_oracle(T, Cn, dt):
    g = (512.0, 256.0) if dt == "f16" else (1.25, 0.5)
    seed = 40
    for Rn in (1, 7, 1031):
        for specific in (True, False):
            seed += 1
            case = TL.roi_case(Rn, Cn, specific, DTYPES[dt], seed)
            n = torch.tensor([Rn // 2, 3], dtype=torch.int32, device="cuda")
            forms = {0: (None, None), 1: (37.0, 37.0), 2: (n, np.array([Rn // 2, 3]))}
            gpu, ref = forms[seed % 3]
            beta, alpha, gamma = PARAMS[seed % 2]
            run_balanced(T, *case, gpu, ref, beta, alpha, gamma, g,
                         "balanced R%d C%d %s specific=%s beta=%.3g" % (Rn, Cn, dt, specific, beta))


def test_zero_difference_and_zero_weight_are_exact(T):
    """pred == target: loss 0 and gradient exactly 0; weight 0: not evaluated (the prediction there is inf)."""
    Rn, Cn = 9, 5
    cls = torch.zeros(Rn, Cn, device="cuda")
    labels = np.arange(Rn, dtype=np.int64) % Cn
    bt = np.linspace(-1, 1, Rn * 4, dtype=np.float32).reshape(Rn, 4)
    reg = torch.zeros(Rn, 4 * Cn, device="cuda")
    for r in range(Rn):
        reg[r, 4 * labels[r]:4 * labels[r] + 4] = torch.from_numpy(bt[r]).cuda()
    bw = np.ones((Rn, 4), np.float32)
    bw[3] = 0
    reg[3] = float("inf")
    lw = np.ones(Rn, np.float32)
    tg = [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    r_ = reg.requires_grad_(True)
    losses = T.bbox_head_loss(cls, r_, *tg, beta=0.5, reg_loss="balanced_l1")
    dr, = torch.autograd.grad(losses[1], [r_])
    assert float(losses[1].detach()) == 0.0 and bool((dr == 0).all())


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_smooth_l1_with_the_new_keywords_at_their_defaults_gives_todays_bits(T, dt):
    """``reg_loss='smooth_l1'`` spelled out (and the balanced parameters set to anything) == the call without them ==
    the float32 smooth-L1 oracle of tests/loss_ref.py, bit for bit."""
    case = TL.roi_case(1031, 81, True, DTYPES[dt], 7)
    cls, reg, labels, lw, bt, bw = case
    tg = [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    gt = torch.tensor((1.25, 0.5), dtype=torch.float32, device="cuda")
    outs = []
    for kw in ({}, dict(reg_loss="smooth_l1", reg_alpha=0.3, reg_gamma=2.0)):
        x, r = cls.detach().requires_grad_(True), reg.detach().requires_grad_(True)
        losses = T.bbox_head_loss(x, r, *tg, beta=0.5, **kw)
        outs.append((losses,) + torch.autograd.grad(losses, [x, r], gt))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))
    ref = L.bbox_head_loss(cls.float().cpu().numpy(), reg.float().cpu().numpy(), labels, lw, bt, bw, None, 0.5, (1.25, 0.5))
    TL._check_smooth_l1(outs[1][2], ref["dreg32"], DTYPES[dt], "smooth L1 through the new keywords")


def test_graph_replay_matches_eager(T):
    case = TL.roi_case(1031, 81, True, torch.bfloat16, 9)
    cls, reg, labels, lw, bt, bw = case
    tg = [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    gt = torch.tensor((1.0, 1.0), dtype=torch.float32, device="cuda")
    x, r = cls.detach().clone().requires_grad_(True), reg.detach().clone().requires_grad_(True)

    def step():
        losses = T.bbox_head_loss(x, r, *tg, reg_loss="balanced_l1")
        return (losses,) + torch.autograd.grad(losses, [x, r], gt)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for seed in (10, 11):
        c2, r2, labels2, lw2, bt2, bw2 = TL.roi_case(1031, 81, True, torch.bfloat16, seed)
        with torch.no_grad():
            x.copy_(c2)
            r.copy_(r2)
        for t, a in zip(tg, (labels2, lw2, bt2, bw2)):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        eager = step()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(eager, held)), seed


# ---- IoU-balanced negative sampling ---------------------------------------------------------------------------------
SETTINGS = [(ft, ff, nb) for ft in (-1.0, 0.0, 0.1) for ff in (0.0, 0.25) for nb in (1, 3)]
NAMES = ("rois", "labels", "label_weights", "bbox_targets", "bbox_weights", "pos_gt_inds", "num_pos", "num_neg")


def _candidates(seed=0, P=2100, G=40, gt_counts=(0, 1, 37), counts=(2100, 1800, 2063)):
    """B = 3 images of about 2100 proposals: jittered copies of the ground truths (IoU from 0 to 1 with them) and boxes
    elsewhere; an image without ground truths, one with one, one with 37."""
    g = np.random.default_rng(seed)
    Bn = len(gt_counts)
    gt = np.zeros((Bn, G, 4), np.float32)
    props = np.zeros((Bn, P, 5), np.float32)
    for b in range(Bn):
        n = gt_counts[b]
        xy = g.uniform(0, 900, (n, 2))
        wh = g.uniform(40, 300, (n, 2))
        gt[b, :n] = np.floor(np.concatenate([xy, xy + wh], 1)).astype(np.float32)
        far = g.uniform(0, 1200, (P, 2))
        box = np.concatenate([far, far + g.uniform(16, 200, (P, 2))], 1)
        if n:
            near = g.random(P) < 0.7
            src = gt[b, g.integers(0, n, P)]
            size = (src[:, 2:] - src[:, :2])
            jit = src + g.normal(0, 1, (P, 4)) * np.tile(size, 2) * g.choice([0.02, 0.1, 0.25, 0.5], (P, 1))
            jit[:, 2:] = np.maximum(jit[:, 2:], jit[:, :2] + 2)
            box[near] = jit[near]
        props[b, :, :4] = box.astype(np.float32)
        props[b, :, 4] = g.random(P)
    labels = g.integers(1, 81, (Bn, G)).astype(np.int64)
    return props, np.asarray(counts, np.int32), gt, labels, np.asarray(gt_counts, np.int32)


def _same(got, ref, name):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == ref.dtype and got.shape == ref.shape, name
    assert np.array_equal(TT._bits(got), TT._bits(ref)), "%s: %d differ" % (name, int((got != ref).sum()))


def test_sample_assigned_iou_balanced_vs_oracle(T):
    props, counts, gt, labels, gt_counts = _candidates()
    Bn, P = props.shape[:2]
    boxes = np.ascontiguousarray(props[:, :, :4])
    valid = (np.arange(P)[None] < counts[:, None]).astype(np.uint8)
    ra, rm = TR.assign_max_iou(boxes, gt, gt_counts, 0.5, 0.5, 0.5, True, valid)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ga, gm = T.assign_max_iou(cuda(boxes), cuda(gt), cuda(gt_counts), 0.5, 0.5, 0.5, True, cuda(valid))
    _same(ga, ra, "assigned")
    _same(gm, rm, "max_overlaps")
    assert (ra[2] > 0).sum() > 100 and (ra == 0).sum(1).min() > 900 and ((rm > 0) & (rm < 0.1) & (ra == 0)).sum() > 50
    seen = set()
    for keys in (None, TC.caller_keys(Bn, P, 9)):
        kd = None if keys is None else cuda(keys)
        for ft, ff, nb in SETTINGS:
            for num, frac, ub in ((512, 0.25, -1), (64, 0.25, 3), (8192, 0.5, -1)):
                ref = R.sample_assigned_iou_balanced(ra, rm, num, frac, ub, ft, ff, nb, keys, 123)
                runs = [T.sample_assigned_iou_balanced(ga, gm, num, frac, ub, ft, ff, nb, kd, 123) for _ in range(2)]
                for r, g0, g1, nm in zip(ref, runs[0], runs[1], ("pos_mask", "neg_mask", "num_pos", "num_neg")):
                    _same(g0, r, "%s %s" % (nm, (ft, ff, nb, num, frac, ub, keys is None)))
                    assert torch.equal(g0, g1)
                seen.add(bytes(ref[1][2].tobytes()))
        # the positives and the counts are sample_assigned's
        rnd = T.sample_assigned(ga, 512, 0.25, -1, kd, 123)
        bal = T.sample_assigned_iou_balanced(ga, gm, 512, 0.25, -1, -1.0, 0.0, 3, kd, 123)
        assert torch.equal(rnd[0], bal[0]) and torch.equal(rnd[2], bal[2]) and torch.equal(rnd[3], bal[3])
        assert not torch.equal(rnd[1], bal[1])
    assert len(seen) >= 10                                 # the settings choose differently


def _check_sample_rois_balanced(T, props, counts, gt, labels, gt_counts, **kw):
    bal = {k: kw.pop(k) for k in ("floor_thr", "floor_fraction", "num_bins")}
    ref = R.sample_rois_iou_balanced(props.cpu().numpy(), counts.cpu().numpy(), gt, labels, gt_counts, **kw, **bal)
    dk = dict(kw)
    if dk.get("keys") is not None:
        dk["keys"] = torch.from_numpy(dk["keys"]).cuda()
    args = (props, counts, torch.from_numpy(gt).cuda(), torch.from_numpy(labels).cuda(),
            torch.from_numpy(np.asarray(gt_counts, np.int32)).cuda())
    runs = [T.sample_rois(*args, neg_sampler="iou_balanced", **dk, **bal) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    got = [g.cpu().numpy() for g in runs[0]]
    for k in (6, 7, 0, 1, 2, 4, 5):
        _same(got[k], ref[k], NAMES[k])
    rows = np.nonzero(ref[4][:, 0])[0]
    num = kw.get("num", 512)
    g = gt[rows // num, ref[5][rows]]
    TT._compare_targets(got[3], ref[3], None, None, (rows, ref[0][rows, 1:], g), kw.get("target_means", (0, 0, 0, 0)),
                        kw.get("target_stds", (0.1, 0.1, 0.2, 0.2)), "sample_rois iou_balanced")
    return got, ref


@pytest.mark.parametrize("own_keys", [False, True])
def test_sample_rois_iou_balanced_vs_oracle(T, own_keys):
    props, counts, gt, labels, gt_counts = _candidates(seed=1)
    G = gt.shape[1]
    pd, cd = torch.from_numpy(props).cuda(), torch.from_numpy(counts).cuda()
    for i, (ft, ff, nb) in enumerate(SETTINGS):
        keys = TC.caller_keys(3, props.shape[1] + (G if i % 3 else 0), 4) if own_keys else None
        got, ref = _check_sample_rois_balanced(T, pd, cd, gt, labels, gt_counts, num=512, keys=keys, seed=5,
                                               neg_pos_ub=(-1, 3)[i % 2], pos_fraction=0.25, floor_thr=ft,
                                               floor_fraction=ff, num_bins=nb, add_gt_as_proposals=bool(i % 3))
        assert got[7].min() > 0 and got[6][0] == 0


def test_sample_rois_iou_balanced_on_rpn_proposals_then_roi_align(T):
    props, counts = TT._rpn_output(T, 2)
    c = counts.cpu().numpy()
    gt, labels = TT._roi_gts(props.cpu().numpy(), c, 40, (40, 3), 3)
    num = 512
    got, ref = _check_sample_rois_balanced(T, props, counts, gt, labels, (40, 3), num=num, seed=5, pos_fraction=0.25,
                                           floor_thr=-1.0, floor_fraction=0.0, num_bins=3)
    rois = got[0]
    feats = [torch.randn(2, 64, h, w, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
             for h, w in ((200, 336), (100, 168), (50, 84), (25, 42))]
    out = T.roi_align(feats, torch.from_numpy(rois).cuda(), 7, [4, 8, 16, 32]).float().cpu().numpy()
    assert out.shape[0] == 2 * num and np.all(out[rois[:, 0] == -1] == 0) and np.any(out[rois[:, 0] >= 0] != 0)


def test_random_sampler_spelled_out_gives_todays_outputs(T):
    props, counts, gt, labels, gt_counts = _candidates(seed=2)
    args = [torch.from_numpy(a).cuda() for a in (props, counts, gt, labels, gt_counts)]
    ref = TR.sample_rois(props, counts, gt, labels, gt_counts, num=512, seed=7, neg_pos_ub=3)
    a = T.sample_rois(*args, num=512, seed=7, neg_pos_ub=3)
    b = T.sample_rois(*args, num=512, seed=7, neg_pos_ub=3, neg_sampler="random", floor_thr=0.1, floor_fraction=0.25,
                      num_bins=5)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y), NAMES[k]
    for k in (6, 7, 0, 1, 2, 4, 5):
        _same(b[k], ref[k], NAMES[k])


def test_sampler_graph_replay_on_new_ground_truths(T):
    props, counts, gt, labels, gt_counts = _candidates(seed=3)
    pd, cd, gd, ld, gc = [torch.from_numpy(a).cuda() for a in (props, counts, gt, labels, gt_counts)]
    kw = dict(num=512, seed=9, neg_sampler="iou_balanced", floor_thr=0.1, floor_fraction=0.25, num_bins=3)
    T.sample_rois(pd, cd, gd, ld, gc, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = T.sample_rois(pd, cd, gd, ld, gc, **kw)
    seen = []
    for seed in (4, 5):
        new = _candidates(seed=seed)
        gd.copy_(torch.from_numpy(new[2]))
        graph.replay()
        eager = T.sample_rois(pd, cd, gd, ld, gc, **kw)
        for a, b in zip(held, eager):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b)
        seen.append(held[0].clone())
    assert not torch.equal(seen[0], seen[1])


# ---- under the guard ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import libra_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, libra_ops, g)
    return g


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_guarded_balanced_roi(T, guard, dt):
    from torch_detection_amd import libra_ops
    cls, reg, labels, lw, bt, bw = TL.roi_case(1031, 81, True, DTYPES[dt], 5)
    tg = [torch.from_numpy(a).cuda() for a in (labels, lw, bt, bw)]
    cls, reg = guard.guard_copy(cls), guard.guard_copy(reg)
    losses, avg = libra_ops.bbox_head_loss_balanced_fwd(cls, reg, *tg, None, 1.0, 0.5, 1.5)
    gt = torch.tensor((1.0, 1.0), dtype=torch.float32, device="cuda")
    dcls, dreg = libra_ops.bbox_head_loss_balanced_bwd(cls, reg, *tg, gt, avg, 1.0, 0.5, 1.5)
    log = list(guard.ws_log)
    found = guard.check()
    assert not found, "\n".join(found)
    ref = R.bbox_head_loss_balanced(cls.float().cpu().numpy(), reg.float().cpu().numpy(), labels, lw, bt, bw, None)
    TL._check_losses(losses, ref, "guarded balanced")
    assert np.array_equal(_np64(dreg) == 0, ref["dreg"] == 0)
    ENTERED.update(["bbox_head_loss_balanced_fwd", "bbox_head_loss_balanced_bwd"])
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


def test_guarded_balanced_sampler(T, guard):
    from torch_detection_amd import libra_ops
    props, counts, gt, labels, gt_counts = _candidates(seed=6)
    pd, cd, gd, ld, gc = [torch.from_numpy(a).cuda() for a in (props, counts, gt, labels, gt_counts)]
    got = libra_ops.sample_rois_iou_balanced(pd, cd, gd, ld, gc, 0.5, 0.5, 0.5, True, 512, 0.25, -1, True, (0, 0, 0, 0),
                                             (0.1, 0.1, 0.2, 0.2), None, 5, 0.1, 0.25, 3)
    ref = R.sample_rois_iou_balanced(props, counts, gt, labels, gt_counts, num=512, seed=5, floor_thr=0.1,
                                     floor_fraction=0.25, num_bins=3)
    boxes = np.ascontiguousarray(props[:, :, :4])
    valid = (np.arange(props.shape[1])[None] < counts[:, None]).astype(np.uint8)
    ga, gm = T.assign_max_iou(torch.from_numpy(boxes).cuda(), gd, gc, 0.5, 0.5, 0.5, True, torch.from_numpy(valid).cuda())
    masks = libra_ops.sample_assigned_iou_balanced(ga, gm, 512, 0.25, -1, 0.1, 0.25, 3, None, 5)
    log = list(guard.ws_log)
    found = guard.check()
    assert not found, "\n".join(found)
    for k in (6, 7, 0, 1, 2, 4, 5):
        _same(got[k], ref[k], NAMES[k])
    assert int(masks[1].sum()) == int(masks[3].sum())
    ENTERED.update(["sample_rois_iou_balanced", "sample_assigned_iou_balanced"])
    for op, asked, given in log:
        WS_SEEN.setdefault(op, (asked, given))


def test_every_libra_loss_entry_point_ran_under_the_guard():
    """Counts what the guarded tests above did IN THIS RUN (run the file as a whole): the public wrappers of libra_ops.py
    that serve the sampler and the losses (tests/test_gpu_bfp.py has the neck's) returned under the guard, with the
    workspaces at their exact size."""
    from torch_detection_amd import libra_ops
    public = sorted(n for n, v in vars(libra_ops).items()
                    if inspect.isfunction(v) and v.__module__ == libra_ops.__name__ and not n.startswith(("_", "bfp_")))
    assert public == ["bbox_head_loss_balanced_bwd", "bbox_head_loss_balanced_fwd", "sample_assigned_iou_balanced",
                      "sample_rois_iou_balanced"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    for op in ("bbox_head_loss_balanced_fwd", "sample_rois_iou_balanced"):
        asked, given = WS_SEEN[op]
        assert 0 <= given - asked < 256 and asked > 0, (op, asked, given)
