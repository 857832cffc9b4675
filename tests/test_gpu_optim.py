"""GPU tests of the fused SGD step (torch_detection_amd.SGD, optim_ops.py, csrc/optim.hip) against the
numpy reference tests/optim_ref.py: parameters, momentum buffers and the state bit for bit on all three access paths,
the clip, the non-finite skip and the loss-scale state machine, untouched gradients, run-to-run reproducibility, graph
capture with a learning-rate schedule, every entry point of optim_ops.py under guard-banded, poisoned allocations with
exact-size workspaces (tests/guard_util.py), a ResNet-18 step end to end with a gradient reducer, and checkpoints."""
import inspect

import numpy as np
import pytest
import torch

import guard_util as G
import optim_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
ENTERED, WS_SEEN = set(), {}        # what ran under the guard in this run (checked by the last test of the file)
L, TR, GEN = 0, 1, 2                 # _lib.SGD_PATH_*

SIZES_1D = [1, 63, 64, 65, 4095, 4096, 4097]
CONVS = [(64, 64, 3, 3), (5, 7, 3, 3), (2, 130, 3, 3), (64, 3, 7, 7), (3, 512, 3, 3)]   # the last: taps x Cin > one chunk
GROUPS3 = [dict(lr=0.05, weight_decay=1e-4, momentum=0.9), dict(lr=0.013, weight_decay=0.0, momentum=0.8),
           dict(lr=0.02, weight_decay=3e-3, momentum=0.0)]


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def _bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---- cases: (shape, layout) lists turned into device tensors -----------------------------------------------------------
def spec_all(many=0):
    """(shape, layout, expected path): 1-D sizes, conv weights as reducer pairs and with one layout, a channels_last
    parameter with a contiguous gradient, a pair of misaligned slices, and ``many`` small extra items."""
    spec = [((n,), "same", L) for n in SIZES_1D]
    spec += [(s, "reducer", TR) for s in CONVS] + [(s, "same", L) for s in CONVS[:4]]
    spec += [((6, 10, 3, 3), "channels_last", GEN), ((4097,), "misaligned", L), ((64, 64, 1, 1), "reducer", L)]
    spec += [((1 + (7 * i) % 97,), "same", L) for i in range(many)]
    return spec


def make(spec, seed, alloc=None, alloc_in=None):
    """-> (params, grads, numpy params).  ``alloc(shape)`` gives a contiguous float32 device tensor for a parameter,
    ``alloc_in`` for a gradient (default: torch.empty); layouts are views of those."""
    rng = np.random.default_rng(seed)
    new = alloc or (lambda shape: torch.empty(shape, dtype=torch.float32, device="cuda"))
    new_in = alloc_in or new
    ps, gs, nps = [], [], []
    for shape, layout, _ in spec:
        val = rng.standard_normal(shape).astype(F32)
        if layout == "misaligned":
            p = new((shape[0] + 1,))[1:]
            g = new_in((shape[0] + 3,))[3:]
        elif layout == "channels_last":
            O, I, kh, kw = shape
            p = new((O, kh, kw, I)).permute(0, 3, 1, 2)
            g = new_in(shape)
        elif layout == "reducer":
            O, I, kh, kw = shape
            p = new(shape)
            g = new_in((O, kh, kw, I)).permute(0, 3, 1, 2)
        else:
            p, g = new(shape), new_in(shape)
        p.copy_(torch.from_numpy(val))
        g.zero_()
        ps.append(p)
        gs.append(g)
        nps.append(val)
    return ps, gs, nps


def grads_for(spec, seed, step, scale=0.3):
    rng = np.random.default_rng(1000 * seed + step)
    out = [(rng.standard_normal(shape) * scale).astype(F32) for shape, _, _ in spec]
    if step == 0:
        for g in out:
            g.reshape(-1)[::3] = -0.0          # the first step copies: the sign must reach the buffer
    return out


def load_grads(gs, vals):
    for g, v in zip(gs, vals):
        g.copy_(torch.from_numpy(v))


def group_lists(n, groups):
    return [dict(g, params=list(range(k, n, len(groups)))) for k, g in enumerate(groups)]


def build(T, spec, seed, groups, alloc=None, alloc_in=None, **kw):
    ps, gs, nps = make(spec, seed, alloc, alloc_in)
    for p, g in zip(ps, gs):
        p.grad = g
    gl = group_lists(len(ps), groups)
    opt = T.SGD([dict(params=[ps[i] for i in g["params"]], lr=g["lr"], weight_decay=g["weight_decay"],
                      momentum=g["momentum"]) for g in gl], lr=0.1, momentum=0.9, **kw)
    ref_kw = dict(nesterov=kw.get("nesterov", False), max_norm=kw.get("max_norm"),
                  skip_nonfinite=kw.get("skip_nonfinite", True))
    ls = kw.get("loss_scale")
    if ls == "dynamic":
        ref_kw.update(dynamic=True, scale=kw.get("init_scale", 512.0), growth=kw.get("growth_factor", 2.0),
                      backoff=kw.get("backoff_factor", 0.5), interval=kw.get("growth_interval", 2000))
    elif ls is not None:
        ref_kw.update(scale=ls)
    ref = R.RefSGD(nps, gl, **ref_kw)
    return opt, ref, ps, gs, gl


def norm_ok(opt, ref_grads, scale):
    """grad_norm within 2 fp32 ulp of the float64 value: the double accumulation leaves ~2^-50 relative, the one
    rounding to fp32 2^-24, and one ulp of slack."""
    want = np.sqrt(np.float64(R.grad_sumsq(ref_grads))) * np.float64(F32(1.0) / F32(scale))
    got = float(opt.grad_norm.item())
    assert abs(got - want) <= 2 * float(np.spacing(F32(want))), (got, want)


def check_all(opt, ref, ps, gl, what=""):
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert _same(p, ref.params[i]), "%s parameter %d %s" % (what, i, tuple(p.shape))
    for g in gl:
        for i in g["params"]:
            if g["momentum"] != 0:
                assert _same(opt.state[ps[i]]["momentum_buffer"], ref.bufs[i]), "%s buffer %d" % (what, i)
            else:
                assert "momentum_buffer" not in opt.state[ps[i]]
    assert _same(opt.loss_scale, ref.scale)
    got = [int(t.item()) for t in (opt.growth_tracker, opt.steps_taken, opt.steps_skipped, opt.last_skipped)]
    assert got == [ref.tracker, ref.taken, ref.skipped, ref.last_skipped], (what, got)


# ---- 1. bitwise, every path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "nesterov"])
def test_bitwise_vs_reference_on_every_path(T, variant):
    spec = spec_all(many=300 if variant == "plain" else 0)
    groups = GROUPS3 if variant == "plain" else GROUPS3[:2]
    opt, ref, ps, gs, gl = build(T, spec, 3, groups, nesterov=variant == "nesterov")
    for step in range(5):
        vals = grads_for(spec, 3, step)
        load_grads(gs, vals)
        opt.step()
        ref.step(vals)
        assert float(opt.clip_coef.item()) == 1.0
        norm_ok(opt, vals, 1.0)
        check_all(opt, ref, ps, gl, "step %d" % step)
        assert all(_same(g, v) for g, v in zip(gs, vals)), "a gradient was written"
    assert len(ps) > 300 or variant != "plain"
    assert opt._plan.paths == [spec[i][2] for g in gl for i in g["params"]]      # items come group by group
    assert {L, TR, GEN} == set(opt._plan.paths)
    assert opt._plan.n == len(spec) and opt._plan.update_chunks > opt._plan.n
    # the buffers are views of ONE allocation
    lo, hi = opt._flats[0].data_ptr(), opt._flats[0].data_ptr() + 4 * opt._flats[0].numel()
    assert len(opt._flats) == 1
    assert all(lo <= st["momentum_buffer"].data_ptr() < hi for st in opt.state.values() if "momentum_buffer" in st)


# ---- 2. clip ----------------------------------------------------------------------------------------------------------
def test_clip(T):
    spec = spec_all()
    base, base_ref, bps, bgs, gl = build(T, spec, 4, GROUPS3[:2])
    loose, _, lps, lgs, _ = build(T, spec, 4, GROUPS3[:2], max_norm=1e6)
    tight, ref, tps, tgs, _ = build(T, spec, 4, GROUPS3[:2], max_norm=0.5)
    for step in range(3):
        vals = grads_for(spec, 4, step)
        for opt, gs in ((base, bgs), (loose, lgs), (tight, tgs)):
            load_grads(gs, vals)
            opt.step()
        n, c = F32(tight.grad_norm.item()), F32(tight.clip_coef.item())
        norm_ok(tight, vals, 1.0)
        assert n > 0.5 and c < 1 and _same(c, F32(0.5) / (n + F32(1e-6)))       # clip_grad_norm_'s formula, in fp32
        assert float(loose.clip_coef.item()) == 1.0 and _same(loose.grad_norm, n)
        ref.step(vals, coef=c)                               # fed the reported coefficient: bitwise
        base_ref.step(vals)
        check_all(tight, ref, tps, gl, "clipped step %d" % step)
        check_all(loose, base_ref, lps, gl, "loose step %d" % step)
        check_all(base, base_ref, bps, gl, "no clip step %d" % step)
        assert all(_same(g, v) for g, v in zip(tgs, vals)), "the clip wrote a gradient"
    assert not all(_same(a, b) for a, b in zip(tps, bps))


# ---- 3. non-finite gradients, the loss scale ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["inf_last", "nan_first"])
def test_nonfinite_step_is_skipped_and_the_scale_follows(T, where):
    spec = spec_all()
    opt, ref, ps, gs, gl = build(T, spec, 5, GROUPS3[:2], loss_scale="dynamic", init_scale=512.0, growth_interval=2)
    seq = [0, 0, 1, 1, 0, 0, 0]
    scales = []
    for step, bad in enumerate(seq):
        vals = grads_for(spec, 5, step, scale=30.0)
        if bad and where == "inf_last":
            vals[-1].reshape(-1)[-1] = np.inf
        elif bad:
            vals[0].reshape(-1)[0] = np.nan
        load_grads(gs, vals)
        before = [p.clone() for p in ps] + [opt.state[p]["momentum_buffer"].clone() for p in ps] if bad else None
        first = ps[0].clone()
        opt.step()
        ref.step(vals)
        check_all(opt, ref, ps, gl, "step %d" % step)
        scales.append(float(opt.loss_scale.item()))
        after = ps + [opt.state[p]["momentum_buffer"] for p in ps]
        if bad:
            assert all(_same(a, b) for a, b in zip(after, before)) and int(opt.last_skipped.item()) == 1
        else:
            assert not _same(after[0], first) and int(opt.last_skipped.item()) == 0
            norm_ok(opt, vals, scales[-2] if step else 512.0)
    assert scales == [512.0, 1024.0, 512.0, 256.0, 256.0, 512.0, 512.0]
    assert int(opt.steps_taken.item()) == 5 and int(opt.steps_skipped.item()) == 2


def test_nonfinite_step_is_taken_on_request(T):
    spec = spec_all()[:9]
    opt, ref, ps, gs, gl = build(T, spec, 6, GROUPS3[:2], skip_nonfinite=False, loss_scale=8.0)
    for step in range(2):
        vals = grads_for(spec, 6, step)
        if step == 1:
            vals[-1].reshape(-1)[-1] = np.inf
        load_grads(gs, vals)
        opt.step()
        ref.step(vals)
    torch.cuda.synchronize()
    assert int(opt.steps_taken.item()) == 2 and int(opt.steps_skipped.item()) == 0 and float(opt.loss_scale.item()) == 8.0
    for i, p in enumerate(ps):
        assert np.array_equal(p.cpu().numpy(), ref.params[i], equal_nan=True)
    assert not np.isfinite(ps[-1].cpu().numpy()).all() and np.isfinite(ps[0].cpu().numpy()).all()


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------
def _partials(opt):
    off = opt._ws_ptr.value - opt._ws.data_ptr()
    return opt._ws[off:off + 8 * opt._plan.norm_chunks].view(torch.float64).clone()


def test_two_fresh_runs_give_identical_bits(T):
    spec = spec_all(many=40)
    runs = []
    for _ in range(2):
        opt, _, ps, gs, _ = build(T, spec, 7, GROUPS3, max_norm=0.5, loss_scale="dynamic", growth_interval=2)
        for step in range(3):
            load_grads(gs, grads_for(spec, 7, step))
            opt.step()
        torch.cuda.synchronize()
        bufs = [opt.state[p]["momentum_buffer"] for p in ps if "momentum_buffer" in opt.state[p]]
        runs.append([_bits(t) for t in ps + bufs + [opt._fstate]] + [opt._istate.cpu().numpy(),
                                                                      _partials(opt).cpu().numpy().view(np.int64)])
    assert len(runs[0]) == len(runs[1]) and all(np.array_equal(a, b) for a, b in zip(*runs))
    assert runs[0][-1].size == opt._plan.norm_chunks > len(spec)


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------
def test_captured_step_replays_with_a_schedule(T, monkeypatch):
    """The capture holds the two launches, on one stream: a linear chain with no parallel branches.  The learning rate
    changes between replays through sync_hyper() alone."""
    spec = spec_all()
    lrs = [0.05, 0.04, 0.03, 0.02]
    results = []
    for graphed in (False, True):
        opt, _, ps, gs, _ = build(T, spec, 8, GROUPS3[:2], max_norm=0.5)
        graph = None
        for step, lr in enumerate(lrs):
            load_grads(gs, grads_for(spec, 8, step))
            opt.param_groups[0]["lr"] = lr
            if not graphed or step == 0:
                opt.step()
                if graphed:
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    versions = [p._version for p in ps]
                    with torch.cuda.graph(graph):
                        opt.step()
                    assert [p._version for p in ps] == versions      # nothing but the two launches inside a capture
            else:
                opt.sync_hyper()
                graph.replay()
        torch.cuda.synchronize()
        assert int(opt.steps_taken.item()) == len(lrs)
        results.append([_bits(p) for p in ps] + [_bits(opt.state[p]["momentum_buffer"]) for p in ps])
    assert all(np.array_equal(a, b) for a, b in zip(*results))
    # a step that would have to rebuild its table inside a capture says so (the capture state is faked: no launch)
    fresh, _, _, _, _ = build(T, spec[:3], 8, GROUPS3[:1])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="rebuilt during a graph capture"):
        fresh.step()
    ps[0].grad = ps[0].grad.clone()
    with pytest.raises(RuntimeError, match="rebuilt during a graph capture"):
        opt.step()
    with pytest.raises(RuntimeError, match="inside a graph capture"):
        opt.param_groups[0]["lr"] = 0.5
        opt.sync_hyper()


# ---- 7. under the guard --------------------------------------------------------------------------------------------------
@pytest.fixture()
def guard(monkeypatch):
    from torch_detection_amd import optim_ops
    g = G.GuardAlloc()
    G.install(monkeypatch, optim_ops, g)
    yield g
    torch.cuda.synchronize()


@pytest.mark.parametrize("nesterov", [False, True])
def test_guarded_step(T, guard, nesterov):
    """Parameters and gradients in guard bands (NaN bands: a stray read poisons the result), the state arrays, the
    momentum buffers, the table and the workspace allocated by optim_ops under the guard — the workspace at exactly the
    planned size and filled with NaN bytes, so a partial read before it was written would make S a NaN and skip the step."""
    spec = spec_all()
    mk = lambda label: (lambda shape: guard.alloc(shape, torch.float32, "cuda", interior="zero", label=label,
                                                  band_byte=G.NAN_BYTE))
    groups = GROUPS3[:2] if nesterov else GROUPS3
    opt, ref, ps, gs, gl = build(T, spec, 9, groups, alloc=mk("parameter"), alloc_in=mk("gradient"), nesterov=nesterov,
                                 max_norm=0.5, loss_scale="dynamic", growth_interval=2)
    for step in range(3):
        vals = grads_for(spec, 9, step)
        load_grads(gs, vals)
        opt.step()
        c = F32(opt.clip_coef.item())
        ref.step(vals, coef=c)
        check_all(opt, ref, ps, gl, "guarded step %d" % step)
    assert int(opt.steps_taken.item()) == 3
    log = list(guard.ws_log)
    found = guard.check()
    assert not found, "\n".join(found)
    asked = sorted(a for op, a, given in log if op == "sgd_upload")
    assert asked == sorted([opt._plan.table_bytes, opt._plan.workspace_bytes]) and all(a == g for _, a, g in log)
    assert opt._ws.numel() == opt._plan.workspace_bytes and opt._table.numel() == opt._plan.table_bytes
    for op in ("sgd_state", "sgd_momentum"):
        assert guard.calls[op] >= 1
    ENTERED.update(["sgd_item", "sgd_plan", "sgd_state", "sgd_momentum", "sgd_upload", "sgd_step"])
    for op, a, given in log:
        WS_SEEN.setdefault(op, (a, given))


# ---- 8. end to end ---------------------------------------------------------------------------------------------------
def _resnet18(T, sd=None):
    from golden_util import fill_state_dict
    m = T.ResNet(18)
    m.load_state_dict(sd if sd is not None else fill_state_dict(m.state_dict(), 50))
    return m.cuda().train()


def _param_groups(m):
    """Conv weights decay, norm parameters do not (mmdetection's norm_decay_mult = 0)."""
    dims = [p.dim() for p in m.parameters()]
    w = [i for i, d in enumerate(dims) if d == 4]
    rest = [i for i, d in enumerate(dims) if d != 4]
    return [dict(lr=0.02, weight_decay=1e-4, momentum=0.9, params=w),
            dict(lr=0.02, weight_decay=0.0, momentum=0.9, params=rest)]


def _grads(params):
    return [p.grad.cpu().numpy() if p.grad is not None else None for p in params]


@pytest.mark.parametrize("weights", ["as_built", "contiguous"])
def test_resnet18_step_with_a_reducer_end_to_end(T, weights):
    """``as_built``: the layers keep 3x3 weights channels_last, which is the reducer's gradient layout (linear path);
    ``contiguous``: OIHW weights, as a model gets them when its weights are assigned from elsewhere — the reducer's
    gradient views are then permuted against them (transposed path)."""
    from golden_util import det_tensor
    from torch_detection_amd import dp
    m = _resnet18(T)
    params = list(m.parameters())
    if weights == "contiguous":
        for p in params:
            p.data = p.data.contiguous()
    gl = _param_groups(m)
    assert gl[0]["params"] and gl[1]["params"]
    x = det_tensor((1, 3, 64, 64), 700, -2, 2).cuda()
    red = dp.attach_reducer([m])
    opt = T.SGD([dict(params=[params[i] for i in g["params"]], weight_decay=g["weight_decay"]) for g in gl], lr=0.02,
                momentum=0.9, max_norm=35.0)
    ref = R.RefSGD([p.detach().cpu().numpy() for p in params], gl, max_norm=35.0)
    cots = None

    def fwd_bwd():
        nonlocal cots
        outs = m(x)
        if cots is None:
            cots = [det_tensor(tuple(o.shape), 710 + i, -1, 1).cuda().to(o.dtype) for i, o in enumerate(outs)]
        torch.autograd.backward(outs, cots)
        red.finish()

    def fresh_forward():
        sd = m.state_dict()
        for (n, _), v in zip(m.named_parameters(), ref.params):
            sd[n] = torch.from_numpy(v.copy())
        with torch.no_grad():
            return [o.clone() for o in _resnet18(T, sd)(x)]

    for step in range(2):
        fwd_bwd()
        opt.step()
        torch.cuda.synchronize()
        grads = _grads(params)
        ref.step(grads, coef=F32(opt.clip_coef.item()))
        for i, p in enumerate(params):
            assert _same(p, ref.params[i]), (step, i)
        # the next forward runs on the updated weights: the version bump made every unit repack
        with torch.no_grad():
            got = [o.clone() for o in m(x)]
        want = fresh_forward()
        assert all(torch.equal(a, b) for a, b in zip(got, want)), step
    permuted = any(p.grad is not None and p.grad.stride() != p.stride() for p in params)
    assert L in opt._plan.paths and GEN not in opt._plan.paths
    assert (TR in opt._plan.paths) == permuted == (weights == "contiguous")

    # the same step as launch plans: with the optimizer inside, the plan holds exactly its two launches more
    def with_step():
        fwd_bwd()
        opt.step()

    bare = T.PreparedStep(fwd_bwd, modules=(m,))
    assert bare.prepared, bare.error
    n_bare = bare.stats()[0]
    bare.close()
    ps = T.PreparedStep(with_step, modules=(m,))         # two eager warm-up steps, then the recorded one
    assert ps.prepared, ps.error
    assert ps.stats()[0] == n_bare + 2
    torch.cuda.synchronize()
    # three more steps were taken while the plan was made; the reference goes on from the device's state
    ref.params = [p.detach().cpu().numpy().copy() for p in params]
    ref.bufs = [opt.state[p]["momentum_buffer"].cpu().numpy().copy() if "momentum_buffer" in opt.state[p]
                else np.zeros(tuple(p.shape), F32) for p in params]
    ps()                                                  # replay: forward, backward and the update on the device
    torch.cuda.synchronize()
    ref.step(_grads(params), coef=F32(opt.clip_coef.item()))
    for i, p in enumerate(params):
        assert _same(p, ref.params[i]), ("replay", i)
    assert int(opt.steps_taken.item()) == 2 + 3 + 1
    ps.close()


# ---- 9. checkpoints ---------------------------------------------------------------------------------------------------
def test_state_dict_round_trips_with_torch_sgd(T, tmp_path):
    spec = [((4097,), "same", L), ((5, 7, 3, 3), "reducer", TR), ((6, 10, 3, 3), "channels_last", GEN), ((64,), "same", L)]
    groups = GROUPS3[:2]
    # torch -> ours: two steps of torch.optim.SGD, its state loaded here, two more steps == the reference continuing
    # from torch's parameters and buffers
    ps, gs, _ = make(spec, 10)
    for p, g in zip(ps, gs):
        p.grad = g
    gl = group_lists(len(ps), groups)
    tgroups = lambda: [dict(params=[ps[i] for i in g["params"]], lr=g["lr"], weight_decay=g["weight_decay"],
                            momentum=g["momentum"]) for g in gl]
    topt = torch.optim.SGD(tgroups(), lr=0.1, momentum=0.9, foreach=False)
    for step in range(2):
        load_grads(gs, grads_for(spec, 10, step))
        topt.step()
    opt = T.SGD(tgroups(), lr=0.1, momentum=0.9)
    opt.load_state_dict(topt.state_dict())
    ref = R.RefSGD([p.cpu().numpy() for p in ps], gl)
    ref.bufs = [topt.state[p]["momentum_buffer"].cpu().numpy().copy() for p in ps]
    ref.buf_init = True
    for step in range(2, 4):
        vals = grads_for(spec, 10, step)
        load_grads(gs, vals)
        opt.step()
        ref.step(vals)
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert _same(p, ref.params[i]) and _same(opt.state[p]["momentum_buffer"], ref.bufs[i]), i
    # ours -> a checkpoint file -> ours: continuing equals the uninterrupted run; ours -> torch: buffers and groups arrive
    from torch_detection_amd import checkpoint
    holder = torch.nn.Module()
    path = str(tmp_path / "ckpt.pth")
    checkpoint.save_checkpoint(holder, path, optimizer=opt)
    sd = torch.load(path, weights_only=True)["optimizer"]
    ps2 = [p.clone() for p in ps]
    for p, g in zip(ps2, gs):
        p.grad = g
    groups2 = [dict(params=[ps2[i] for i in g["params"]], lr=0.5, weight_decay=0.5, momentum=0.5) for g in gl]
    opt2 = T.SGD(groups2, lr=0.1, momentum=0.9, loss_scale="dynamic")
    opt2.load_state_dict(sd)
    assert [g["lr"] for g in opt2.param_groups] == [g["lr"] for g in groups]
    t2 = torch.optim.SGD([dict(params=[p.clone() for p in g["params"]]) for g in groups2], lr=0.5, momentum=0.5)
    t2.load_state_dict(opt.state_dict())
    for g_t, g_o in zip(t2.param_groups, opt.param_groups):
        assert (g_t["lr"], g_t["momentum"], g_t["weight_decay"]) == (g_o["lr"], g_o["momentum"], g_o["weight_decay"])
        for pt, po in zip(g_t["params"], g_o["params"]):
            assert torch.equal(t2.state[pt]["momentum_buffer"], opt.state[po]["momentum_buffer"])
    vals = grads_for(spec, 10, 4)
    load_grads(gs, vals)
    opt.step()
    opt2.step()
    torch.cuda.synchronize()
    for a, b in zip(ps, ps2):
        assert _same(a, b) and _same(opt.state[a]["momentum_buffer"], opt2.state[b]["momentum_buffer"])
    assert int(opt2.steps_taken.item()) == 3 and float(opt2.loss_scale.item()) == 1.0


def test_every_optim_entry_point_ran_under_the_guard():
    """Counts what the guarded tests above did IN THIS RUN (run the file as a whole): every public wrapper of
    optim_ops.py returned under the guard, and the table and the workspace were handed out at exactly the planned sizes."""
    from torch_detection_amd import optim_ops
    public = sorted(n for n, v in vars(optim_ops).items()
                    if inspect.isfunction(v) and v.__module__ == optim_ops.__name__ and not n.startswith("_"))
    assert public == ["sgd_item", "sgd_momentum", "sgd_plan", "sgd_state", "sgd_step", "sgd_upload"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
    asked, given = WS_SEEN["sgd_upload"]
    assert asked == given and asked > 0 and asked % 256 == 0, (asked, given)
