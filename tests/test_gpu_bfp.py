"""GPU: the Balanced Feature Pyramid kernels (csrc/bfp.hip) through the wrappers of libra_ops.py, bit for bit
against the NumPy oracle tests/bfp_ref.py — forward outputs and all gradients, bf16 and fp16 — under guard-banded, poisoned
allocations (tests/guard_util.py); the BFP module behind FPN against the fp32 torch CPU composition with the tolerances
tests/test_gpu_models.py applies to the necks (test_fpn_vs_golden: outputs 6e-3, input and parameter gradients 1e-2,
relative l2); graph replay on new inputs.  Every call runs twice and must give the same bits.

Input values come from a handful of 16-bit values, so ties are everywhere; channel 0 of image 0 is all negative with the
maximum of nearly every window in its last element, channel 1 is constant (bfp_ref.planted).  The map handed to the
scatter and the cotangent handed to the gather's adjoint are either the kernels' own results (``refine_type=None``) or
other tied maps, standing for what a refine conv and its input gradient would hand over."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bfp_ref as R
import guard_util as G
from golden_util import det_tensor, fill_state_dict, rel_l2

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
ENTERED = set()             # the wrappers that returned under the guard in this run (checked by the last test of the file)

# name -> (B, C, [(H, W)], refine levels)
CASES = {
    "halving": (2, 64, [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)], (0, 2, 4)),
    "fp32-nearest": (1, 8, [(10, 164), (5, 82), (3, 41), (2, 2)], (1,)),
    "overlap": (3, 72, [(25, 42), (13, 21), (7, 11)], (1, 2)),
    "single": (2, 8, [(5, 7)], (0,)),
    "one-pixel": (1, 16, [(4, 6), (1, 1)], (0, 1)),
    "wide": (1, 256, [(8, 12), (4, 6), (2, 3)], (1,)),
}


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    from torch_detection_amd import libra_ops
    return libra_ops


@pytest.fixture()
def guard(monkeypatch, P):
    g = G.GuardAlloc()
    G.install(monkeypatch, P, g)
    return g


_REF = {}


def reference(name, r, dt, own):
    """The oracle's results for a case, computed once and shared (read only)."""
    key = (name, r, dt, own)
    if key not in _REF:
        B, C, sizes, _ = CASES[name]
        rnd = R.quant(dt)
        xs = R.planted([R.tied((B, C) + s, 11 + i) for i, s in enumerate(sizes)])
        gs = [R.tied((B, C) + s, 31 + i) for i, s in enumerate(sizes)]
        bsf, ga = R.gather_fwd(xs, r, rnd)
        refined = bsf if own else R.planted([R.tied(bsf.shape, 51)])[0]
        outs, sa = R.scatter_fwd(xs, refined, r, rnd)
        dref = R.scatter_bwd(gs, sa, sizes[r], rnd)
        dbsf = dref if own else R.tied(bsf.shape, 52)
        dxs = R.gather_bwd(gs, ga, dbsf, rnd)
        _REF[key] = dict(xs=xs, gs=gs, bsf=bsf, refined=refined, outs=outs, dref=dref, dbsf=dbsf, dxs=dxs)
    return _REF[key]


def dev(a, dt, guard=None):
    """NCHW array of dt-representable values -> logical NCHW device tensor in channels_last memory (a guarded copy with NaN
    bands under the guard)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).permute(0, 2, 3, 1).contiguous().to(dt).cuda()
    if guard is not None:
        t = guard.guard_copy(t)
    return t.permute(0, 3, 1, 2)


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def equals(t, ref, dt, what):
    """device tensor (logical NCHW, channels_last memory, dtype dt) == the oracle's array, bit for bit"""
    assert t.dtype == dt and tuple(t.shape) == ref.shape and t.permute(0, 2, 3, 1).is_contiguous(), what
    want = torch.from_numpy(ref).to(dt)
    got = t.detach().cpu().contiguous()
    bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert len(bad) == 0, "%s: %d of %d elements differ, first at %s: got %r, want %r" % (
        what, len(bad), want.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def twice(fn):
    a, b = fn(), fn()
    for s, t in zip(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b]):
        assert same_bits(s, t)
    return a


def run(P, guard, name, r, dt, own):
    ref = reference(name, r, dt, own)
    tag = "%s refine_level=%d %s %s" % (name, r, dt, "own" if own else "given")
    xd = [dev(x, dt, guard) for x in ref["xs"]]
    gd = [dev(g, dt, guard) for g in ref["gs"]]
    bsf = twice(lambda: P.bfp_gather_fwd(xd, r))
    equals(bsf, ref["bsf"], dt, tag + ": bsf")
    refined = bsf if own else dev(ref["refined"], dt, guard)
    outs = twice(lambda: P.bfp_scatter_fwd(xd, refined, r))
    for l, o in enumerate(outs):
        equals(o, ref["outs"][l], dt, tag + ": out %d" % l)
    dref = twice(lambda: P.bfp_scatter_bwd(gd, refined, r))
    equals(dref, ref["dref"], dt, tag + ": d bsf'")
    dbsf = dref if own else dev(ref["dbsf"], dt, guard)
    dxs = twice(lambda: P.bfp_gather_bwd(xd, gd, dbsf, r))
    for l, d in enumerate(dxs):
        equals(d, ref["dxs"][l], dt, tag + ": dx %d" % l)
    if guard is not None:
        found = guard.check()
        assert not found, "\n".join(found)
        assert not guard.ws_log, guard.ws_log                                  # no workspace
        for op in ("bfp_gather_fwd", "bfp_scatter_fwd", "bfp_scatter_bwd", "bfp_gather_bwd"):
            assert guard.calls[op] >= 2, (op, dict(guard.calls))               # every output came from the guard
            ENTERED.add(op)


def _id(v):
    return "bf16" if v is BF else "fp16" if v is FP else str(v)


@pytest.mark.parametrize("dt", [BF, FP], ids=_id)
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_oracle_bit_for_bit_under_the_guard(P, guard, name, dt):
    for r in CASES[name][3]:
        run(P, guard, name, r, dt, True)
    run(P, guard, name, CASES[name][3][-1], dt, False)


def test_the_cases_hold_what_they_are_for():
    """The fp32 nearest rule at destination 41 both ways, overlapping windows both ways, a one-pixel level, windows that
    are all negative with the maximum last."""
    assert R.nearest_src(2, 82)[41] == 0                                          # level 3 -> refine level 1, and back
    assert CASES["fp32-nearest"][2][3] == (2, 2) and CASES["fp32-nearest"][2][1] == (5, 82)
    w = R.pool_windows(25, 13)
    assert any(a[1] > b[0] for a, b in zip(w, w[1:]))
    w = R.pool_windows(21, 11)
    assert any(a[1] > b[0] for a, b in zip(w, w[1:]))
    ref = reference("halving", 2, BF, True)
    assert all((x[0, 0] < 0).all() for x in ref["xs"]) and (ref["bsf"][0, 0] < 0).all()
    _, arg = R.resize("pool", ref["xs"][0], (4, 6))
    assert ((arg[0, 0, :, :, 0] % 4 == 3) & (arg[0, 0, :, :, 1] % 4 == 3)).mean() > 0.9
    assert (ref["xs"][0][:, 1] == 0.25).all()


def test_one_level_doubles_its_input(P):
    x = R.tied((2, 8, 5, 7), 5)
    xd = dev(x, BF)
    bsf = P.bfp_gather_fwd([xd], 0)
    assert same_bits(bsf, xd)
    out = P.bfp_scatter_fwd([xd], bsf, 0)[0]
    assert same_bits(out, (xd.float() * 2).to(BF))


# ---- module level ---------------------------------------------------------------------------------------------------------
def _torch_bfp(xs, r, weight=None, bias=None):
    size = xs[r].shape[2:]
    feats = [F.adaptive_max_pool2d(x, output_size=size) if l < r else F.interpolate(x, size=size, mode="nearest")
             for l, x in enumerate(xs)]
    bsf = sum(feats) / len(feats)
    if weight is not None:
        bsf = F.relu(F.conv2d(bsf, weight, bias, padding=1))
    return [(F.interpolate(bsf, size=x.shape[2:], mode="nearest") if l < r else
             F.adaptive_max_pool2d(bsf, output_size=x.shape[2:])) + x for l, x in enumerate(xs)]


@pytest.mark.parametrize("refine_type", [None, "conv"], ids=["plain", "conv"])
def test_bfp_behind_fpn_against_the_torch_composition(refine_type):
    """FPN on the feature maps of a 64 x 96 image batch, then BFP(256, 5, 2): outputs, input gradients and the refine conv's
    parameter gradients against torch's CPU ops in fp32 on the FPN's own (16-bit) outputs."""
    import torch_detection_amd as T
    chans, sizes = [64, 128, 256, 512], [(16, 24), (8, 12), (4, 6), (2, 3)]
    fpn = T.FPN(chans, 256, 5)
    fpn.load_state_dict(fill_state_dict(fpn.state_dict(), 910))
    fpn.cuda()
    bfp = T.NECKS.build(dict(type="BFP", in_channels=256, num_levels=5, refine_level=2, refine_type=refine_type))
    sd = fill_state_dict(bfp.state_dict(), 920)
    bfp.load_state_dict(sd)
    bfp.cuda()
    ins = [det_tensor((2, c, h, w), 930 + i, -1, 1).cuda() for i, (c, (h, w)) in enumerate(zip(chans, sizes))]
    with torch.no_grad():
        feats = fpn(ins)
    assert [tuple(f.shape[2:]) for f in feats] == sizes + [(1, 2)]
    leaves = [f.detach().requires_grad_(True) for f in feats]
    cots = [det_tensor(tuple(f.shape), 940 + i, -1, 1) for i, f in enumerate(feats)]

    def both():
        for t in leaves:
            t.grad = None
        bfp.zero_grad()
        outs = bfp(leaves)
        torch.autograd.backward(outs, [c.cuda().to(o.dtype) for c, o in zip(cots, outs)])
        return list(outs) + [t.grad for t in leaves] + [p.grad for p in bfp.parameters()]

    first, second = both(), both()
    assert all(same_bits(a, b) for a, b in zip(first, second))
    outs, dins = first[:5], first[5:10]
    for o, f in zip(outs, feats):
        assert o.dtype == f.dtype and o.shape == f.shape and o.permute(0, 2, 3, 1).is_contiguous()
    for d, f in zip(dins, feats):
        assert d.dtype == f.dtype and d.shape == f.shape
    rin = [f.detach().float().cpu().requires_grad_(True) for f in feats]
    ps = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    routs = _torch_bfp(rin, 2, ps.get("refine.conv.weight"), ps.get("refine.conv.bias"))
    torch.autograd.backward(routs, cots)
    eo = [rel_l2(o.float().cpu(), r_) for o, r_ in zip(outs, routs)]
    ei = [rel_l2(d.float().cpu(), r_.grad) for d, r_ in zip(dins, rin)]
    eg = {k: rel_l2(p.grad.float().cpu(), ps[k].grad) for k, p in bfp.named_parameters()}
    print("bfp %s: out %s din %s grads %s" % (refine_type, eo, ei, eg))
    # test_gpu_models.py's neck tolerances: outputs 6e-3 (test_fpn_vs_golden); gradients 1e-2 for a neck without an
    # activation (test_fpn_vs_golden) and 2.5e-1 for one with ReLU (test_pafpn_vs_golden), where the masks of tiny maps
    # flip on a visible fraction of elements between a 16-bit and an fp32 evaluation.  The conv case is then compared a
    # second time with the masks and the arg-maxima taken from the device's own 16-bit maps, at the tight tolerance.
    assert max(eo) <= 6e-3, eo
    tol = 1e-2 if refine_type is None else 2.5e-1
    assert max(ei) <= tol, ei
    assert not eg or max(eg.values()) <= tol, eg
    assert (refine_type == "conv") == bool(eg)
    if refine_type != "conv":
        return
    from torch_detection_amd import libra_ops
    with torch.no_grad():
        bsf_d = libra_ops.bfp_gather_fwd(list(feats), 2)
        refined_d = bfp.refine(bsf_d)
    xs = [f.detach().float().cpu().numpy() for f in feats]
    gs = [c.numpy() for c in cots]
    host = lambda t: t.detach().float().cpu().contiguous()
    _, ga = R.gather_fwd(xs, 2)
    _, sa = R.scatter_fwd(xs, host(refined_d).numpy(), 2)
    dref = torch.from_numpy(R.scatter_bwd(gs, sa, sizes[2])) * (host(refined_d) > 0)
    leaf = host(bsf_d).requires_grad_(True)
    w, b = (sd[k].clone().requires_grad_(True) for k in ("refine.conv.weight", "refine.conv.bias"))
    F.conv2d(leaf, w, b, padding=1).backward(dref)
    rdx = R.gather_bwd(gs, ga, leaf.grad.numpy())
    ei = [rel_l2(host(d), torch.from_numpy(r_)) for d, r_ in zip(dins, rdx)]
    eg = {"refine.conv.weight": rel_l2(host(bfp.refine.conv.weight.grad), w.grad),
          "refine.conv.bias": rel_l2(host(bfp.refine.conv.bias.grad), b.grad)}
    print("bfp conv, masks and arg-maxima of the device's maps: din %s grads %s" % (ei, eg))
    assert max(ei) <= 1e-2, ei
    assert max(eg.values()) <= 1e-2, eg


def test_one_level_with_the_refine_conv():
    """num_levels = 1: out = x + refine(x)"""
    import torch_detection_amd as T
    bfp = T.BFP(64, 1, 0, "conv")
    sd = fill_state_dict(bfp.state_dict(), 950)
    bfp.load_state_dict(sd)
    bfp.cuda()
    x = det_tensor((2, 64, 6, 10), 951, -1, 1)
    out = bfp([x.cuda().to(BF).contiguous(memory_format=torch.channels_last)])[0]
    ref = x + F.relu(F.conv2d(x, sd["refine.conv.weight"], sd["refine.conv.bias"], padding=1))
    assert rel_l2(out.float().cpu(), ref) <= 6e-3


@pytest.mark.parametrize("norm", ["GN", "BN"])
def test_bfp_with_a_normalised_refine_conv(norm):
    """``norm_cfg``: the refine unit is conv (no bias) -> GroupNorm(32) / BatchNorm2d (batch statistics) -> ReLU.  Outputs,
    input gradients and the gradients of ``refine.conv.weight`` / ``refine.norm.*`` against the same modules of torch in
    fp32 on the CPU, at test_gpu_models.py's tolerances for normalised necks: outputs 1.5e-2 (its GN FPN), gradients
    behind a ReLU 2.5e-1 (test_pafpn_vs_golden)."""
    import torch_detection_amd as T
    cfg = dict(type="GN", num_groups=32) if norm == "GN" else dict(type="BN")
    sizes = [(12, 16), (6, 8), (3, 4)]
    bfp = T.BFP(64, 3, 1, "conv", norm_cfg=cfg)
    sd = fill_state_dict(bfp.state_dict(), 960)
    bfp.load_state_dict(sd)
    bfp.cuda().train()
    assert sorted(n for n, _ in bfp.named_parameters()) == ["refine.conv.weight", "refine.norm.bias", "refine.norm.weight"]
    xs = [det_tensor((2, 64) + s, 961 + i, -1, 1) for i, s in enumerate(sizes)]
    cots = [det_tensor((2, 64) + s, 971 + i, -1, 1) for i, s in enumerate(sizes)]
    leaves = [x.cuda().to(BF).contiguous(memory_format=torch.channels_last).requires_grad_(True) for x in xs]

    def both():
        for t in leaves:
            t.grad = None
        bfp.zero_grad()
        outs = bfp(leaves)
        torch.autograd.backward(outs, [c.cuda().to(BF) for c in cots])
        return list(outs) + [t.grad for t in leaves] + [p.grad for _, p in sorted(bfp.named_parameters())]

    first = both()
    if norm == "GN":                                       # BatchNorm's running statistics move between two calls
        assert all(same_bits(a, b) for a, b in zip(first, both()))
    conv = torch.nn.Conv2d(64, 64, 3, padding=1, bias=False)
    nrm = torch.nn.GroupNorm(32, 64) if norm == "GN" else torch.nn.BatchNorm2d(64)
    conv.weight.data.copy_(sd["refine.conv.weight"])
    nrm.weight.data.copy_(sd["refine.norm.weight"])
    nrm.bias.data.copy_(sd["refine.norm.bias"])
    nrm.train()
    rin = [x.clone().requires_grad_(True) for x in xs]
    size = sizes[1]
    feats = [F.adaptive_max_pool2d(rin[0], size), F.interpolate(rin[1], size=size, mode="nearest"),
             F.interpolate(rin[2], size=size, mode="nearest")]
    bsf = F.relu(nrm(conv(sum(feats) / 3)))
    routs = [F.interpolate(bsf, size=sizes[0], mode="nearest") + rin[0], F.adaptive_max_pool2d(bsf, sizes[1]) + rin[1],
             F.adaptive_max_pool2d(bsf, sizes[2]) + rin[2]]
    torch.autograd.backward(routs, cots)
    eo = [rel_l2(o.float().cpu(), r_) for o, r_ in zip(first[:3], routs)]
    ei = [rel_l2(d.float().cpu(), r_.grad) for d, r_ in zip(first[3:6], rin)]
    eg = [rel_l2(g.float().cpu(), r_.grad) for g, r_ in zip(first[6:], (conv.weight, nrm.bias, nrm.weight))]
    print("bfp conv + %s: out %s din %s grads (conv.weight, norm.bias, norm.weight) %s" % (norm, eo, ei, eg))
    assert all(bool(torch.isfinite(t.float()).all()) for t in first)
    assert max(eo) <= 1.5e-2, eo
    assert max(ei) <= 2.5e-1, ei
    assert max(eg) <= 2.5e-1, eg


# ---- graph capture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, FP], ids=_id)
def test_graph_replays_on_new_inputs_equal_eager(P, dt):
    B, C, sizes, _ = CASES["overlap"]
    r = 1
    xd = [dev(R.tied((B, C) + s, 61 + i), dt) for i, s in enumerate(sizes)]
    gd = [dev(R.tied((B, C) + s, 71 + i), dt) for i, s in enumerate(sizes)]

    def all_four():
        bsf = P.bfp_gather_fwd(xd, r)
        outs = P.bfp_scatter_fwd(xd, bsf, r)
        dref = P.bfp_scatter_bwd(gd, bsf, r)
        return [bsf] + outs + [dref] + P.bfp_gather_bwd(xd, gd, dref, r)

    all_four()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = all_four()
    for k in (1, 2):
        for i, s in enumerate(sizes):                                              # new inputs in the captured buffers
            xd[i].copy_(dev(R.tied((B, C) + s, 100 * k + i), dt))
            gd[i].copy_(dev(R.tied((B, C) + s, 100 * k + 10 + i), dt))
        graph.replay()
        eager = all_four()
        assert all(same_bits(a, b) for a, b in zip(eager, held)), k


def test_refusals_launch_nothing(P):
    z = lambda C, H=4, W=4, B=1, dt=BF: torch.zeros(B, H, W, C, dtype=dt, device="cuda").permute(0, 3, 1, 2)
    with pytest.raises(ValueError, match="multiple of 8"):
        P.bfp_gather_fwd([z(12)], 0)
    with pytest.raises(ValueError, match="refine_level"):
        P.bfp_scatter_fwd([z(8)], z(8), 1)
    with pytest.raises(ValueError, match="bsf"):
        P.bfp_scatter_bwd([z(8), z(8, 2, 2)], z(8, 2, 2), 0)
    with pytest.raises(ValueError, match="dbsf"):
        P.bfp_gather_bwd([z(8), z(8, 2, 2)], [z(8), z(8, 2, 2)], z(8, 2, 2), 0)
    with pytest.raises(ValueError, match="gs"):
        P.bfp_gather_bwd([z(8), z(8, 2, 2)], [z(8)], z(8), 0)
    # the library's own checks answer the same way when the wrapper is bypassed
    from torch_detection_amd import _lib
    arr = (_lib.BfpLevel * 1)()
    arr[0].H, arr[0].W = 4, 0
    assert _lib.load().tdn_bfp_gather_fwd(arr, 1, 0, 1, 8, None, 0, None) != 0
    assert b"out of 1..32767" in _lib.load().tdn_last_error()


def test_every_bfp_entry_point_ran_under_the_guard(P):
    """Counts what the guarded tests above did IN THIS RUN (run the file as a whole): every public wrapper of libra_ops.py
    that serves the BFP neck returned under the guard."""
    public = sorted(n for n, v in vars(P).items()
                    if inspect.isfunction(v) and v.__module__ == P.__name__ and n.startswith("bfp_"))
    assert public == ["bfp_gather_bwd", "bfp_gather_fwd", "bfp_scatter_bwd", "bfp_scatter_fwd"]
    assert set(public) <= ENTERED, sorted(set(public) - ENTERED)
