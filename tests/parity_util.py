"""Teacher-forced parity check of the HIP ResNet+FPN schedule against oracle/sched_ref.py (test infrastructure).

Deep bf16 pipelines cannot be compared end to end at rounding accuracy: a 1e-6 difference in fp32 accumulation
order flips a few bf16 roundings, each flip perturbs the next layer's roundings, and after a handful of layers
two bit-different-but-equally-valid implementations sit a full quantisation-noise apart (~1e-2 forward); through
~50 ReLU masks the gradients then differ by tens of percent.  So the comparison is made *in situ*:

  forward   every fused launch is recomputed on CPU from the GPU's own input tensors of that launch;
  backward  the CPU schedule is given the GPU's saved activations (identical ReLU masks / pool indices) and
            runs the whole backward itself; bf16 rounding noise of the activation-gradients then only adds up
            linearly (~sqrt(#layers) * 2^-9), while any routing / indexing / epilogue bug is O(1).
"""
import os

import torch
import torch.nn.functional as F

import bound_util as B
from golden_util import det_tensor, fill_state_dict, rel_l2


def nchw(t):
    return t.detach().float().cpu().permute(0, 3, 1, 2).contiguous()


class Elementwise(object):
    """Worst elementwise ratio |got - v| / allowance (tests/bound_util.py) per launch kind, with the element it
    occurred at.  ``cheap``: the full-size form — v from the oracle's own fp32 convolution (its error term added to the
    allowance) and the Cauchy-Schwarz bound for S; otherwise fp64 v and the exact S."""

    def __init__(self, cheap, dtype):
        self.cheap, self.dtype = cheap, dtype
        self.rec = {}

    def put(self, kind, r):
        if kind not in self.rec or r["ratio"] > self.rec[kind]["ratio"]:
            self.rec[kind] = r

    def fwd(self, kind, name, ref_u, gu, x, got, addend=None, mode=None, relu=False, extra=None):
        """One forward launch: the oracle unit's 16-bit weights, the GPU unit's own fp32 scale / shift vectors (the
        operands of the launch).  Returns (bound, the oracle's fp32 conv for its own fwd(conv=) or None)."""
        pin_fold(name, ref_u, gu)
        conv = ref_u.conv(x) if self.cheap else None
        b = B.fwd_bound(x, ref_u.wb, ref_u.stride, ref_u.pad, gu.scale, gu.shift, addend, mode, relu,
                        cheap=self.cheap, conv32=conv)
        if got is not None:
            self.put(kind, B.check(got, b, self.dtype, extra, name))
        return b, conv

    def result(self):
        out = dict(self.rec)
        out["mode"] = ("fp32 reference + its K*2^-24*S term, Cauchy-Schwarz S" if self.cheap else "fp64 reference, exact S")
        return out


FOLD_RTOL = 2.0 ** -19     # scale = gamma / sqrt(var + eps): four rounded fp32 operations on either side (2^-24 each)
                           # and a reciprocal square root good to two ulps on the GPU: under 2^-20; one bit of margin


def pin_fold(name, ref_u, gu):
    """The launch's own fp32 scale / shift vectors (the elementwise checks take them as operands) against the oracle's
    fold: a bias is the parameter itself, bit for bit; a BN fold agrees to FOLD_RTOL, the shift = beta - mean * scale
    relative to |beta| + |mean * scale|."""
    if ref_u.scale is None:
        assert gu.scale is None, name
        assert (gu.shift is None) == (ref_u.shift is None), name
        if ref_u.shift is not None:
            assert torch.equal(gu.shift.detach().float().cpu(), ref_u.shift), name + ": bias"
        return
    sc, sh = gu.scale.detach().double().cpu(), gu.shift.detach().double().cpu()
    rs, rh = ref_u.scale.double(), ref_u.shift.double()
    assert bool(((sc - rs).abs() <= FOLD_RTOL * rs.abs()).all()), name + ": folded scale"
    ms = (ref_u.mean.double() * rs).abs()
    assert bool(((sh - rh).abs() <= FOLD_RTOL * ((rh.abs() + ms) + ms)).all()), name + ": folded shift"


def pin_dgrad_weights(name, w_eff, ref_u, dtype):
    """The launch's packed dgrad operand against the oracle's 16-bit(scale * 16-bit(w)): the scale may differ by
    FOLD_RTOL and the product is rounded once more, so the two lie within one ulp16 of each other."""
    d = (w_eff.double() - ref_u.wd.double()).abs()
    assert bool((d <= 2.0 * B.half_ulp16(ref_u.wd, dtype)).all()), name + ": packed dgrad weights"


ELEMENTWISE_GATED = ("stem", "block_conv1", "block_conv2", "block_conv3", "block_residual_downsample", "block_last_basic",
                     "fpn_lateral", "fpn_lateral_up2x", "fpn_out", "dgrad")


def gpu_units(rb, rf, launches):
    """conv name -> the HIP path's ConvUnit, from the recorded backward launches (every conv has a weight gradient)."""
    names = {}
    for prefix, mod in (("backbone.", rb), ("neck.", rf)):
        for name, m in mod.named_modules():
            if isinstance(m, torch.nn.Conv2d):
                names[id(m)] = prefix + name
    return {names[id(rec[1].conv)]: rec[1] for rec in launches}


def run_teacher_forced(T, depth, shape, dev="cuda", threads=None, dtype=torch.bfloat16, cot_scale=1.0,
                       res_gain=1.0, end_to_end=True, cheap_bound=False):
    """Returns a dict of measured relative-L2 errors (forward in situ, backward teacher-forced, and the plain
    end-to-end distances to the fp32 autograd oracle for the record) and, under "elementwise", the worst ratio of every
    launch kind against the a-priori rounding bound of tests/bound_util.py (``cheap_bound``: its full-size form)."""
    from oracle import sched_ref as S
    from oracle import torch_ref as O
    from torch_detection_amd import functional as HF
    torch.set_num_threads(threads or min(16, os.cpu_count() or 1))
    chans = [64, 128, 256, 512] if depth < 50 else [256, 512, 1024, 2048]
    rb, rf = T.ResNet(depth), T.FPN(chans, 256, 5)
    sdb = fill_state_dict(rb.state_dict(), 50)
    sdf = fill_state_dict(rf.state_dict(), 51)
    if res_gain != 1.0:   # damp every residual branch (its last BN's gamma): keeps a deep net inside fp16's range
        last_bn = "bn2.weight" if depth < 50 else "bn3.weight"
        for k in sdb:
            if k.endswith(last_bn):
                sdb[k] = sdb[k] * res_gain
    rb.load_state_dict(sdb)
    rf.load_state_dict(sdf)
    rb.to(dev).train()
    rf.to(dev)
    rb.compute_dtype = rf.compute_dtype = dtype   # bf16 (default) or fp16 operands; parameters stay fp32
    x = det_tensor(shape, 700, -2, 2)
    cap = {}
    bwd_launches = []
    HF.DEBUG_CAPTURE = cap
    try:
        outs = rf(rb(x.to(dev)))
    finally:
        HF.DEBUG_CAPTURE = None
    # cot_scale: the loss scale of an fp16 run (a power of two, so the cotangents stay exactly representable)
    cots = [det_tensor(tuple(o.shape), 710 + i, -1, 1) * cot_scale for i, o in enumerate(outs)]
    HF.DEBUG_BWD = bwd_launches
    try:
        torch.autograd.backward(outs, [c.to(dev).to(o.dtype) for c, o in zip(cots, outs)])
        torch.cuda.synchronize()
    finally:
        HF.DEBUG_BWD = None
    assert all(o.dtype == dtype for o in outs), [o.dtype for o in outs]
    got = {}
    for prefix, mod in (("backbone.", rb), ("neck.", rf)):
        for k, p in mod.named_parameters():
            assert p.grad is not None, k
            got[prefix + k] = p.grad.detach().float().cpu()
    st, saved = cap["seq"]
    xs, lat = cap["fpn"]
    g_s = nchw(st["s"])
    g_saved = [tuple(nchw(t) if t is not None else None for t in sv) for sv in saved]
    g_lat = [nchw(t) for t in lat]
    g_outs = [o.detach().float().cpu() for o in outs]

    sch = S.Sched(sdb, sdf, depth, 5, quant=dtype)
    fwd = {}
    # ---- forward, launch by launch, from the GPU's own inputs ----
    gu = gpu_units(rb, rf, bwd_launches)
    el = Elementwise(cheap_bound, dtype)
    xq = S.rnd(x, dtype)
    _, cv = el.fwd("stem", "backbone.conv1", sch.stem, gu["backbone.conv1"], xq, g_s, relu=True)
    fwd["stem"] = rel_l2(g_s, sch.stem.fwd(xq, relu=True, conv=cv))
    # exact operations (selections of already-rounded values): the max pool of the GPU's own stem output, and P6
    fwd["maxpool"] = rel_l2(g_saved[0][0], F.max_pool2d(g_s, 3, 2, 1))
    exact = {"maxpool": bool(torch.equal(g_saved[0][0], F.max_pool2d(g_s, 3, 2, 1))),
             "p6": bool(torch.equal(g_outs[4], g_outs[3][:, :, ::2, ::2]))}
    worst_blk = 0.0
    for blk, (bx, h1, h2, out) in zip(sch.blocks, g_saved):
        pre = "backbone.%s." % blk.p
        _, cv = el.fwd("block_conv1", pre + "conv1", blk.u1, gu[pre + "conv1"], bx, h1, relu=True)
        worst_blk = max(worst_blk, rel_l2(h1, blk.u1.fwd(bx, relu=True, conv=cv)))
        res, res_e, extra = bx, bx, None
        if blk.ud is not None:   # not saved by the HIP path: one launch deep on CPU
            # the elementwise check takes the residual from the same bound it derives the operand slack from (the
            # GPU's own scale / shift): the GPU's 16-bit residual is within E (+ R) + one ulp16 of it
            bd, cv = el.fwd(None, pre + "downsample.0", blk.ud, gu[pre + "downsample.0"], bx, None)
            res = blk.ud.fwd(bx, conv=cv)
            res_e = S.rnd(bd.v.float(), dtype)
            extra = B.operand_slack(bd, dtype)
            del bd
        last = "conv3" if blk.kind == "bottleneck" else "conv2"
        if blk.kind == "bottleneck":
            _, cv = el.fwd("block_conv2", pre + "conv2", blk.u2, gu[pre + "conv2"], h1, h2, relu=True)
            worst_blk = max(worst_blk, rel_l2(h2, blk.u2.fwd(h1, relu=True, conv=cv)))
            kind = "block_conv3" if blk.ud is None else "block_residual_downsample"
            _, cv = el.fwd(kind, pre + last, blk.u3, gu[pre + last], h2, out, res_e, "same", True, extra)
            worst_blk = max(worst_blk, rel_l2(out, blk.u3.fwd(h2, res, "same", True, conv=cv)))
        else:
            kind = "block_last_basic" if blk.ud is None else "block_residual_downsample"
            _, cv = el.fwd(kind, pre + last, blk.u2, gu[pre + last], h1, out, res_e, "same", True, extra)
            worst_blk = max(worst_blk, rel_l2(out, blk.u2.fwd(h1, res, "same", True, conv=cv)))
    fwd["blocks_worst"] = worst_blk
    feats = [g_saved[i][3] for i in sch.stage_last]
    worst = 0.0
    for i in reversed(range(4)):
        name = "neck.lateral_convs.%d.conv" % i
        if i == 3:
            _, cv = el.fwd("fpn_lateral", name, sch.lat_u[i], gu[name], feats[i], g_lat[i])
            ref = sch.lat_u[i].fwd(feats[i], conv=cv)
        else:
            _, cv = el.fwd("fpn_lateral_up2x", name, sch.lat_u[i], gu[name], feats[i], g_lat[i], g_lat[i + 1], "up2x")
            ref = sch.lat_u[i].fwd(feats[i], g_lat[i + 1], "up2x", conv=cv)
        worst = max(worst, rel_l2(g_lat[i], ref))
    for i in range(4):
        name = "neck.fpn_convs.%d.conv" % i
        _, cv = el.fwd("fpn_out", name, sch.fpn_u[i], gu[name], g_lat[i], g_outs[i])
        worst = max(worst, rel_l2(g_outs[i], sch.fpn_u[i].fwd(g_lat[i], conv=cv)))
    worst = max(worst, rel_l2(g_outs[4], g_outs[3][:, :, ::2, ::2]))
    fwd["fpn_worst"] = worst
    del cv
    # ---- backward, launch by launch, from the GPU's own operands of that launch ----
    bwd = backward_in_situ(sch, rb, rf, bwd_launches, xq, cheap=cheap_bound)
    elem = el.result()
    elem.update({k: v for k, v in bwd.pop("elementwise").items() if k != "mode"})
    # ---- backward with the GPU's saved activations ----
    sch.x = S.rnd(x, dtype)
    sch.out_shapes = [tuple(o.shape) for o in g_outs]
    sch.load_saved(g_s, g_saved, g_lat)
    ref_grads = sch.backward(cots)
    assert set(ref_grads) == set(got)
    eg = {k: rel_l2(got[k], ref_grads[k]) for k in got}
    srt = sorted(eg.values())
    worst_g = max(eg.items(), key=lambda kv: kv[1])
    # ---- for the record: end-to-end distance to the fp32 autograd oracle (== the reference's arithmetic) ----
    if end_to_end:
        ref_outs, ref32 = O.resnet_fpn_fwd_bwd(sdb, sdf, x, depth, cots)
        eo32 = [rel_l2(a, b) for a, b in zip(g_outs, ref_outs)]
        eg32 = sorted(rel_l2(got[k], ref32[k]) for k in got)
    else:   # full-size runs skip the fp32 autograd pass of the whole net (the in-situ checks are the point there)
        eo32, eg32 = [0.0], [0.0]
    return {"forward_in_situ": fwd,
            "forward_exact": exact,
            "elementwise": elem,
            "backward_in_situ": bwd,
            "backward_teacher_forced": {"grad_worst": list(worst_g), "grad_median": srt[len(srt) // 2]},
            "end_to_end_vs_fp32_autograd": {"out": eo32, "grad_median": eg32[len(eg32) // 2],
                                            "grad_worst": eg32[-1]}}


def backward_in_situ(sch, rb, rf, launches, x_img, cheap=False):
    """Every dgrad launch and every weight-gradient member of the GPU's backward pass, recomputed on the CPU by the
    schedule oracle's unit of the same layer from the GPU's OWN operands of that launch (the activation gradient g it
    read, the addend / ReLU-mask tensors of its epilogue, the saved forward input).  Identical inputs on both sides:
    what is left is one layer's arithmetic — fp32 accumulation order and one rounding to the 16-bit storage type —
    so the per-launch bound is the north star's 1e-3, for every layer, at any depth.
    Returns the worst relative-L2 error per kind and where it occurred; under "elementwise" the worst ratio against
    the a-priori rounding bound (tests/bound_util.py) of the dgrad launches — computed on the launch's own packed
    dgrad weights — and of dw (recorded; a gate only where the caller makes it one: at full size K = N * Ho * Wo makes
    the worst-case bound looser than a typical element)."""
    from torch_detection_amd import ops
    units = {}
    conv_name = {}
    for prefix, mod in (("backbone.", rb), ("neck.", rf)):
        for name, m in mod.named_modules():
            if isinstance(m, torch.nn.Conv2d):
                conv_name[id(m)] = prefix + name
    units["backbone.conv1"] = sch.stem
    for blk in sch.blocks:
        units["backbone.%s.conv1" % blk.p] = blk.u1
        units["backbone.%s.conv2" % blk.p] = blk.u2
        if blk.u3 is not None:
            units["backbone.%s.conv3" % blk.p] = blk.u3
        if blk.ud is not None:
            units["backbone.%s.downsample.0" % blk.p] = blk.ud
    for i in range(sch.nlat):
        units["neck.lateral_convs.%d.conv" % i] = sch.lat_u[i]
        units["neck.fpn_convs.%d.conv" % i] = sch.fpn_u[i]
    worst = {"dgrad": [0.0, None], "dw": [0.0, None], "dgamma": [0.0, None], "dbeta_or_dbias": [0.0, None]}
    count = {"dgrad": 0, "wgrad": 0}
    dtype = torch.bfloat16 if sch.q is True else sch.q
    el = Elementwise(cheap, dtype)

    def upd(kind, err, name):
        if err > worst[kind][0]:
            worst[kind] = [err, name]

    for rec in launches:
        name = conv_name[id(rec[1].conv)]
        ref_u = units[name]
        if rec[0] == 'dgrad':
            _, u, g, in_hw, addend, mode, mask_src, dx = rec
            a = nchw(addend) if addend is not None and mode != ops.ADD_NONE else None
            gc, mode_s = nchw(g), 'same' if mode == ops.ADD_SAME else 'sumpool'
            msk = nchw(mask_src) if mask_src is not None else None
            # the launch's own dgrad operand [Cin][kh][kw][Cout] (16-bit(scale * 16-bit(w)), packed on the GPU)
            w_eff = u.w_dgrad.detach().float().cpu().permute(3, 0, 1, 2).contiguous()
            pin_dgrad_weights(name, w_eff, ref_u, dtype)
            same_w = torch.equal(w_eff, ref_u.wd)
            cv = ref_u.conv_t(gc, in_hw) if cheap else None
            cv_e = cv if same_w or not cheap else True
            b = B.dgrad_bound(gc, w_eff, in_hw, ref_u.stride, ref_u.pad, a, mode_s if a is not None else None, msk,
                              cheap=cheap, conv32=cv_e)
            el.put("dgrad", B.check(nchw(dx), b, dtype, None, name))
            del b
            ref = ref_u.dgrad(gc, in_hw, a, mode_s, msk, conv=cv)
            upd("dgrad", rel_l2(nchw(dx), ref), name)
            count["dgrad"] += 1
        else:
            _, u, x_in, g, img_hw, (dw, dg, db) = rec
            xin = x_img if u.is_stem else nchw(x_in)
            gc = nchw(g)
            G = torch.nn.grad.conv2d_weight(xin, ref_u.w.shape, gc, ref_u.stride, ref_u.pad)
            b = B.wgrad_bound(xin, gc, ref_u.w.shape, ref_u.stride, ref_u.pad, u.scale, cheap=cheap, G32=G)
            el.put("dw", B.check(dw.detach().float().cpu(), b, torch.float32, None, name))
            del b
            ref = ref_u.wgrad(xin, gc, G=G)
            upd("dw", rel_l2(dw.detach().float().cpu(), ref[0]), name)
            if len(ref) == 3:
                upd("dgamma", rel_l2(dg.float().cpu(), ref[1]), name)
                upd("dbeta_or_dbias", rel_l2(db.float().cpu(), ref[2]), name)
            elif len(ref) == 2:
                upd("dbeta_or_dbias", rel_l2(db.float().cpu(), ref[1]), name)
            count["wgrad"] += 1
    out = {k: v for k, v in worst.items()}
    out["launches"] = count
    out["elementwise"] = el.result()
    return out


# bounds (relative L2); see module docstring
FWD_IN_SITU_TOL = 1e-3      # north-star figure for conv activations, per fused launch on identical inputs
                            # (measured ~3e-5: a ~2e-4 fraction of outputs round to the neighbouring bf16)
BWD_TEACHER_TOL = 6e-2      # every parameter gradient, whole backward, identical saved activations
                            # (measured: R18 ~1e-2, R50 ~2e-2, R101 ~3e-2 worst; medians ~1e-2): rounding noise of the
                            # 16-bit activation-gradients adding up over the depth.  This run checks the ROUTING of the
                            # schedule (a missing residual / FPN / stage gradient is O(1)); the arithmetic of every
                            # launch is bounded separately at 1e-3 on its own operands (backward_in_situ).
BWD_TEACHER_TOL_DEEP = 6e-2  # R101: the same bound since the per-launch backward check exists (was 1.2e-1)
FWD_END_TO_END_TOL = 2e-2   # bf16 activations vs the fp32 reference path (~1e-2 expected)


BWD_IN_SITU_TOL = 1e-3      # every dgrad launch / weight-gradient member on its own operands (fp32 outputs of the
                            # weight gradients: accumulation order only; dgrad: one 16-bit rounding, like the forward)


def check_elementwise(res, weights=False):
    """Every forward and dgrad launch kind: worst |got - v| / allowance <= 1, the failure naming the element; the two
    exact operations bit for bit.  ``weights``: dw too (sizes where K = N * Ho * Wo is a few thousand)."""
    e = res["elementwise"]
    kinds = [k for k in ELEMENTWISE_GATED if k in e]
    assert "stem" in kinds and "dgrad" in kinds and "fpn_out" in kinds and len(kinds) >= 7, kinds
    for k in kinds + (["dw"] if weights else []):
        assert e[k]["ratio"] <= 1.0, k + " / " + B.message(e[k])
    assert "dw" in e
    assert res["forward_exact"] == {"maxpool": True, "p6": True}, res["forward_exact"]


def check(res, depth=50):
    f = res["forward_in_situ"]
    assert max(f.values()) <= FWD_IN_SITU_TOL, f
    check_elementwise(res, weights=True)
    b = res["backward_in_situ"]
    assert b["launches"]["dgrad"] > 0 and b["launches"]["wgrad"] > 0, b
    for kind in ("dgrad", "dw", "dgamma", "dbeta_or_dbias"):
        assert b[kind][0] <= BWD_IN_SITU_TOL, (kind, b[kind])
    tol = BWD_TEACHER_TOL if depth <= 50 else BWD_TEACHER_TOL_DEEP
    assert res["backward_teacher_forced"]["grad_worst"][1] <= tol, res["backward_teacher_forced"]
    assert res["backward_teacher_forced"]["grad_median"] <= 3e-2, res["backward_teacher_forced"]
    assert max(res["end_to_end_vs_fp32_autograd"]["out"]) <= FWD_END_TO_END_TOL, res["end_to_end_vs_fp32_autograd"]
