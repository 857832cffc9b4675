"""GPU: every weight-gradient plan of tests/wgrad_cases.py — tile shape, kernel variant, split layout, direct or slab —
forced on a tiny member, asserted on ``ops.wgrad_group_plan`` BEFORE the launch, and checked element by element against
the fp64 oracle of tests/wgrad_ref.py: dw, dgamma and dbeta within their a-priori allowances (``uniform`` operands) or
bit-equal to the oracle (``integers`` operands, where no fp32 summation order can round).  No outlier fraction, no
element excluded.  A failure names the worst element, the split whose pixels explain the error, and the tile.

test_gpu_guarded.py runs the same cases under poisoned, guard-banded outputs and a NaN-filled exact-size workspace.
"""
import pytest
import torch

import wgrad_cases as WC
import wgrad_ref as R

pytestmark = pytest.mark.gpu

# every switch the planner reads: a case runs with exactly its own
PLANNER_KNOBS = ("TDN_WGRAD9", "TDN_WGRAD9_64", "TDN_WGRAD9_TMIN", "TDN_WGRAD_TMIN", "TDN_WGRAD_SHAPE", "TDN_WGRAD_S256",
                 "TDN_WGRAD_S256F", "TDN_WGRAD_S128", "TDN_WGRAD_S64", "TDN_WGRAD_UNIFORM", "TDN_WGRAD_DIRECT",
                 "TDN_WGRAD_DMIN", "TDN_WGRAD_DMAX", "TDN_WGRAD_T", "TDN_WGRAD9_STAGGER")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from torch_detection_amd import ops as _ops
    from torch_detection_amd import _lib
    _lib.load()
    return _ops


def _nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def _vec(t):
    return None if t is None else t.cuda()


def _device_call(ops, m, o, dtype, as_item):
    """Stage one member's operands and either launch it through its own entry point or return its group item.
    Returns (item or None, (dw, dgamma, dbeta), tensors to keep alive)."""
    bn = (_vec(o.scale), _vec(o.mean), _vec(o.invstd))
    kw = {}
    if o.prev is not None:
        pdw = o.prev[0] if m.kind == "stem" else o.prev[0].permute(0, 2, 3, 1)
        kw = dict(dw=pdw.contiguous().cuda(), dgamma=_vec(o.prev[1]), dbeta=_vec(o.prev[2]), beta=1.0)
    g = _nhwc(o.g, dtype)
    if m.kind == "stem":
        xp = ops.stage_image(o.x.cuda(), dtype)
        ws = ops.pack_stem_weight(o.w.cuda(), dtype)
        args, keep = (xp, g, ws, (m.H, m.W)) + bn, (xp, g, ws, bn)
        fn = ops.stem_conv_wgrad_item if as_item else ops.stem_conv_wgrad
    elif m.kind == "gconv":
        x = _nhwc(o.x, dtype)
        wf, _ = ops.pack_gconv_weight(o.w.cuda(), m.groups, None, False, dtype)
        args, keep = (x, g, wf, m.groups, m.k, m.stride, m.pad) + bn, (x, g, wf, bn)
        fn = ops.gconv2d_wgrad_item if as_item else ops.gconv2d_wgrad
    else:
        x = _nhwc(o.x, dtype)
        wf = _nhwc(o.w, dtype)                                     # OIHW -> [O][kh][kw][I]
        args, keep = (x, g, wf, m.k, m.stride, m.pad) + bn, (x, g, wf, bn)
        fn = ops.conv2d_wgrad_item if as_item else ops.conv2d_wgrad
    out = fn(*args, **kw)
    if as_item:
        return out[0], out[1:], keep
    return None, out, keep


def _oihw(m, dw):
    dw = dw.float().cpu()
    return dw if m.kind == "stem" else dw.permute(0, 3, 1, 2)


def run_case(ops, case, monkeypatch, records=None):
    """Knobs -> plan predicate -> launch -> element-wise check, once per generator the case runs.  Appends
    (member, generator, plan row, check records) to ``records``; raises AssertionError with the explained worst
    element of every failed output."""
    for k in PLANNER_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.knobs.items():
        monkeypatch.setenv(k, str(v))
    dtype = WC.DTYPES[case.dtype]
    per, _ = ops.wgrad_group_plan(WC.shape_only_items(case), dtype)
    problems = WC.plan_problems(case, per)
    assert not problems, "%s no longer exercises its plan:\n%s" % (case.id, "\n".join(problems))

    refs = []
    for i, m in enumerate(case.members):
        args = (dtype, case.bn[i], case.accumulate, case.seed + i)
        uni = R.cached_reference(m, "uniform", *args)
        gens = R.generators(m, *args, ref_uniform=uni)
        refs.append({g: (uni if g == "uniform" else R.cached_reference(m, g, *args)) for g in gens})
    gens = [g for g in ("integers", "uniform") if any(g in r for r in refs)]
    assert gens, case.id
    failures = []
    for gen in gens:
        rs = [r[gen] if gen in r else R.cached_reference(m, gen, dtype, case.bn[i], case.accumulate, case.seed + i)
              for i, (m, r) in enumerate(zip(case.members, refs))]
        group = len(case.members) > 1
        items, results, keep = [], [], []
        for m, ref in zip(case.members, rs):
            it, res, kp = _device_call(ops, m, ref.o, dtype, group)
            items.append(it)
            results.append(res)
            keep.append(kp)
        if group:
            # the launch must be planned exactly as the shape-only query was
            assert ops.wgrad_group_plan(items, dtype)[0] == per, case.id
            ops.wgrad_group(items, dtype, torch.device("cuda"))
        torch.cuda.synchronize()
        for i, (m, ref, (dw, dg, db)) in enumerate(zip(case.members, rs, results)):
            assert (dg is not None) == ref.bn, (case.id, i)
            recs = R.check_member(ref, _oihw(m, dw), None if dg is None else dg.float().cpu(), db.float().cpu(),
                                  "%s member %d (%s, %s)" % (case.id, i, m.kind, gen))
            if records is not None:
                records.append((i, gen, per[i], recs))
            failures += [R.explain(ref, r, per[i]) for r in recs if r["bad"]]
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_wgrad_plan_case(ops, case, monkeypatch):
    run_case(ops, case, monkeypatch)
