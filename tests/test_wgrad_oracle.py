"""CPU: the weight-gradient oracle (wgrad_ref.py) against autograd, the sensitivity of its check to the faults a wrong
kernel would make, and every case's plan predicate on the host-only planner (wgrad_cases.py).

Sensitivity: for every case of the table each fault model of wgrad_ref.mutants is applied to the oracle's own result
and handed to ``check_member`` — the function test_gpu_wgrad_plans.py calls on the GPU's output.  The case's check
(all the generators it runs) must reject every fault that can be expressed on the member; a fault is inexpressible
only for a structural reason that is asserted here (no padded tap, a single image, no BN operands).  The unmutated
oracle, rounded to fp32, must pass.  ``python tests/test_wgrad_oracle.py`` prints the table kept in
profiles/wgrad_plan_checks.md.
"""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as WC
import wgrad_ref as R


@contextlib.contextmanager
def knobs(case):
    """The case's planner switches in the environment; every TDN_ variable restored afterwards."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("TDN_")}
    for k in saved:
        del os.environ[k]
    os.environ.update({k: str(v) for k, v in case.knobs.items()})
    try:
        yield
    finally:
        for k in [k for k in os.environ if k.startswith("TDN_")]:
            del os.environ[k]
        os.environ.update(saved)


def plan_of(case):
    from torch_detection_amd import ops
    with knobs(case):
        per, tot = ops.wgrad_group_plan(WC.shape_only_items(case), WC.DTYPES[case.dtype])
    return per, tot


def refs_of(case, i):
    """{generator: Ref} of member ``i`` of a case."""
    m, dt = case.members[i], WC.DTYPES[case.dtype]
    args = (dt, case.bn[i], case.accumulate, case.seed + i)
    uni = R.cached_reference(m, "uniform", *args)
    return {g: (uni if g == "uniform" else R.cached_reference(m, g, *args))
            for g in R.generators(m, *args, ref_uniform=uni)}


# ---- the oracle against autograd ------------------------------------------------------------------------------------------
_GEOMETRIES = sorted({(m, c.dtype) for c in WC.CASES for m in c.members},
                     key=lambda t: (t[0].kind, t[0][1:], t[1]))


@pytest.mark.parametrize("m,dt", _GEOMETRIES, ids=["%s-%s" % ("x".join(str(v) for v in m), dt) for m, dt in _GEOMETRIES])
def test_oracle_matches_autograd(m, dt):
    """dw, dgamma, dbeta of the oracle == fp64 autograd through conv -> batch norm with fixed statistics, and through
    torch.nn.grad.conv2d_weight, on every geometry of the table (stem, grouped, dilated, stride 2 included)."""
    ref = R.reference(m, "uniform", WC.DTYPES[dt], True, False, 7)
    o = ref.o
    w = o.w.double().requires_grad_(True)
    gamma = (o.scale.double() / o.invstd.double()).requires_grad_(True)
    beta = torch.zeros(m.Cout, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(o.x.double(), w, None, m.stride, m.pad, R.dilation(m), m.groups)
    z = (y - o.mean.double().view(1, -1, 1, 1)) * o.invstd.double().view(1, -1, 1, 1) * gamma.view(1, -1, 1, 1) + \
        beta.view(1, -1, 1, 1)
    z.backward(o.g.double())
    dw, dgamma, dbeta = ref.exact()
    for name, a, b in (("dw", dw, w.grad), ("dgamma", dgamma, gamma.grad), ("dbeta", dbeta, beta.grad)):
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-12 * max(scale, 1.0), (name, m)
    cw = torch.nn.grad.conv2d_weight(o.x.double(), R.wshape(m), o.g.double(), m.stride, m.pad, R.dilation(m), m.groups)
    assert torch.equal(cw, ref.G)
    # the per-pixel terms of the fault models add up to the oracle
    if R.pixels(m) <= 200:
        G = torch.zeros_like(ref.G)
        col = torch.zeros_like(ref.colsum)
        for p in range(R.pixels(m)):
            dG, dc = R.pixel_term(ref, p)
            G += dG
            col += dc
        assert float((G - ref.G).abs().max()) <= 1e-12 * float(ref.Gabs.max())
        assert float((col - ref.colsum).abs().max()) <= 1e-12 * float(ref.colabs.max())
        for idx in ((0, 0, 0, 0), (m.Cout - 1, R.wshape(m)[1] - 1, m.k - 1, m.k - 1)):
            terms = R.element_split_terms(ref, idx, 64)
            assert abs(sum(terms) - float(ref.exact()[0][idx])) <= 1e-12 * float(ref.Gabs.max()) * 2


def test_integer_operands_are_exactly_summable():
    """The premise of the equality check: with the integer generator every partial sum is an integer below 2^24."""
    for c in WC.CASES:
        for m in c.members:
            K = R.pixels(m)
            assert K <= 2 ** 14 and K * R.ktot(m) + K <= 2 ** 24, (c.id, K, R.ktot(m))
    ref = R.reference(WC.CASES[0].members[0], "integers", torch.bfloat16, True, True, 3)
    for t in ref.exact():
        assert torch.equal(t, t.round()) or torch.equal(t * 4, (t * 4).round())     # invstd down to 2^-2
    o = ref.o
    assert set(o.x.unique().tolist()) <= {-1.0, 0.0, 1.0} and set(o.mean.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert set(torch.log2(o.invstd).unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert bool((o.mean != 0).any()) and torch.equal(o.scale, torch.ones_like(o.scale))


# ---- plan predicates ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_plan_predicate_holds_on_the_host_planner(case):
    before = {k: v for k, v in os.environ.items() if k.startswith("TDN_")}
    per, _ = plan_of(case)
    assert not WC.plan_problems(case, per), "\n".join(WC.plan_problems(case, per))
    assert {k: v for k, v in os.environ.items() if k.startswith("TDN_")} == before


def test_the_table_covers_what_it_is_for():
    """Per tap-tile id 1..8 and per nine-tap variant: a direct plan, a 2..7-split plan and a >= 8-split plan with idle
    workgroup slots; id 0 (the stem's row, never direct) and the grouped members: slab plans at >= 8 splits with idle
    slots; BN operands on a direct and a slab member of every finalize map_mode; both 256-split cases."""
    seen = {}
    bn_seen = set()
    for c in WC.CASES:
        per, _ = plan_of(c)
        for m, bn, row in zip(c.members, c.bn, per):
            variant, bmw, bnw, splitk, mchunk, direct = row[:6]
            if variant:
                key = "t9v%d" % variant
            elif m.kind != "conv":
                key = m.kind
            else:
                key = "s%s" % c.knobs.get("TDN_WGRAD_SHAPE", "default")
            kind = "direct" if direct else ("2-7" if 2 <= splitk <= 7 else
                                            ("idle" if splitk >= 8 and WC.slots(splitk) > splitk else "other"))
            seen.setdefault(key, set()).add(kind)
            if bn:
                bn_seen.add((m.kind, bool(direct)))
                if direct and (m.Cin // 64 if variant else m.k * m.k * (m.Cin // bnw)) > 1:
                    bn_seen.add(("several dot partials", "t9" if variant else "tap"))
    for key in ["s%d" % i for i in range(1, 9)] + ["t9v1", "t9v2"]:
        assert {"direct", "2-7", "idle"} <= seen[key], (key, seen[key])
    for key in ("stem", "gconv"):
        assert {"2-7", "idle"} <= seen[key] and "direct" not in seen[key], (key, seen[key])
    assert {("conv", True), ("conv", False), ("stem", False), ("gconv", False), ("several dot partials", "tap"),
            ("several dot partials", "t9")} <= bn_seen, bn_seen
    caps = [c for c in WC.CASES if c.expect[0].get("splitk") == 256]
    assert len(caps) >= 3
    for c in caps:
        assert list(refs_of(c, 0)) == ["integers"], c.id        # decided from the numbers, not from a list
    accs = {(c.members[0].kind, plan_of(c)[0][0][5]) for c in WC.CASES if c.accumulate}
    assert accs == {("conv", 1), ("conv", 0), ("stem", 0), ("gconv", 0)}, accs


# ---- sensitivity ----------------------------------------------------------------------------------------------------------------
def sensitivity(case):
    """[(member, mutation, {generator: 'rejected' | 'passes'} or None when inexpressible)] and the clean verdicts."""
    per, _ = plan_of(case)
    rows, clean = [], []
    for i, m in enumerate(case.members):
        splitk, mchunk = per[i][3], per[i][4]
        refs = refs_of(case, i)
        verdicts = {}
        for gen, ref in refs.items():
            recs = R.check_member(ref, *[None if t is None else t.float() for t in ref.exact()], what=case.id)
            clean.append((i, gen, [r for r in recs if r["bad"]]))
            for name, mut in R.mutants(ref, splitk, mchunk):
                if mut is None:
                    verdicts.setdefault(name, None)
                    continue
                bad = any(r["bad"] for r in R.check_member(ref, *mut, what=case.id))
                verdicts.setdefault(name, {})[gen] = "rejected" if bad else "passes"
        for name in R.MUTATIONS:
            rows.append((i, name, verdicts[name]))
    return rows, clean


@pytest.mark.parametrize("case", WC.CASES, ids=WC.IDS)
def test_every_fault_is_rejected(case):
    rows, clean = sensitivity(case)
    for i, gen, bad in clean:
        assert not bad, "the oracle's own result fails its check: member %d, %s: %s" % (i, gen, bad)
    for i, name, v in rows:
        m = case.members[i]
        if v is None:        # inexpressible: only for these structural reasons
            why = {R.MUTATIONS[3]: m.pad == 0, R.MUTATIONS[4]: m.pad == 0 or m.N == 1, R.MUTATIONS[6]: not case.bn[i]}
            assert why.get(name, False), (case.id, i, name)
            continue
        assert "rejected" in v.values(), "%s member %d: '%s' passes the check (%s)" % (case.id, i, name, v)
        if "integers" in v:
            assert v["integers"] == "rejected", (case.id, i, name, v)


def test_failure_report_names_the_split_and_the_tile():
    """explain() on a dropped pixel: the report names that pixel, the split that owns it, and the tile."""
    case = [c for c in WC.CASES if c.id == "tap-s3-k3-s13of16"][0]
    per, _ = plan_of(case)
    ref = refs_of(case, 0)["uniform"]
    splitk, mchunk = per[0][3], per[0][4]
    muts = dict(R.mutants(ref, splitk, mchunk))
    for name, pixel in ((R.MUTATIONS[0], mchunk), (R.MUTATIONS[1], ref.K - 1)):
        bad = [r for r in R.check_member(ref, *muts[name], what=case.id) if r["bad"]]
        assert bad and bad[0]["what"].endswith(" dw")
        kind, mp, sp, _ = R.owner(ref, tuple(bad[0]["index"]), bad[0]["got"] - bad[0]["v"], mchunk)
        assert (kind, mp, sp) == ("pixel", pixel, pixel // mchunk), (name, kind, mp, sp)
        text = R.explain(ref, bad[0], per[0])
        assert "split %d (pixels" % (pixel // mchunk) in text and "tile (co " in text and "13 splits of 64 px" in text, text
    bad = [r for r in R.check_member(ref, *muts[R.MUTATIONS[5]], what=case.id) if r["bad"]]
    assert [r["what"].split()[-1] for r in bad] == (["dgamma", "dbeta"] if ref.bn else ["dbeta"])
    assert "co tile" in R.explain(ref, bad[-1], per[0])


def test_fault_models_are_expressible_somewhere():
    """Every fault model applies to many cases (none is vacuous), on every kernel family."""
    count = {n: 0 for n in R.MUTATIONS}
    for c in WC.CASES:
        for m, bn in zip(c.members, c.bn):
            count[R.MUTATIONS[3]] += m.pad > 0
            count[R.MUTATIONS[4]] += m.pad > 0 and m.N > 1
            count[R.MUTATIONS[6]] += bool(bn)
    assert count[R.MUTATIONS[3]] >= 40 and count[R.MUTATIONS[4]] >= 20 and count[R.MUTATIONS[6]] >= 40, count


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("| case | member | generators | " + " | ".join(R.MUTATIONS) + " |")
    print("|---|---|---|" + "---|" * len(R.MUTATIONS))
    for c in WC.CASES:
        rows, _ = sensitivity(c)
        for i in range(len(c.members)):
            cells = []
            for _, name, v in [r for r in rows if r[0] == i]:
                cells.append("n/a" if v is None else ", ".join("%s: %s" % (g[0], s) for g, s in sorted(v.items())))
            print("| %s | %d | %s | %s |" % (c.id, i, "+".join(sorted(refs_of(c, i))), " | ".join(cells)))
