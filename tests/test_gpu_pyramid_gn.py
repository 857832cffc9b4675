"""GPU: GroupNorm (+ ReLU) with shared affine parameters over a pyramid (csrc/pyramid_gn.hip) through the
wrappers of pyramid_ops.py against the float64 oracle tests/pyramid_gn_ref.py, under guard-banded, poisoned allocations
with exact-size workspaces (tests/guard_util.py).  The criteria are those of tests/test_gpu_gn.py, imported from it:

  y       |err| <= |ref| * ulp + 1e-5 * max|ref|                      per level
  dz      max|err| / max|ref| <= 2 ulp                                per level
  mean    |err| <= 2^-23 |ref| + 2^-23 std_ref,   rstd  relative error <= 2^-12
  dbeta   |err| <= K 2^-24 sum|g|,  dgamma  |err| <= (K 2^-24 + 2^-12) sum|g * xhat_ref|  per channel, K and the sums taken
          over the whole pyramid (its levels laid side by side as one map); rel_l2 <= 1e-3 too

The backward is specified on the y it is handed — the cotangent counts as 0 where that y <= 0 — so the reference masks
by the device's stored y, which the forward check has just compared with the oracle's."""
import numpy as np
import pytest
import torch

import guard_util as G
import pyramid_gn_ref as R
import test_gpu_gn as GN
from test_gpu_gn import BF, FP, ULP

pytestmark = pytest.mark.gpu

EPS = 1e-5
CG = [(64, 32), (64, 1), (256, 32), (512, 32), (128, 2)]
# (B, [(H, W)]): four levels down to one pixel; a first level of several chunks with a ragged last
# one (asserted from the plan) over a small tail; an empty level in the middle; a single level
PYRAMIDS = {
    "four": (2, [(9, 8), (5, 4), (3, 2), (1, 1)]),
    "chunks": (1, [(37, 41), (3, 2)]),
    "hole": (2, [(5, 4), (0, 4), (3, 2)]),
    "single": (1, [(6, 10)]),
}


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    from torch_detection_amd import pyramid_ops
    return pyramid_ops


@pytest.fixture()
def guard(monkeypatch, P):
    g = G.GuardAlloc()
    G.install(monkeypatch, P, g)
    return g


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def dev(a, dt, guard=None):
    """NCHW array of dt-representable values -> logical NCHW device tensor in channels_last memory (a guarded copy with
    NaN bands under the guard)"""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).permute(0, 2, 3, 1).contiguous().to(dt).cuda()
    if guard is not None:
        t = guard.guard_copy(t)
    return t.permute(0, 3, 1, 2)


def host(t):
    """logical NCHW device tensor -> float64 NCHW array"""
    return t.detach().float().cpu().contiguous().numpy().astype(np.float64)


def inputs(B, sizes, C, dt, seed=1):
    """Per level: z with statistics that differ between the images and the levels, and an unmasked cotangent."""
    zs, gs = [], []
    for l, (H, W) in enumerate(sizes):
        if H * W == 0:
            zs.append(np.zeros((B, C, H, W)))
            gs.append(np.zeros((B, C, H, W)))
            continue
        zs.append(GN._rq(GN._varied((B, C, H, W), seed + 10 * l, dt) * (1.0 + 0.5 * l) - 0.7 * l, dt))
        gs.append(GN._rq(GN._det((B, C, H, W), 5 + 10 * l, -1, 1), dt))
    return zs, gs


def side_by_side(maps):
    """The levels of a pyramid as one (B, C, sum H W, 1) map"""
    return np.concatenate([m.reshape(m.shape[0], m.shape[1], -1, 1) for m in maps], axis=2)


def check_fwd(ys, stats, zs, gamma, beta, Gr, relu, dt, tag, eps=EPS):
    """-> the device's y per level as float64"""
    C = gamma.shape[0]
    cpg = C // Gr
    ref, mean, rstd = R.fwd(zs, gamma, beta, Gr, eps, relu)
    assert tuple(stats.shape) == (len(zs), zs[0].shape[0], C, 2) and stats.dtype == torch.float32
    got = []
    for l, z in enumerate(zs):
        assert ys[l].dtype == dt and tuple(ys[l].shape) == z.shape and ys[l].permute(0, 2, 3, 1).is_contiguous()
        got.append(host(ys[l]))
        if z.size == 0:
            assert float(stats[l].abs().max()) == 0.0, tag + ": an empty level's statistics are zero"
            continue
        std = np.sqrt(np.maximum(rstd[l] ** -2 - eps, 0.0))
        GN._check_stats(stats[l], mean[l].repeat(cpg, 1), rstd[l].repeat(cpg, 1), std.repeat(cpg, 1),
                        "%s level %d" % (tag, l))
        GN._check_y(got[l], ref[l], ULP[dt], "%s level %d" % (tag, l))
    return got


def check_bwd(dzs, dg, db, gs, ys_dev, zs, gamma, beta, Gr, relu, dt, tag, eps=EPS):
    rdz, rdg, rdb = R.bwd(gs, zs, gamma, beta, Gr, eps, relu, mask_src=ys_dev)
    gm = [g * (y > 0) for g, y in zip(gs, ys_dev)] if relu else gs
    live = [l for l, z in enumerate(zs) if z.size]
    for l in live:
        assert dzs[l].dtype == dt and tuple(dzs[l].shape) == zs[l].shape
        den = np.abs(rdz[l]).max()
        mr = float(np.abs(host(dzs[l]) - rdz[l]).max() / (den if den > 0 else 1.0))
        print("%s level %d: dz max_rel %.3g (limit %.3g)" % (tag, l, mr, 2 * ULP[dt]))
        assert mr <= 2 * ULP[dt], "%s level %d dz" % (tag, l)
    xhat = [R.N.gn_xhat(zs[l], Gr, eps) for l in live]
    GN._check_bwd(side_by_side([host(dzs[l]) for l in live]), GN._f64(dg), GN._f64(db),
                  (side_by_side([rdz[l] for l in live]), rdg, rdb), side_by_side([gm[l] for l in live]),
                  side_by_side(xhat), ULP[dt], tag)


def run(P, guard, B, sizes, C, Gr, dt, relu, tag, zs=None, eps=EPS):
    gamma, beta = GN._affine(C)
    z0, gs = inputs(B, sizes, C, dt)
    zs = z0 if zs is None else zs
    zd = [dev(z, dt, guard) for z in zs]
    gd = [dev(g, dt, guard) for g in gs]
    gam, bet = GN._vec(gamma), GN._vec(beta)
    ys, stats = P.pyramid_gn_fwd(zd, gam, bet, Gr, eps, relu)
    ys_dev = check_fwd(ys, stats, zs, gamma, beta, Gr, relu, dt, tag, eps)
    dzs, dg, db = P.pyramid_gn_bwd(gd, ys if relu else None, zd, stats, gam, Gr, relu)
    check_bwd(dzs, dg, db, gs, ys_dev, zs, gamma, beta, Gr, relu, dt, tag, eps)
    if guard is not None:
        found = guard.check()
        assert not found, "\n".join(found)
        assert all(asked == given for _, asked, given in guard.ws_log), guard.ws_log
        assert guard.ws_calls["pyramid_gn_fwd"] == guard.ws_calls["pyramid_gn_bwd"] >= 1   # one workspace per call
    return zd, gd, ys, stats, dzs, dg, db


def _id(v):
    return "bf16" if v is BF else "fp16" if v is FP else "%d-%d" % v if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("dt", [BF, FP], ids=_id)
@pytest.mark.parametrize("cg", CG, ids=_id)
@pytest.mark.parametrize("name", list(PYRAMIDS))
def test_pyramid_gn_against_the_oracle_under_the_guard(P, guard, name, cg, dt):
    B, sizes = PYRAMIDS[name]
    C, Gr = cg
    if name == "chunks":
        pl = P.pyramid_gn_plan(P.GN_FWD, B, sizes, C, Gr)
        assert pl.chunks[0] >= 3 and (sizes[0][0] * sizes[0][1]) % pl.chunk_pixels[0] != 0
    if name == "hole":
        assert P.pyramid_gn_plan(P.GN_BWD, B, sizes, C, Gr).chunks[1] == 0
    for relu in (True, False):
        run(P, guard, B, sizes, C, Gr, dt, relu, "pyr gn %s %s %s relu=%d" % (name, _id(cg), _id(dt), relu))


@pytest.mark.parametrize("row", [("fp16-m8-k2", FP, 8.0, 2), ("fp16-m64-k3", FP, 64.0, 3), ("bf16-m8-k2", BF, 8.0, 2)],
                         ids=lambda r: r[0])
def test_ill_conditioned_row_spread_over_a_pyramid(P, guard, row):
    """|mean| / std in the hundreds (asserted for the fp16 rows) in every level of a pyramid: rstd within 2^-12."""
    name, dt, m, kmax = row
    B, sizes, C, Gr = 2, [(16, 24), (8, 12), (4, 6), (2, 3)], 256, 32
    zs = [GN.cond_input((B, C, H, W), dt, m, kmax, seed=11 + l) for l, (H, W) in enumerate(sizes)]
    if dt is FP:
        assert min(GN._cond_ratio_gn(z, Gr) for z in zs) >= 250.0
    run(P, guard, B, sizes, C, Gr, dt, False, "pyr gn cond " + name, zs=zs)


def test_constant_group_gives_beta_exactly(P, guard):
    B, sizes, C, Gr, dt = 2, [(16, 24), (4, 6), (1, 1)], 256, 32, FP
    cpg = C // Gr
    const = (np.arange(C) // cpg) % 2 == 0
    zs = []
    for l, (H, W) in enumerate(sizes):
        z = GN.cond_input((B, C, H, W), dt, 8.0, 2, seed=21 + l)
        z[:, const] = 8.0 + l
        zs.append(z)
    _, beta = GN._affine(C)
    want = torch.from_numpy(beta.astype(np.float32)).half().float().numpy().astype(np.float64)
    _, _, ys, stats, _, _, _ = run(P, guard, B, sizes, C, Gr, dt, False, "pyr gn const", zs=zs)
    for l, y in enumerate(ys):
        yh = host(y)
        assert np.array_equal(yh[:, const], np.broadcast_to(want[None, const, None, None], yh[:, const].shape)), l
        assert np.allclose(stats[l][:, const, 1].cpu().numpy(), EPS ** -0.5, rtol=1e-6)


def test_outputs_that_are_exactly_zero_are_masked(P, guard):
    """beta = 0 and every z of a group equal to the group mean: y == 0 exactly there, with and without a sign; such
    elements count as masked — their cotangent is 0 in the sums, and dz is the masked form."""
    B, sizes, C, Gr, dt = 2, [(5, 4), (3, 2)], 64, 32, BF
    cpg = C // Gr
    zero = (np.arange(C) // cpg) % 2 == 0                     # constant groups: z == mean, xhat == 0, y == 0
    z0, gs = inputs(B, sizes, C, dt)
    for z in z0:
        z[:, zero] = 1.5
    gamma = GN._affine(C)[0]
    gamma[1::4] *= -1.0                                       # -0.0 as well as +0.0
    beta = np.zeros(C)
    zd, gd = [dev(z, dt, guard) for z in z0], [dev(g, dt, guard) for g in gs]
    gam, bet = GN._vec(gamma), GN._vec(beta)
    ys, stats = P.pyramid_gn_fwd(zd, gam, bet, Gr, EPS, True)
    ys_dev = [host(y) for y in ys]
    for y in ys_dev:
        assert (y[:, zero] == 0).all() and (y[:, ~zero] > 0).any()
    dzs, dg, db = P.pyramid_gn_bwd(gd, ys, zd, stats, gam, Gr, True)
    # constant groups: every cotangent masked -> no contribution to the sums, dz == 0 exactly
    assert (GN._f64(dg)[zero] == 0).all() and (GN._f64(db)[zero] == 0).all()
    for dz in dzs:
        assert (host(dz)[:, zero] == 0).all()
    check_bwd(dzs, dg, db, gs, ys_dev, z0, gamma, beta, Gr, True, dt, "pyr gn zero outputs")
    # the masked form: the same as handing in cotangents that are already zero there, bit for bit
    gz = [dev(np.where(y > 0, g, 0.0), dt) for g, y in zip(gs, ys_dev)]     # +0, as the kernel's own mask gives
    dzs2, dg2, db2 = P.pyramid_gn_bwd(gz, ys, zd, stats, gam, Gr, True)
    dzs3, dg3, db3 = P.pyramid_gn_bwd(gz, None, zd, stats, gam, Gr, False)
    for a, b, c in zip(dzs, dzs2, dzs3):
        assert same_bits(a, b) and same_bits(a, c)
    assert same_bits(dg, dg2) and same_bits(db, db2) and same_bits(dg, dg3) and same_bits(db, db3)
    assert not guard.check()


@pytest.mark.parametrize("name,cg", [("four", (64, 32)), ("chunks", (256, 32)), ("hole", (128, 2))], ids=_id)
def test_one_launch_over_the_pyramid_equals_level_by_level(P, name, cg):
    """The same entry point with one level at a time: y, stats and dz bit for bit; dgamma / dbeta of the pyramid call
    against the level-order fp32 sum of the single-level calls within the bound of the sums."""
    B, sizes = PYRAMIDS[name]
    C, Gr = cg
    dt = BF
    gamma, beta = GN._affine(C)
    zs, gs = inputs(B, sizes, C, dt)
    zd, gd = [dev(z, dt) for z in zs], [dev(g, dt) for g in gs]
    gam, bet = GN._vec(gamma), GN._vec(beta)
    ys, stats = P.pyramid_gn_fwd(zd, gam, bet, Gr, EPS, True)
    dzs, dg, db = P.pyramid_gn_bwd(gd, ys, zd, stats, gam, Gr, True)
    sum_g = torch.zeros_like(dg)
    sum_b = torch.zeros_like(db)
    for l in range(len(sizes)):
        y1, s1 = P.pyramid_gn_fwd([zd[l]], gam, bet, Gr, EPS, True)
        if not zs[l].size:
            continue
        assert same_bits(ys[l], y1[0]) and same_bits(stats[l], s1[0]), l
        dz1, dg1, db1 = P.pyramid_gn_bwd([gd[l]], [ys[l]], [zd[l]], s1, gam, Gr, True)
        assert same_bits(dzs[l], dz1[0]), l
        sum_g, sum_b = sum_g + dg1, sum_b + db1
    # (the pyramid call adds image by image through the levels, the loop above level totals: the same terms, another
    # bracketing, so the sums are compared through the bound and not bit for bit)
    ys_dev = [host(y) for y in ys]
    check_bwd(dzs, sum_g, sum_b, gs, ys_dev, zs, gamma, beta, Gr, True, dt, "pyr gn level sums " + name)
    check_bwd(dzs, dg, db, gs, ys_dev, zs, gamma, beta, Gr, True, dt, "pyr gn pyramid sums " + name)


@pytest.mark.parametrize("dt", [BF, FP], ids=_id)
@pytest.mark.parametrize("shape", [(2, 6, 10, 64, 32), (1, 37, 41, 64, 32), (2, 3, 2, 512, 2)],
                         ids=lambda s: "B%d-%dx%d-C%d-G%d" % s)
def test_a_single_level_equals_the_single_map_kernels_bit_for_bit(P, shape, dt):
    """One level through pyramid_gn_fwd and the same map through ops.gn_fwd (no addend): the same bits of y and of the
    statistics.  The shapes: one chunk; several chunks with a ragged last one; 256 channels per group."""
    from torch_detection_amd import ops
    B, H, W, C, Gr = shape
    gamma, beta = GN._affine(C)
    zs, _ = inputs(B, [(H, W)], C, dt)
    zd = dev(zs[0], dt)
    gam, bet = GN._vec(gamma), GN._vec(beta)
    for relu in (False, True):
        ys, stats = P.pyramid_gn_fwd([zd], gam, bet, Gr, EPS, relu)
        y1, stats1 = ops.gn_fwd(zd.permute(0, 2, 3, 1), gam, bet, Gr, EPS, None, relu)
        assert tuple(stats.shape) == (1, B, C, 2) and tuple(stats1.shape) == (B, C, 2)
        assert same_bits(ys[0].permute(0, 2, 3, 1), y1), "y, relu=%d" % relu
        assert same_bits(stats[0], stats1), "stats, relu=%d" % relu


@pytest.mark.parametrize("dt", [BF, FP], ids=_id)
def test_twice_and_graph_replay_are_bit_identical(P, dt):
    B, sizes = PYRAMIDS["chunks"]
    C, Gr = 256, 32
    gamma, beta = GN._affine(C)
    zs, gs = inputs(B, sizes, C, dt)
    zd, gd = [dev(z, dt) for z in zs], [dev(g, dt) for g in gs]
    gam, bet = GN._vec(gamma), GN._vec(beta)

    def both():
        ys, stats = P.pyramid_gn_fwd(zd, gam, bet, Gr, EPS, True)
        dzs, dg, db = P.pyramid_gn_bwd(gd, ys, zd, stats, gam, Gr, True)
        return ys + [stats] + dzs + [dg, db]

    first, second = both(), both()
    assert all(same_bits(a, c) for a, c in zip(first, second))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = both()
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))
    graph.replay()
    assert all(same_bits(a, c) for a, c in zip(first, held))


def test_acc_accumulates_and_zero_overwrites(P):
    B, sizes = PYRAMIDS["four"]
    C, Gr, dt = 64, 32, BF
    gamma, beta = GN._affine(C)
    zs, gs = inputs(B, sizes, C, dt)
    zd, gd = [dev(z, dt) for z in zs], [dev(g, dt) for g in gs]
    gam, bet = GN._vec(gamma), GN._vec(beta)
    ys, stats = P.pyramid_gn_fwd(zd, gam, bet, Gr, EPS, True)
    dz0, dg0, db0 = P.pyramid_gn_bwd(gd, ys, zd, stats, gam, Gr, True)
    base_g, base_b = GN._det((C,), 8, -30, 30).astype(np.float32), GN._det((C,), 9, -30, 30).astype(np.float32)
    bg, bb = GN._vec(base_g), GN._vec(base_b)
    _, dg1, db1 = P.pyramid_gn_bwd(gd, ys, zd, stats, gam, Gr, True, bg, bb, True)
    assert dg1.data_ptr() == bg.data_ptr() and db1.data_ptr() == bb.data_ptr()
    # acc = 1: old + sum, one fp32 addition of two fp32 values
    assert same_bits(bg, torch.from_numpy(base_g).cuda() + dg0) and same_bits(bb, torch.from_numpy(base_b).cuda() + db0)
    dz2, _, _ = P.pyramid_gn_bwd(gd, ys, zd, stats, gam, Gr, True, bg, bb, False)
    assert same_bits(bg, dg0) and same_bits(bb, db0) and all(same_bits(a, c) for a, c in zip(dz0, dz2))


def test_refusals_launch_nothing(P):
    z = lambda C, H=4, W=4, B=1, dt=BF: torch.zeros(B, H, W, C, dtype=dt, device="cuda").permute(0, 3, 1, 2)
    w = lambda C: torch.ones(C, device="cuda")
    with pytest.raises(ValueError, match="C must be one of"):
        P.pyramid_gn_fwd([z(96)], w(96), w(96), 32)
    with pytest.raises(ValueError, match="groups must divide"):
        P.pyramid_gn_fwd([z(64)], w(64), w(64), 48)
    with pytest.raises(ValueError, match="1..8 levels"):
        P.pyramid_gn_fwd([z(64)] * 9, w(64), w(64), 32)
    with pytest.raises(ValueError, match="channels_last"):
        P.pyramid_gn_fwd([torch.zeros(1, 64, 4, 4, dtype=BF, device="cuda")], w(64), w(64), 32)
    with pytest.raises(ValueError):
        P.pyramid_gn_fwd([z(64), z(64, B=2)], w(64), w(64), 32)            # one batch size
    with pytest.raises(ValueError):
        P.pyramid_gn_fwd([z(64), z(64, dt=FP)], w(64), w(64), 32)          # one dtype
    with pytest.raises(ValueError, match="gamma"):
        P.pyramid_gn_fwd([z(64)], w(32), w(64), 32)
    ys, stats = P.pyramid_gn_fwd([z(64)], w(64), w(64), 32)
    with pytest.raises(ValueError, match="stats"):
        P.pyramid_gn_bwd([z(64)], ys, [z(64)], stats[0], w(64), 32)
    with pytest.raises(ValueError, match="ys"):
        P.pyramid_gn_bwd([z(64)], None, [z(64)], stats, w(64), 32, True)
    # an empty batch launches nothing forward and writes zero sums backward
    e = [z(64, B=0)]
    ye, se = P.pyramid_gn_fwd(e, w(64), w(64), 32)
    assert tuple(ye[0].shape) == (0, 64, 4, 4) and tuple(se.shape) == (1, 0, 64, 2)
    _, dg, db = P.pyramid_gn_bwd(e, ye, e, se, w(64), 32)
    assert float(dg.abs().max()) == 0 and float(db.abs().max()) == 0
