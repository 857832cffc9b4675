"""CPU-only proofs about the case tables of fp16_conv_cases.py: what the GPU tests of test_gpu_fp16_conv.py take for
granted.  Every planted value's expected bit pattern, the exactness of the summable inputs (two summation orders and
fp64), that every forced tile divides its shape and leaves a partial last M tile, that every halo id runs somewhere,
and the receptive-field sets."""
import pytest
import torch
import torch.nn.functional as F

import bound_util as B
import fp16_conv_cases as C

H16, BF16 = torch.float16, torch.bfloat16


# ---- part 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("geom", C.P1_GEOMS)
def test_every_forced_tile_divides_and_leaves_an_m_tail(geom, kind):
    N, H, W, Cin, Cout = C.P1_SHAPE
    k, s = geom
    d = C.gemm_dims(kind, N, H, W, Cin, Cout, k, s)
    assert len(d["classes"]) == (s * s if kind == 1 else 1)
    if kind == 1 and s == 2:
        assert len(set(d["classes"])) == 4, "four parity classes of unequal size"
    for tile, (bm, bn, bk) in C.TILES.items():
        # the divisibility choose_cfg tests: for tiles 0 and 25, which report the same extents, this IS the evidence
        assert C.tile_divides(tile, d["ngemm"], d["ktap"]), (tile, d)
        assert d["M"] % bm != 0, "partial last M tile (tile %d, M = %d)" % (tile, d["M"])
    assert set(C.P1_BF16_DGRAD_TILES) | set(C.P1_BF16_FWD_TILES) <= set(C.TILES)


def test_p1_shape_has_no_image_on_a_tile_boundary():
    N, H, W, _, _ = C.P1_SHAPE
    assert N * H * W == 297
    for bm in (64, 128, 192):
        assert 297 % bm != 0 and all((n * H * W) % bm != 0 for n in range(1, N))


def test_tile_table_matches_the_source():
    """TILES restates TDN_GEMM_CFGS of csrc/conv_igemm.hip: read the rows out of the source."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "torch_detection_amd", "csrc", "conv_igemm.hip")).read()
    rows = re.findall(r"^\s*X\((\d+), (\d+), (\d+), (\d+), ", src, re.M)
    assert {int(r[0]): (int(r[1]), int(r[2]), int(r[3])) for r in rows} == dict(C.TILES)


# ---- part 2 --------------------------------------------------------------------------------------------------------------
def test_every_halo_id_runs_on_a_listed_shape():
    for kind in (0, 1):
        for cfg in C.CFG3:
            assert any(C.halo3_applies(cfg, kind, case) for case in C.HALO3_SHAPES), (cfg, kind)
    for cfg in C.CFG1:
        assert all(C.halo1_applies(cfg, case) for case in C.HALO1_SHAPES), cfg
    assert {c for c, _ in C.HALO3_PARAMS} == set(C.CFG3) and {c for c, _ in C.HALO1_PARAMS} == set(C.CFG1)
    import test_gpu_halo as TH     # the bf16 suite's tables: the same ids and multiples, the shapes a subset of its own
    assert dict(C.CFG3) == TH.CFG3 and dict(C.CFG1) == TH.CFG1
    assert set(C.HALO3_SHAPES) <= set(TH.CASES3) and set(C.HALO1_SHAPES) <= set(TH.CASES1)
    assert set(C.HALO3_ONE_CHUNK) <= set(C.CFG3)


def _halo_id(kind, case, k, s, pad, env):
    """The halo configuration the host-only planner reports for the conv under ``env`` (None: the generic kernel)."""
    import ctypes
    import os
    from torch_detection_amd import _lib
    saved = {n: os.environ.pop(n) for n in list(os.environ) if n.startswith("TDN_")}
    try:
        os.environ.update({n: str(v) for n, v in env.items()})
        o = (ctypes.c_int32 * 16)()
        assert _lib.load().tdn_conv2d_plan(kind, case[0], case[1], case[2], case[3], case[4], k, s, pad, o) == 0
    finally:
        for n in env:
            os.environ.pop(n, None)
        os.environ.update(saved)
    return o[8] - 100 if o[8] >= 100 else None


def test_planner_takes_every_halo_id_on_a_listed_shape():
    """The channel multiples are necessary, not sufficient (patch images and weight ring must fit LDS): ask the
    planner itself, which needs no GPU.  Every 3x3 id runs a forward AND an input gradient on some listed shape, every
    1x1 id on both of its shapes."""
    for kind in (0, 1):
        for cfg in C.CFG3:
            cases = [case for c, case in C.HALO3_PARAMS if c == cfg and C.halo3_applies(cfg, kind, case)]
            assert any(_halo_id(kind, case, 3, 1, 1, {"TDN_HALO_CFG3": cfg}) == cfg for case in cases), (cfg, kind)
    for cfg, case in C.HALO1_PARAMS:
        assert _halo_id(0, case, 1, case[5], 0, {"TDN_HALO": 3, "TDN_HALO_CFG1": cfg}) == cfg, (cfg, case)
    # part 4's and part 5's halo routes
    c3, n3 = C.EDGE_HALO3
    assert _halo_id(0, (1, 8, 8, 64, n3), 3, 1, 1, {"TDN_HALO_CFG3": c3}) == c3
    assert _halo_id(1, (1, 8, 8, n3, 64), 3, 1, 1, {"TDN_HALO_CFG3": c3}) == c3
    c1, n1 = C.EDGE_HALO1
    assert _halo_id(0, (1, 8, 8, 64, n1), 1, 1, 0, {"TDN_HALO": 3, "TDN_HALO_CFG1": c1}) == c1
    assert _halo_id(1, (1, 8, 8, n1, 64), 1, 1, 0, {"TDN_HALO": 3, "TDN_HALO_CFG1": c1}) == c1
    cfg, case = C.POISON_HALO
    assert _halo_id(0, case, 3, 1, 1, {"TDN_HALO_CFG3": cfg}) == cfg and _halo_id(1, case, 3, 1, 1, {"TDN_HALO_CFG3": cfg}) == cfg
    assert C.CFG3[C.EDGE_HALO3[0]] <= C.EDGE_HALO3[1] and C.CFG1[C.EDGE_HALO1[0]] <= C.EDGE_HALO1[1]


# ---- part 4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_planted_values_have_the_expected_bit_patterns(dtname):
    dtype = C.DTYPES[dtname]
    assert {n for n, _, _ in C.PLANTS[dtname]} == set(C.PLANT_BITS[dtname])
    for name, value, e in C.PLANTS[dtname]:
        v = torch.tensor([value], dtype=torch.float64)
        assert float(v.float().double()) == value, "fp32 holds the planted value"
        got = int(C.bits16(C.expected16(v, dtype))[0])
        assert got == C.PLANT_BITS[dtname][name], (name, hex(got))
        assert value / 2.0 ** e == round(value / 2.0 ** e), "a multiple of its channel's quantum"
    if dtype == H16:
        names = [n for n, _, _ in C.PLANTS[dtname]]
        for need in ("65504", "65519->65504", "65520->inf", "65536->inf", "-65520->-inf", "2^-14", "2^-24",
                     "2^-25 tie->0", "3*2^-25 tie->2^-23", "2^-14-2^-25"):
            assert need in names
        for n in ("2^-14", "2^-24", "2^-25 tie->0", "3*2^-25 tie->2^-23", "2^-14-2^-25"):
            assert "-(" + n + ")" in names, "a negative twin of each subnormal"
        inf = torch.tensor([65520.0, 65536.0, -65520.0], dtype=torch.float64)
        assert bool(torch.isinf(C.expected16(inf, H16)).all()) and float(C.expected16(torch.tensor([65519.99]), H16)) == 65504
    # ReLU6 knee: [TOP, 6) stores as TOP, never as 6; 6 and up as exactly 6
    top = C.TOP6[dtype]
    v = torch.tensor([top, (top + 6) / 2, 6 - 2.0 ** -20, 6.0, 6.5, top - 2.0 ** -12, -1.0], dtype=torch.float64)
    got = C.expected16(v, dtype, relu=2).double().tolist()
    assert got[:5] == [top, top, top, 6.0, 6.0] and got[5] <= top and got[6] == 0.0


def _two_orders(x, w, k, transpose):
    """The same sums in fp32 in two orders: the library's, and with the channels and the taps reversed (the conv of
    flipped operands sums the identical products backwards).  Plus one with the channels split in halves."""
    f = F.conv_transpose2d if transpose else F.conv2d
    a = f(x, w, None, 1, k // 2)
    if transpose:
        b = f(x.flip(1), w.flip(0), None, 1, k // 2)
        h = x.shape[1] // 2
        c = f(x[:, h:], w[h:], None, 1, k // 2) + f(x[:, :h], w[:h], None, 1, k // 2)
    else:
        b = f(x.flip(1), w.flip(1), None, 1, k // 2)
        h = x.shape[1] // 2
        c = f(x[:, h:], w[:, h:], None, 1, k // 2) + f(x[:, :h], w[:, :h], None, 1, k // 2)
    return a, b, c


EDGE_FWD = [(dt, k, cout, 64, 8, 8, 0) for dt in C.DTYPES for k in (1, 3) for cout in (64, 128)] + \
           [(dt, 1, 64, 256, 8, 16, 1) for dt in C.DTYPES] + [(dt, k, 64, 64, 8, 8, 2) for dt in C.DTYPES for k in (1, 3)] + \
           [(dt, 3, 128, 64, 8, 8, 2) for dt in C.DTYPES]


@pytest.mark.parametrize("args", EDGE_FWD)
def test_edge_forward_inputs_are_exactly_summable(args):
    dtname = args[0]
    dtype = C.DTYPES[dtname]
    e = C.edge_fwd(*args)
    k = e.k
    assert torch.equal(C.q(e.x, dtype), e.x) and torch.equal(C.q(e.w, dtype), e.w) and float(e.w.abs().min()) >= 1
    conv64 = F.conv2d(e.x.double(), e.w.double(), None, 1, k // 2)
    for c32 in _two_orders(e.x, e.w, k, False):
        assert torch.equal(c32.double(), conv64)
    assert float(conv64.abs().max()) < 2 ** 24 and torch.equal(conv64, conv64.round())       # integers: the quantum is 1
    # the epilogue: a power-of-two scale (exact) and ONE addition whose result fp32 holds exactly
    sc, sh = e.scale.view(1, -1, 1, 1), e.shift.view(1, -1, 1, 1)
    assert torch.equal(torch.log2(e.scale), torch.log2(e.scale).round())
    v32 = conv64.float() * sc + sh
    assert torch.equal(v32.double(), e.exact) and torch.equal(e.exact.float().double(), e.exact)
    # the planted value sits at EDGE_PIX of its channel, and every table entry is planted
    table = C.RELU6_PLANTS[dtname] if e.relu == 2 else C.PLANTS[dtname]
    assert {n for n, _, _ in e.plants} == {n for n, _, _ in table}
    for name, value, ch in e.plants:
        assert float(e.exact[0, ch, C.EDGE_PIX[0], C.EDGE_PIX[1]]) == value
    want = C.expected16(e.exact, dtype, e.relu)
    if e.relu == 2:
        top = C.TOP6[dtype]
        knee = (e.exact >= top) & (e.exact < 6)
        assert int(knee.sum()) > 50 and int((e.exact >= 6).sum()) > 50 and int((e.exact < top).sum()) > 50
        assert bool((want[knee].double() == top).all()) and bool((want[e.exact >= 6].double() == 6).all())
    elif dtype == H16 and e.relu == 0:
        # the sweep around the planted values really crosses the edges
        assert int(torch.isinf(want).sum()) > 100 and int((want.double().abs() == 65504).sum()) > 20
        sub = (want != 0) & (want.double().abs() < 2.0 ** -14)
        assert int(sub.sum()) > 100 and int(((want == 0) & (e.exact != 0)).sum()) > 0
        ties = (e.exact / 2.0 ** -24) % 1 == 0.5
        assert int((ties & (e.exact.abs() < 2.0 ** -14)).sum()) > 100


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_edge_dgrad_inputs_are_exactly_summable(dtname, k, cin):
    dtype = C.DTYPES[dtname]
    e = C.edge_dgrad(dtname, k, cin)
    conv64 = F.conv_transpose2d(e.g.double(), e.w_eff.double(), None, 1, k // 2)
    for c32 in _two_orders(e.g, e.w_eff, k, True):
        assert torch.equal(c32.double(), conv64)
    for ci in range(cin):
        quantum = 2.0 ** C.PLANTS[dtname][ci % len(C.PLANTS[dtname])][2]
        n = conv64[0, ci] / quantum
        assert torch.equal(n, n.round()) and float(n.abs().max()) < 2 ** 24
    v32 = conv64.float() + e.add
    assert torch.equal(v32.double(), e.exact) and torch.equal(e.exact.float().double(), e.exact)
    want = C.expected16(e.exact, dtype)
    for name, value, ch in e.plants:
        assert float(e.exact[0, ch, C.EDGE_PIX[0], C.EDGE_PIX[1]]) == value, name
        assert float(conv64[0, ch, C.EDGE_PIX[0], C.EDGE_PIX[1]]) != 0, "the conv contributes to the planted value"
        assert int(C.bits16(want)[0, ch, C.EDGE_PIX[0], C.EDGE_PIX[1]]) == C.PLANT_BITS[dtname][name]
    if dtype == H16:
        assert int(torch.isinf(want).sum()) > 100
        assert int(((want != 0) & (want.double().abs() < 2.0 ** -14)).sum()) > 100


def test_edge_routes_divide():
    for tile, n in C.EDGE_TILES.items():
        assert C.tile_divides(tile, n, 64), tile
    # the tiles left out do not divide 64 -> 64 or 64 -> 128: BK = 128, BN = 256
    for tile in set(C.TILES) - set(C.EDGE_TILES):
        assert not C.tile_divides(tile, 64, 64) and not C.tile_divides(tile, 128, 64)


@pytest.mark.parametrize("k", [1, 3])
def test_subnormal_operand_case(k):
    v, w, fwd, dg = C.subnormal_operands(k)
    assert torch.equal(C.q(v, H16), v) and float(v.max()) < 2.0 ** -14 and float(v.min()) >= 2.0 ** -24
    m = v.double() / 2.0 ** -24
    assert torch.equal(m, m.round()) and int(m.min()) >= 1 and int(m.max()) <= 1023 and len(m.unique()) > 900
    assert set(w.unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
    for tr, ref in ((False, fwd), (True, dg)):
        for c32 in _two_orders(v, w, k, tr):
            assert torch.equal(c32.double(), ref)
        assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) / 2.0 ** -24 < 2 ** 24
    assert float(fwd.abs().max()) > 0


# ---- part 5 --------------------------------------------------------------------------------------------------------------
GEOMS5 = [(9, 11, k, s, k // 2, 1) for k, s in C.P1_GEOMS] + [(13, 21, 3, 1, 1, 1), (13, 21, 1, 1, 0, 1)]


@pytest.mark.parametrize("geom", GEOMS5)
def test_receptive_fields(geom):
    H, W, k, s, pad, d = geom
    N = 3
    for name, pos in C.poison_positions(N, H, W):
        m = C.field_fwd((N, H, W), pos, k, s, pad, d)
        assert torch.equal(m, C.field_fwd_loops((N, H, W), pos, k, s, pad, d)), (name, pos)
        assert int(m.sum()) > 0, "every chosen position is read by some output (%s)" % name
        assert not bool(m[[n for n in range(N) if n != pos[0]]].any())
        if s == 1:
            assert int(m.sum()) == {"interior": k * k, "corner": ((k + 1) // 2) ** 2, "last": ((k + 1) // 2) ** 2}[name]
    Ho, Wo = C.conv_out(H, k, s, pad, d), C.conv_out(W, k, s, pad, d)
    for name, pos in C.poison_positions(N, Ho, Wo):
        m = C.field_dgrad((N, H, W), pos, k, s, pad, d)
        assert torch.equal(m, C.field_dgrad_loops((N, H, W), pos, k, s, pad, d)), (name, pos)
        assert int(m.sum()) > 0
        # adjointness: input pixel p is in the footprint of cotangent pixel o  <=>  o is in the field of p
        for p in m.nonzero().tolist():
            assert bool(C.field_fwd((N, H, W), tuple(p), k, s, pad, d)[pos])


def test_last_pixel_sits_in_the_m_tail_tile():
    N, H, W, Cin, Cout = C.P1_SHAPE
    for k, s in C.P1_GEOMS:
        for kind in (0, 1):
            M = C.gemm_dims(kind, N, H, W, Cin, Cout, k, s)["M"]
            for tile in C.POISON_TILES:
                bm = C.TILES[tile][0]
                assert (M - 1) // bm == -(-M // bm) - 1 and M % bm != 0


def test_poison_problem_has_no_zero_weight():
    for dtname in C.DTYPES:
        x, w, scale, shift, g, w_eff = C.poison_problem(dtname, 3, 9, 11, 256, 256, 3, 1)
        assert float(w.abs().min()) > 0 and float(scale.min()) > 0 and bool(torch.isfinite(x).all())


# ---- the shared problems are what bound_util judges ---------------------------------------------------------------------------
def test_conv_problem_is_cached_and_representable():
    N, H, W, Cin, Cout = C.P1_SHAPE
    a = C.conv_problem("f16", N, H, W, Cin, Cout, 3, 2)
    assert a is C.conv_problem("f16", N, H, W, Cin, Cout, 3, 2)
    for t in (a.x, a.w, a.res, a.g, a.w_eff, a.add, a.msk):
        assert torch.equal(t.half().float(), t)
    ref = F.relu(F.conv2d(a.x.double(), a.w.double(), None, 2, 1) * a.scale.double().view(1, -1, 1, 1)
                 + a.shift.double().view(1, -1, 1, 1) + a.res.double())
    assert torch.equal(ref, a.fwd_bound.v) and isinstance(a.dgrad_bound, B.Bound)
    assert tuple(a.dgrad_bound.v.shape) == (N, Cin, H, W)
