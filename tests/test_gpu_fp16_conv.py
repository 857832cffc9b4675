"""GPU tests of the conv family in float16: every generic tile and halo configuration forced, the other conv routes,
range edges with exactly known answers, and poison confinement (the last two in both element types).  The cases and
every expectation come from fp16_conv_cases.py; test_fp16_conv_cases_oracle.py proves them on the CPU.

References are F.conv2d and its autograd in fp64 on the CPU over operands made representable in the element type; the
judge of every tolerance check is bound_util.assert_within, elementwise, exactly as the bf16 tests use it.  Parts 4 and
5 have no tolerance at all: the stored bits are the expected bits, and what a poisoned pixel cannot reach is
bit-identical to the clean run.

The worst |err| / allowance per route is printed when the module finishes (pytest -s; recorded in
profiles/fp16_conv_edges.md).
"""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import bound_util as B
import fp16_conv_cases as C
from golden_util import det_tensor, rel_l2

pytestmark = pytest.mark.gpu

H16, BF16 = torch.float16, torch.bfloat16
KNOBS = ("TDN_HALO", "TDN_HALO_CFG3", "TDN_HALO_CFG1", "TDN_HALO_TH", "TDN_HALO_TW", "TDN_HALO_NT", "TDN_HALO_XBUF",
         "TDN_GEMM_CFG")
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from torch_detection_amd import ops as _ops
    from torch_detection_amd import _lib
    _lib.load()
    yield _ops
    if RATIOS:
        print("\nfp16 conv worst ratios: " + json.dumps(RATIOS, indent=1, sort_keys=True))


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def knobs(**kw):
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update({k: str(v) for k, v in kw.items()})


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def pack_w(w, dtype):                 # OIHW -> [O][kh][kw][I]
    return w.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def pack_wd(w, dtype):                # OIHW (scale folded) -> [I][kh][kw][O]
    return w.permute(1, 2, 3, 0).contiguous().to(dtype).cuda()


def plan(ops, kind, N, H, W, Cin, Cout, k, s, pad):
    o = (ctypes.c_int32 * 16)()
    assert ops._lib.load().tdn_conv2d_plan(kind, N, H, W, Cin, Cout, k, s, pad, o) == 0
    return list(o)


def within(route, got, bound, dtype, what):
    r = B.assert_within(got, bound, dtype, what)
    RATIOS[route] = max(RATIOS.get(route, 0.0), r["ratio"])
    return r


def run_fwd(ops, p, dtype, out_f32):
    N, H, W, Cin, Cout, k, s, pad, d = p.geom
    return ops.conv2d_fwd(nhwc(p.x, dtype), pack_w(p.w, dtype), k, s, pad, p.scale.cuda(), p.shift.cuda(),
                          nhwc(p.res, dtype), ops.ADD_SAME, True, out_f32=out_f32)


def run_dgrad(ops, p, dtype, out_f32):
    N, H, W, Cin, Cout, k, s, pad, d = p.geom
    return ops.conv2d_dgrad(nhwc(p.g, dtype), pack_wd(p.w_eff, dtype), (H, W), k, s, pad, nhwc(p.add, dtype),
                            ops.ADD_SAME, nhwc(p.msk, dtype), out_f32=out_f32)


def check_fwd(ops, p, dtype, route, what):
    """Forward with scale, shift, residual and ReLU, stored once as fp32 and once in the element type."""
    y32 = run_fwd(ops, p, dtype, True)
    within(route + " fwd f32", nchw(y32), p.fwd_bound, torch.float32, what + " fwd, f32 store")
    y16 = run_fwd(ops, p, dtype, False)
    assert y16.dtype == dtype
    within(route + " fwd 16", nchw(y16), p.fwd_bound, dtype, what + " fwd, 16-bit store")
    return y32


def check_dgrad(ops, p, dtype, route, what):
    """Input gradient with the folded weight, addend and ReLU mask, stored once as fp32 and once in the element type."""
    dx32 = run_dgrad(ops, p, dtype, True)
    within(route + " dgrad f32", nchw(dx32), p.dgrad_bound, torch.float32, what + " dgrad, f32 store")
    dx16 = run_dgrad(ops, p, dtype, False)
    assert dx16.dtype == dtype
    within(route + " dgrad 16", nchw(dx16), p.dgrad_bound, dtype, what + " dgrad, 16-bit store")
    return dx32


# ---- part 1: every generic tile, forced --------------------------------------------------------------------------------------
def force_tile(ops, tile, kinds, shape):
    """TDN_GEMM_CFG = tile, and the proof that it took: a forced tile that does not divide falls back silently."""
    knobs(TDN_GEMM_CFG=tile, TDN_HALO=0)
    for kind in kinds:
        o = plan(ops, kind, *shape)
        assert tuple(o[3:6]) == C.TILES[tile] and o[8] < 100, "tile %d was not taken: plan %s" % (tile, o)


def forced_tile(ops, dtname, geom, tile, fwd, dgrad):
    dtype = C.DTYPES[dtname]
    N, H, W, Cin, Cout = C.P1_SHAPE
    k, s = geom
    force_tile(ops, tile, [0] * fwd + [1] * dgrad, (N, H, W, Cin, Cout, k, s, k // 2))
    p = C.conv_problem(dtname, N, H, W, Cin, Cout, k, s)
    what = "%s %dx%d s%d tile %d" % (dtname, k, k, s, tile)
    if fwd:
        check_fwd(ops, p, dtype, "%s tile %d" % (dtname, tile), what)
    if dgrad:
        check_dgrad(ops, p, dtype, "%s tile %d" % (dtname, tile), what)


GEOM_IDS = ["%dx%ds%d" % (k, k, s) for k, s in C.P1_GEOMS]


@pytest.mark.parametrize("tile", list(C.TILES))
@pytest.mark.parametrize("geom", C.P1_GEOMS, ids=GEOM_IDS)
def test_forced_tile_f16(ops, geom, tile):
    forced_tile(ops, "f16", geom, tile, True, True)


@pytest.mark.parametrize("tile", sorted(set(C.P1_BF16_DGRAD_TILES) | set(C.P1_BF16_FWD_TILES)))
@pytest.mark.parametrize("geom", C.P1_GEOMS, ids=GEOM_IDS)
def test_forced_tile_bf16_left_out_so_far(ops, geom, tile):
    """The forced dgrad on tiles 0, 1 and 2 and tile 2's forward: what the bf16 lists of test_gpu_kernels.py omit."""
    forced_tile(ops, "bf16", geom, tile, tile in C.P1_BF16_FWD_TILES, tile in C.P1_BF16_DGRAD_TILES)


# ---- part 2: the halo kernel ----------------------------------------------------------------------------------------------------
def uses_halo(ops, kind, *shape):
    return plan(ops, kind, *shape)[8] >= 100


@pytest.mark.parametrize("cfg,case", C.HALO3_PARAMS, ids=["cfg%d-%s" % (c, "x".join(map(str, s))) for c, s in C.HALO3_PARAMS])
def test_halo3_f16(ops, cfg, case):
    N, H, W, Cin, Cout = case
    p = C.conv_problem("f16", N, H, W, Cin, Cout, 3, 1)
    shape = (N, H, W, Cin, Cout, 3, 1, 1)
    knobs(TDN_GEMM_CFG=0)
    y_gen, dx_gen = run_fwd(ops, p, H16, True), run_dgrad(ops, p, H16, True)
    knobs(TDN_HALO_CFG3=cfg)
    ran = 0
    route, what = "f16 halo3 cfg %d" % cfg, "f16 halo %s cfg %d" % (case, cfg)
    if C.halo3_applies(cfg, 0, case) and uses_halo(ops, 0, *shape):
        assert plan(ops, 0, *shape)[8] == 100 + cfg
        y = check_fwd(ops, p, H16, route, what)
        assert torch.equal(y, y_gen), "halo and generic kernels share the K order: bit-identical"
        ran += 1
    if C.halo3_applies(cfg, 1, case) and uses_halo(ops, 1, *shape):
        assert plan(ops, 1, *shape)[8] == 100 + cfg
        dx = check_dgrad(ops, p, H16, route, what)
        assert torch.equal(dx, dx_gen), "halo and generic dgrad share the K order: bit-identical"
        ran += 1
    if not ran:
        pytest.skip("the plan does not fit LDS for this shape")


@pytest.mark.parametrize("cfg,case", C.HALO1_PARAMS, ids=["cfg%d-%s" % (c, "x".join(map(str, s))) for c, s in C.HALO1_PARAMS])
def test_halo1_f16(ops, cfg, case):
    N, H, W, Cin, Cout, s = case
    p = C.conv_problem("f16", N, H, W, Cin, Cout, 1, s)
    shape = (N, H, W, Cin, Cout, 1, s, 0)
    ran = 0
    for nt in (1, 2):
        knobs(TDN_HALO=3, TDN_HALO_CFG1=cfg, TDN_HALO_NT=nt)
        if not uses_halo(ops, 0, *shape):
            continue
        assert plan(ops, 0, *shape)[8] == 100 + cfg
        check_fwd(ops, p, H16, "f16 halo1 cfg %d" % cfg, "f16 halo 1x1 %s cfg %d nt %d" % (case, cfg, nt))
        ran += 1
        if s == 1 and Cin % C.CFG1[cfg] == 0 and uses_halo(ops, 1, *shape):
            check_dgrad(ops, p, H16, "f16 halo1 cfg %d" % cfg, "f16 halo 1x1 %s cfg %d nt %d" % (case, cfg, nt))
    if not ran:
        pytest.skip("the plan does not fit LDS for this shape")


@pytest.mark.parametrize("patch", C.HALO_PATCHES)
def test_halo_patch_shapes_f16(ops, patch):
    N, H, W, Cin, Cout = C.HALO_PATCH_SHAPE
    p = C.conv_problem("f16", N, H, W, Cin, Cout, 3, 1)
    knobs(TDN_HALO_CFG3=5, TDN_HALO_TH=patch[0], TDN_HALO_TW=patch[1])
    for kind in (0, 1):
        o = plan(ops, kind, N, H, W, Cin, Cout, 3, 1, 1)
        assert o[8] == 105 and o[11] == patch[0] * 1000 + patch[1], o
    check_fwd(ops, p, H16, "f16 halo3 patches", "f16 halo patch %s" % (patch,))
    check_dgrad(ops, p, H16, "f16 halo3 patches", "f16 halo patch %s" % (patch,))


def epilogue_modes(ops, dtype, N, H, W, Cin, C_, kf, route):
    """ADD_UP2X forward (k = kf, Cin -> C_, bias, ReLU) and ADD_SUMPOOL2 dgrad (3x3, C_ -> C_), both stores."""
    x = C.q(det_tensor((N, Cin, H, W), 51, -1, 1, bf16=False), dtype)
    w = C.q(det_tensor((C_, Cin, kf, kf), 52, -0.2, 0.2, bf16=False), dtype)
    bias = det_tensor((C_,), 54, -0.5, 0.5, bf16=False)
    coarse = C.q(det_tensor((N, C_, H // 2, W // 2), 53, -1, 1, bf16=False), dtype)
    bound = B.fwd_bound(x, w, 1, kf // 2, None, bias, coarse, "up2x", True)
    for f32 in (True, False):
        y = ops.conv2d_fwd(nhwc(x, dtype), pack_w(w, dtype), kf, 1, kf // 2, None, bias.cuda(), nhwc(coarse, dtype),
                           ops.ADD_UP2X, True, out_f32=f32)
        within(route + " up2x", nchw(y), bound, torch.float32 if f32 else dtype, route + " up2x f32=%s" % f32)
    g = C.q(det_tensor((N, C_, H, W), 55, -1, 1, bf16=False), dtype)
    w3 = C.q(det_tensor((C_, C_, 3, 3), 56, -0.2, 0.2, bf16=False), dtype)
    fine = C.q(det_tensor((N, C_, 2 * H, 2 * W), 57, -1, 1, bf16=False), dtype)
    bound = B.dgrad_bound(g, w3, (H, W), 1, 1, fine, "sumpool")
    for f32 in (True, False):
        dx = ops.conv2d_dgrad(nhwc(g, dtype), pack_wd(w3, dtype), (H, W), 3, 1, 1, nhwc(fine, dtype), ops.ADD_SUMPOOL2,
                              None, out_f32=f32)
        within(route + " sumpool", nchw(dx), bound, torch.float32 if f32 else dtype, route + " sumpool f32=%s" % f32)


def test_halo_dilation_and_fpn_epilogues_f16(ops):
    N, H, W, C_ = C.HALO_EPI_SHAPE
    knobs(TDN_HALO_CFG3=5)
    assert plan(ops, 0, N, H, W, C_, C_, 3, 1, 2)[8] == 105 and plan(ops, 1, N, H, W, C_, C_, 3, 1, 2)[8] == 105
    assert plan(ops, 0, N, H, W, C_, C_, 3, 1, 1)[8] == 105 and plan(ops, 1, N, H, W, C_, C_, 3, 1, 1)[8] == 105
    p = C.conv_problem("f16", N, H, W, C_, C_, 3, 1, 2, 2)
    check_fwd(ops, p, H16, "f16 halo3 dilation 2", "f16 halo dilation 2")
    check_dgrad(ops, p, H16, "f16 halo3 dilation 2", "f16 halo dilation 2")
    epilogue_modes(ops, H16, N, H, W, C_, C_, 3, "f16 halo3")


# ---- part 3: the other routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.GROUPED)
def test_grouped_conv_f16(ops, case):
    N, H, W, Cc, G, k, s = case
    cpg = Cc // G
    x = C.q(det_tensor((N, Cc, H, W), 91, -1, 1, bf16=False), H16).requires_grad_(True)
    w = C.q(det_tensor((Cc, cpg, k, k), 92, -0.3, 0.3, bf16=False), H16).requires_grad_(True)
    # a BN with unit variance whose gamma is in eighths: a 4-bit factor times an 11-bit weight is exact in fp32, so the
    # folded operand fp16(scale * w) is the same number whether it is formed with one rounding or with two
    gamma = ((det_tensor((Cc,), 93, 0.5, 1.5, bf16=False) * 8).round() / 8).requires_grad_(True)
    mean = det_tensor((Cc,), 95, -0.2, 0.2, bf16=False)
    beta = det_tensor((Cc,), 94, -0.5, 0.5, bf16=False).requires_grad_(True)
    invstd = torch.ones(Cc)
    scale = gamma.detach().clone()
    shift = beta.detach() - mean * scale
    conv = F.conv2d(x, w, None, s, k // 2, 1, G)
    pre = (conv - mean.view(1, -1, 1, 1)) * (gamma * invstd).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    wf, wd = ops.pack_gconv_weight(w.detach().cuda(), G, scale.cuda(), True, H16)
    assert wf.dtype == H16
    xd, wdt = x.detach(), w.detach()
    bound = B.fwd_bound(xd, wdt, s, k // 2, scale, shift, relu=True, groups=G)
    for f32 in (True, False):
        y = ops.gconv2d_fwd(nhwc(xd, H16), wf, G, k, s, k // 2, scale.cuda(), shift.cuda(), relu=True, out_f32=f32)
        within("f16 grouped fwd", nchw(y), bound, torch.float32 if f32 else H16, "f16 gconv2d_fwd %s f32=%s" % (case, f32))
    g = C.q(det_tensor(tuple(pre.shape), 97, -1, 1, bf16=False), H16)
    pre.backward(g)
    w_eff = C.q(wdt * scale.view(-1, 1, 1, 1), H16)
    bound = B.dgrad_bound(g, w_eff, (H, W), s, k // 2, groups=G)
    for f32 in (True, False):
        dx = ops.gconv2d_dgrad(nhwc(g, H16), wd, G, (H, W), k, s, k // 2, out_f32=f32)
        within("f16 grouped dgrad", nchw(dx), bound, torch.float32 if f32 else H16, "f16 gconv2d_dgrad %s f32=%s" % (case, f32))
    dw, dg, db = ops.gconv2d_wgrad(nhwc(xd, H16), nhwc(g, H16), wf, G, k, s, k // 2, scale.cuda(), mean.cuda(),
                                   invstd.cuda())
    assert tuple(dw.shape) == (Cc, k, k, cpg)
    assert rel_l2(dg.cpu(), gamma.grad) <= 1e-3 and rel_l2(db.cpu(), beta.grad) <= 1e-3
    within("f16 grouped wgrad", dw.cpu().permute(0, 3, 1, 2), B.wgrad_bound(xd, g, w.shape, s, k // 2, scale, groups=G),
           torch.float32, "f16 gconv2d_wgrad %s" % (case,))


@pytest.mark.parametrize("case", C.DILATED)
def test_dilated_conv_f16(ops, case):
    N, H, W, Cin, Cout, d, s = case
    knobs(TDN_HALO=0)
    p = C.conv_problem("f16", N, H, W, Cin, Cout, 3, s, d, d)
    check_fwd(ops, p, H16, "f16 dilated", "f16 dilated %s" % (case,))
    check_dgrad(ops, p, H16, "f16 dilated", "f16 dilated %s" % (case,))
    dw, _, db = ops.conv2d_wgrad(nhwc(p.x, H16), nhwc(p.g, H16), pack_w(p.w, H16), 3, s, d)
    within("f16 dilated wgrad", dw.cpu().permute(0, 3, 1, 2), B.wgrad_bound(p.x, p.g, p.w.shape, s, d, dilation=d),
           torch.float32, "f16 dilated dw %s" % (case,))
    assert rel_l2(db.cpu(), p.g.sum((0, 2, 3))) <= 1e-3


def test_generic_fpn_epilogues_f16(ops):
    N, H, W, C_ = C.EPI_SHAPE
    knobs(TDN_HALO=0)
    epilogue_modes(ops, H16, N, H, W, 128, C_, 1, "f16 generic")


# ---- part 4: range edges with exactly known answers ------------------------------------------------------------------------------
def same_bits(got, want, exact, plants, what):
    """``got`` NHWC GPU tensor of a 16-bit type, ``want`` NCHW CPU tensor of that type: equal bit for bit."""
    got = got.cpu().permute(0, 3, 1, 2).contiguous()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    bad = (C.bits16(got) != C.bits16(want)).nonzero()
    if len(bad):
        names = {ch: n for n, _, ch in plants}
        rows = ["channel %d (%s) pixel (%d, %d): exact %.10g stored as %r (0x%04x), must be %r (0x%04x)" % (
            i[1], names[i[1]], i[2], i[3], float(exact[tuple(i)]), float(got[tuple(i)]), int(C.bits16(got)[tuple(i)]),
            float(want[tuple(i)]), int(C.bits16(want)[tuple(i)])) for i in bad[:8].tolist()]
        raise AssertionError("%s: %d of %d stored values differ from the one correct rounding:\n  %s" % (
            what, len(bad), want.numel(), "\n  ".join(rows)))


def edge_fwd_check(ops, dtname, k, n, what, relu=0):
    dtype = C.DTYPES[dtname]
    e = C.edge_fwd(dtname, k, n, relu=relu)
    args = (nhwc(e.x, dtype), pack_w(e.w, dtype), k, 1, k // 2, e.scale.cuda(), e.shift.cuda(), None, ops.ADD_NONE, relu)
    y32 = ops.conv2d_fwd(*args, out_f32=True)
    if relu == 0:
        assert torch.equal(nchw(y32), e.exact.float()), what + ": the fp32 result is not the exact sum"
    same_bits(ops.conv2d_fwd(*args), C.expected16(e.exact, dtype, relu), e.exact, e.plants, what + " forward")


def edge_dgrad_check(ops, dtname, k, n, what):
    dtype = C.DTYPES[dtname]
    e = C.edge_dgrad(dtname, k, n)
    args = (nhwc(e.g, dtype), pack_wd(e.w_eff, dtype), (8, 8), k, 1, k // 2, nhwc(e.add, dtype), ops.ADD_SAME, None)
    assert torch.equal(nchw(ops.conv2d_dgrad(*args, out_f32=True)), e.exact.float()), what + ": fp32 dgrad is not the exact sum"
    same_bits(ops.conv2d_dgrad(*args), C.expected16(e.exact, dtype), e.exact, e.plants, what + " dgrad")


@pytest.mark.parametrize("tile", list(C.EDGE_TILES))
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_edge_store_generic_tiles(ops, dtname, k, tile):
    n = C.EDGE_TILES[tile]
    force_tile(ops, tile, [0], (1, 8, 8, 64, n, k, 1, k // 2))
    force_tile(ops, tile, [1], (1, 8, 8, n, 64, k, 1, k // 2))
    what = "%s %dx%d tile %d" % (dtname, k, k, tile)
    edge_fwd_check(ops, dtname, k, n, what)
    edge_dgrad_check(ops, dtname, k, n, what)


@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_edge_store_halo(ops, dtname):
    cfg, n = C.EDGE_HALO3
    knobs(TDN_HALO_CFG3=cfg)
    assert plan(ops, 0, 1, 8, 8, 64, n, 3, 1, 1)[8] == 100 + cfg and plan(ops, 1, 1, 8, 8, n, 64, 3, 1, 1)[8] == 100 + cfg
    edge_fwd_check(ops, dtname, 3, n, "%s halo3 cfg %d" % (dtname, cfg))
    edge_dgrad_check(ops, dtname, 3, n, "%s halo3 cfg %d" % (dtname, cfg))
    cfg, n = C.EDGE_HALO1
    knobs(TDN_HALO=3, TDN_HALO_CFG1=cfg)
    assert plan(ops, 0, 1, 8, 8, 64, n, 1, 1, 0)[8] == 100 + cfg and plan(ops, 1, 1, 8, 8, n, 64, 1, 1, 0)[8] == 100 + cfg
    edge_fwd_check(ops, dtname, 1, n, "%s halo1 cfg %d" % (dtname, cfg))
    edge_dgrad_check(ops, dtname, 1, n, "%s halo1 cfg %d" % (dtname, cfg))


def block_weights(dtype, Cm, seed):
    """conv2 / conv3 weights and affines of a bottleneck whose conv1 is under test."""
    w2 = (det_tensor((Cm, 3, 3, Cm), seed + 3) * (2.0 / (9 * Cm)) ** 0.5).to(dtype).cuda()
    w3 = (det_tensor((4 * Cm, 1, 1, Cm), seed + 4) * (2.0 / Cm) ** 0.5).to(dtype).cuda()
    one, zero = torch.ones(Cm, device="cuda"), torch.zeros(Cm, device="cuda")
    return w2, w3, [one, zero, torch.ones(4 * Cm, device="cuda"), torch.zeros(4 * Cm, device="cuda")]


@pytest.mark.parametrize("bit_planes", [False, True])
@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_edge_store_bottleneck_h1(ops, dtname, bit_planes):
    """The one-launch bottleneck's stored h1 = ReLU(scale1 * conv1(x) + shift1), without and with the ReLU bit planes."""
    dtype = C.DTYPES[dtname]
    N, H, W, Cm = C.EDGE_BLOCK
    assert ops.bottleneck_supported(H, W, Cm)
    e = C.edge_fwd(dtname, 1, Cm, 4 * Cm, H, W, 1)
    w2, w3, aff = block_weights(dtype, Cm, 600)
    bits = ops.bottleneck_bit_planes(N, H, W, Cm, torch.device("cuda")) if bit_planes else None
    h1, _, _ = ops.bottleneck_fwd(nhwc(e.x, dtype), pack_w(e.w, dtype), w2, w3, [e.scale.cuda(), e.shift.cuda()] + aff,
                                  bits=bits)
    same_bits(h1, C.expected16(e.exact, dtype, 1), e.exact, e.plants, "%s bottleneck h1" % dtname)


@pytest.mark.parametrize("route,k,n", [("generic", 1, 64), ("generic", 3, 64), ("halo3 cfg 5", 3, 128)])
@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_relu6_knee_of_a_16_bit_store(ops, dtname, route, k, n):
    """Exactly known values through the knee: [TOP, 6) stores as TOP (5.99609375 / 5.96875), never as 6.0; 6 and up
    as exactly 6."""
    if route == "generic":
        knobs(TDN_HALO=0)
        assert plan(ops, 0, 1, 8, 8, 64, n, k, 1, k // 2)[8] < 100
    else:
        knobs(TDN_HALO_CFG3=5)
        assert plan(ops, 0, 1, 8, 8, 64, n, k, 1, k // 2)[8] == 105
    edge_fwd_check(ops, dtname, k, n, "%s relu6 %dx%d %s" % (dtname, k, k, route), relu=2)


SUBNORMAL_ROUTES = {"library choice": {}, "tile 0": {"TDN_GEMM_CFG": 0}, "tile 25": {"TDN_GEMM_CFG": 25},
                    "halo1 cfg 2": {"TDN_HALO": 3, "TDN_HALO_CFG1": 2}}


@pytest.mark.parametrize("route", list(SUBNORMAL_ROUTES))
@pytest.mark.parametrize("k", [1, 3])
def test_subnormal_f16_operands_are_kept(ops, k, route):
    """fp16 operands below 2^-14 (loss-scaled cotangents) entering the matrix cores: m * 2^-24 against weights in
    {+-1, +-2}; the sums are exact in fp32, so the fp32-output forward and input gradient must EQUAL the fp64
    reference.  A kernel (or matrix core) that flushed subnormal A/B operands would return zeros here.
    Measured on MI355X (gfx950): kept — see profiles/fp16_conv_edges.md."""
    knobs(**SUBNORMAL_ROUTES[route])
    v, w, fwd, dg = C.subnormal_operands(k)
    y = ops.conv2d_fwd(nhwc(v, H16), pack_w(w, H16), k, 1, k // 2, out_f32=True)
    dx = ops.conv2d_dgrad(nhwc(v, H16), pack_wd(w, H16), (8, 8), k, 1, k // 2, out_f32=True)
    lost_y = float((nchw(y).double() - fwd).abs().max() / fwd.abs().max())
    lost_dx = float((nchw(dx).double() - dg).abs().max() / dg.abs().max())
    print("subnormal operands %dx%d %s: max |err| / max |ref| forward %.3g, dgrad %.3g" % (k, k, route, lost_y, lost_dx))
    RATIOS["f16 subnormal operands, relative loss (0 = kept)"] = max(
        RATIOS.get("f16 subnormal operands, relative loss (0 = kept)", 0.0), lost_y, lost_dx)
    assert torch.equal(nchw(y).double(), fwd), "forward lost subnormal operands: relative error %.3g" % lost_y
    assert torch.equal(nchw(dx).double(), dg), "dgrad lost subnormal operands: relative error %.3g" % lost_dx


# ---- part 5: poison confinement -------------------------------------------------------------------------------------------------
def int_view(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def confined(clean, dirty, field, what, must_be_nonfinite=True):
    """clean / dirty: NHWC GPU results; field: bool (N, H, W) on the CPU — the pixels the poison may reach."""
    f = field.cuda()
    assert tuple(f.shape) == tuple(clean.shape[:3])
    same = (int_view(clean) == int_view(dirty)).all(dim=3)
    leak = (~same & ~f).nonzero()
    assert len(leak) == 0, "%s: %d pixels outside the receptive field changed, first (n, h, w) = %s" % (
        what, len(leak), leak[0].tolist())
    if must_be_nonfinite:
        inside = dirty[f]
        assert inside.numel() > 0 and not bool(torch.isfinite(inside).any()), \
            "%s: %d finite values inside the receptive field" % (what, int(torch.isfinite(inside).sum()))


POISONS = [("nan", float("nan")), ("inf", float("inf"))]


def poison_conv(ops, dtname, shape, k, s, what):
    """Forward and dgrad of a plain conv (affine only), both stores: NaN and +inf at three positions each."""
    dtype = C.DTYPES[dtname]
    N, H, W, Cin, Cout = shape
    x, w, scale, shift, g, w_eff = C.poison_problem(dtname, N, H, W, Cin, Cout, k, s)
    pad = k // 2
    Ho, Wo = C.conv_out(H, k, s, pad), C.conv_out(W, k, s, pad)
    xg, gg, wf, wd = nhwc(x, dtype), nhwc(g, dtype), pack_w(w, dtype), pack_wd(w_eff, dtype)
    sc, sh = scale.cuda(), shift.cuda()
    for f32 in (True, False):
        clean = ops.conv2d_fwd(xg, wf, k, s, pad, sc, sh, out_f32=f32)
        assert bool(torch.isfinite(clean).all())
        for pname, pos in C.poison_positions(N, H, W):
            field = C.field_fwd((N, H, W), pos, k, s, pad)
            for vname, val in POISONS:
                xd = xg.clone()
                xd[pos[0], pos[1], pos[2], C.POISON_CH] = val
                confined(clean, ops.conv2d_fwd(xd, wf, k, s, pad, sc, sh, out_f32=f32), field,
                         "%s forward, %s at the %s pixel %s, f32=%s" % (what, vname, pname, pos, f32))
        clean = ops.conv2d_dgrad(gg, wd, (H, W), k, s, pad, out_f32=f32)
        assert bool(torch.isfinite(clean).all())
        for pname, pos in C.poison_positions(N, Ho, Wo):
            field = C.field_dgrad((N, H, W), pos, k, s, pad)
            for vname, val in POISONS:
                gd = gg.clone()
                gd[pos[0], pos[1], pos[2], C.POISON_CH] = val
                confined(clean, ops.conv2d_dgrad(gd, wd, (H, W), k, s, pad, out_f32=f32), field,
                         "%s dgrad, %s at the %s pixel %s, f32=%s" % (what, vname, pname, pos, f32))


@pytest.mark.parametrize("tile", C.POISON_TILES)
@pytest.mark.parametrize("geom", C.P1_GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_poison_confined_generic(ops, dtname, geom, tile):
    k, s = geom
    N, H, W, Cin, Cout = C.P1_SHAPE
    force_tile(ops, tile, [0, 1], (N, H, W, Cin, Cout, k, s, k // 2))
    poison_conv(ops, dtname, C.P1_SHAPE, k, s, "%s %dx%d s%d tile %d" % (dtname, k, k, s, tile))


@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_poison_confined_halo(ops, dtname):
    cfg, case = C.POISON_HALO
    N, H, W, Cin, Cout = case
    knobs(TDN_HALO_CFG3=cfg)
    for kind in (0, 1):
        o = plan(ops, kind, N, H, W, Cin, Cout, 3, 1, 1)
        assert o[8] == 100 + cfg and (H % (o[11] // 1000) != 0 or W % (o[11] % 1000) != 0), "an overhanging patch: %s" % o
    poison_conv(ops, dtname, case, 3, 1, "%s halo cfg %d" % (dtname, cfg))


@pytest.mark.parametrize("dtname", list(C.DTYPES))
def test_poison_confined_bottleneck_h1(ops, dtname):
    """x poisoned, h1 checked (the 1x1 field: the pixel itself).  h1 passes a ReLU, and the project leaves NaN through
    fmaxf unspecified: confinement is asserted for NaN and +inf, "non-finite inside" only for +inf, which positive
    weights on the poisoned channel and positive scales carry to +inf, a value the ReLU keeps."""
    dtype = C.DTYPES[dtname]
    N, H, W, Cm = C.POISON_BLOCK
    assert ops.bottleneck_supported(H, W, Cm)
    x = torch.relu(det_tensor((N, H, W, 4 * Cm), 611)).to(dtype).cuda()
    w1 = det_tensor((Cm, 1, 1, 4 * Cm), 612) * (2.0 / (4 * Cm)) ** 0.5
    w1[:, :, :, C.POISON_CH] = w1[:, :, :, C.POISON_CH].abs().clamp(min=0.01)
    w1 = w1.to(dtype).cuda()
    w2, w3, aff = block_weights(dtype, Cm, 610)
    sc1 = det_tensor((Cm,), 613, 0.5, 1.5, bf16=False).cuda()
    sh1 = det_tensor((Cm,), 614, -0.1, 0.1, bf16=False).cuda()
    clean, _, _ = ops.bottleneck_fwd(x, w1, w2, w3, [sc1, sh1] + aff)
    clean = clean.clone()
    assert bool(torch.isfinite(clean).all())
    for pname, pos in C.poison_positions(N, H, W):
        field = torch.zeros(N, H, W, dtype=torch.bool)
        field[pos] = True
        for vname, val in POISONS:
            xd = x.clone()
            xd[pos[0], pos[1], pos[2], C.POISON_CH] = val
            h1, _, _ = ops.bottleneck_fwd(xd, w1, w2, w3, [sc1, sh1] + aff)
            confined(clean, h1, field, "%s bottleneck h1, %s at the %s pixel %s" % (dtname, vname, pname, pos),
                     must_be_nonfinite=vname == "inf")
