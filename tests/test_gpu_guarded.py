"""The parity cases of the GPU suite once more, under guard-banded, poisoned outputs and exact-size workspaces
(tests/guard_util.py): a store outside an output tensor, an output element no kernel wrote, a workspace overrun and a
finalize launch that reads scratch this call did not write all turn into assertions here.

The test functions of the other GPU modules are imported as MODULES and called with ``ops`` under the guard, so their
own references, assertions and tolerances stay in force; with NaN / 0x5A in every fresh output, each of their
comparisons is also a "was it written" check.  After every call ``guard.check()`` must come back empty.

LIMITS (see guard_util.py): a store further than max(1 MiB, one image row) from the tensor, device globals (the zero /
sink pages of conv_block.hip: covered by static_asserts there) and LDS are out of reach.  The input-side tests copy the
operands of the tiled readers into NaN bands and demand bit-identical outputs: a stray read is seen only if the value
read reaches an output — a read whose result is discarded (``ok ? v : 0``) is legal and stays invisible.

The last two tests of this file check that the run reached every allocating entry point of ops.py and an exact-size
workspace for every ``tdn_*_workspace`` of include/tdn.h: they count what the tests above did IN THIS RUN, so run the
file as a whole.
"""
import collections
import functools
import inspect
import os
import re

import pytest
import torch

import bound_util as BU
import elementwise_cases as EC
import elementwise_ref as EWR
import guard_util as G
import test_gpu_block as BL
import test_gpu_box as BX
import test_gpu_elementwise as EW
import test_gpu_gn as GN
import test_gpu_halo as HL
import test_gpu_kernels as K
import test_gpu_proposals as PR
import test_gpu_roi_align as RA
import test_gpu_staging as ST
import test_gpu_wgrad_plans as WP
from golden_util import det_tensor, rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTERED = collections.Counter()     # ops function -> calls that returned under the guard, this run
PROXY_SEEN = collections.Counter()  # ops function -> allocations / workspaces the proxy made for it that were checked
WS_SEEN = {}                        # ops function -> (bytes asked, bytes given) of a workspace that came back clean
# allocates planes that a LATER call fills (and the head tests drop the third one): their being written is asserted
# where they are used (the block tests unpack them; test_caller_buffers_* passes must-write planes explicitly)
FILLED_LATER = ("bottleneck_bit_planes",)


def _public(ops):
    return sorted(n for n, v in vars(ops).items()
                  if inspect.isfunction(v) and v.__module__ == ops.__name__ and not n.startswith("_"))


class Guard(G.GuardAlloc):
    not_must_write = ()       # label prefixes of outputs that may legitimately hold the poison pattern (a stored NaN)

    def alloc(self, shape, dtype=torch.float32, device=None, interior="poison", label="?", must_write=True,
              band_byte=G.BAND_BYTE):
        if label.split(":")[0] in FILLED_LATER or label.startswith(tuple(self.not_must_write)):
            must_write = False
        return super().alloc(shape, dtype, device, interior, label, must_write, band_byte)

    def clean(self):
        """check() must find nothing; remembers the exact-size workspaces that came back clean."""
        log, self.ws_log = self.ws_log, []
        for r in self.recs:                 # the proxy's own labels end in "@<line of ops.py>" or "workspace"
            if re.search(r"(@\d+|: workspace)$", r.label):
                PROXY_SEEN[r.label.split(":")[0]] += 1
        found = self.check()
        assert not found, "\n".join(found)
        for op, asked, given in log:
            WS_SEEN.setdefault(op, (asked, given))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from torch_detection_amd import ops as _ops
    from torch_detection_amd import _lib
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd
    return torch_detection_amd


@pytest.fixture()
def guard(ops, monkeypatch):
    """``ops`` under the guard for one test: guarded torch.empty / zeros / full / empty_like, exact workspaces, a call
    counter on every public function, and the TDN_* environment restored afterwards (the reused tests set it)."""
    g = Guard()
    G.install(monkeypatch, ops, g)

    def counted(name, fn):
        @functools.wraps(fn)
        def wrapper(*a, **kw):
            n0 = len(g.recs)
            try:
                out = fn(*a, **kw)
                ENTERED[name] += 1          # counted on a successful return: a refused call launched nothing
                return out
            except Exception:
                # a call that refuses its arguments (pytest.raises in the reused tests) launched nothing: what it had
                # allocated before raising is not an output
                g.retired.extend(r.buf for r in g.recs[n0:])
                del g.recs[n0:]
                raise
        return wrapper

    for name in _public(ops):
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))
    saved = {k: v for k, v in os.environ.items() if k.startswith("TDN_")}
    for k in saved:
        del os.environ[k]
    yield g
    for k in [k for k in os.environ if k.startswith("TDN_")]:
        del os.environ[k]
    os.environ.update(saved)
    torch.cuda.synchronize()


def _no_tdn_env():
    for k in [k for k in os.environ if k.startswith("TDN_")]:
        del os.environ[k]


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert not bool(torch.isnan(a.float()).any()), "%s: NaN in the result" % what
    assert torch.equal(_bits(a), _bits(b)), "%s: %d of %d elements differ" % (what, int((_bits(a) != _bits(b)).sum()),
                                                                            a.numel())


# ---- positive controls: the guard sees device memory ----------------------------------------------------------
def test_control_short_payload_is_reported(ops, guard):
    """A legitimately written output registered one row too short: its last row counts as band, check() reports it."""
    x = K.nhwc(det_tensor((1, 64, 13, 21), 1, -1, 1))
    y = ops.subsample2_fwd(x)                                   # (1, 7, 11, 64), every element written
    row = 11 * 64 * 2
    guard.shorten(y, y.numel() * 2 - row)
    found = guard.check()
    assert len(found) == 1 and "subsample2_fwd" in found[0] and "UPPER band" in found[0], found
    first, last = (int(v) for v in re.search(r"payload offsets (-?\d+) \.\. (-?\d+)", found[0]).groups())
    assert 6 * row <= first < 6 * row + 16 and 7 * row - 16 <= last < 7 * row, found      # the last row, nothing else


def test_control_untouched_tensor_is_reported(ops, guard):
    """A guarded tensor no kernel touched, registered as "must be fully written": check() reports every element."""
    t = guard.alloc((3, 5, 7, 8), torch.bfloat16, torch.device("cuda"), label="control: t")
    i = guard.alloc((40,), torch.int64, torch.device("cuda"), label="control: i")
    found = guard.check()
    assert len(found) == 2 and "control: t: 840 of 840 elements never written" in found[0], found
    assert "control: i: 40 of 40 elements never written" in found[1], found
    assert t.data_ptr() % 512 == 0 and i.data_ptr() % 512 == 0


# ---- conv forward / dgrad -------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", list(K.GEMM_CFGS))
@pytest.mark.parametrize("case", K.CONV_CASES)
def test_conv_fwd(ops, guard, case, tile):
    K.test_conv_fwd(ops, case, tile)
    guard.clean()


@pytest.mark.parametrize("tile", list(K.GEMM_CFGS))
@pytest.mark.parametrize("case", K.CONV_CASES)
def test_conv_dgrad(ops, guard, case, tile, monkeypatch):
    K.test_conv_dgrad(ops, case, tile, monkeypatch)
    guard.clean()


def test_conv_epilogue_up2x_and_sumpool(ops, guard):
    K.test_conv_epilogue_up2x_and_sumpool(ops)
    guard.clean()


@pytest.mark.parametrize("case", [(2, 14, 18, 64, 128, 2, 1), (1, 13, 21, 128, 64, 4, 1), (1, 16, 20, 64, 64, 2, 2),
                                  (1, 9, 9, 256, 256, 8, 1)])
def test_dilated_conv(ops, guard, case):
    K.test_dilated_conv(ops, case)
    guard.clean()


@pytest.mark.parametrize("case", HL.CASES3)
def test_halo_conv3x3_forced_configs(ops, guard, case):
    """Every forced halo configuration that applies to the shape (the reused test skips the others before it launches
    anything with them: counted here, not skipped)."""
    ran = 0
    for cfg in sorted(HL.CFG3):
        _no_tdn_env()
        try:
            HL.test_halo_conv3x3_fwd_dgrad(ops, case, cfg)
            ran += 1
        except pytest.skip.Exception:
            pass
        guard.clean()
    assert ran >= 1, "no halo configuration took %s" % (case,)


@pytest.mark.parametrize("patch", [(8, 16), (3, 42), (10, 12), (16, 8), (4, 32), (2, 50)])
def test_halo_patch_shapes(ops, guard, patch):
    HL.test_halo_patch_shapes(ops, patch)
    guard.clean()


def test_halo_dilated_and_epilogue_modes(ops, guard):
    HL.test_halo_dilated_and_epilogue_modes(ops)
    guard.clean()


@pytest.mark.parametrize("case", HL.CASES1)
def test_halo_conv1x1_forced_configs(ops, guard, case):
    ran = 0
    for cfg in sorted(HL.CFG1):
        _no_tdn_env()
        try:
            HL.test_halo_conv1x1(ops, case, cfg)
            ran += 1
        except pytest.skip.Exception:
            pass
        guard.clean()
    assert ran >= 1, "no 1x1 halo configuration took %s" % (case,)


# ---- weight gradients -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CONV_CASES + K.T9_CASES)
@pytest.mark.parametrize("bn", [True, False])
def test_conv_wgrad(ops, guard, case, bn, monkeypatch):
    K.test_conv_wgrad(ops, case, bn, monkeypatch)
    guard.clean()


GROUP_MEMBERS = [(2, 40, 48, 64, 256, 3, 1), (2, 40, 48, 64, 64, 3, 1), (1, 7, 7, 192, 384, 3, 1),
                 (1, 13, 21, 128, 128, 3, 1), (2, 25, 42, 128, 128, 3, 2), (1, 25, 43, 64, 128, 1, 2),
                 (2, 10, 12, 256, 64, 1, 1), (1, 12, 16, 256, 512, 1, 2)] + \
    [(1, 20, 24, 64, 256, 1, 1)] * 14 + [(1, 13, 21, 64, 256, 1, 1)] * 14


def test_wgrad_group_many_members(ops, guard, monkeypatch):
    """One tdn_wgrad_group call of 36 members: more than FIN_MAXI = 30 (two finalize launches), 28 of one tile shape
    (more than WG_MAXI = 26: two gradient launches of that shape), tap-per-tile and nine-tap members, split-K and
    direct members, BN and bias mode — against the same members launched one by one.  Both are fp32 sums of the same
    16-bit products in a different split: the module's wgrad tolerance (rel-L2 <= 1e-3, test_gpu_kernels.py) bounds
    the difference.  Every dw / dgamma / dbeta is a poisoned, guard-banded tensor; the slabs, column sums and dot
    partials live in a NaN-filled workspace of exactly tdn_wgrad_group_workspace() bytes."""
    monkeypatch.setenv("TDN_WGRAD9", "1")
    items, outs, keep, singles = [], [], [], []
    for i, (N, H, W, Cin, Cout, k, s) in enumerate(GROUP_MEMBERS):
        Ho, Wo = ops.conv_out_size(H, k, s, k // 2), ops.conv_out_size(W, k, s, k // 2)
        x = K.nhwc(det_tensor((N, Cin, H, W), 500 + i, -1, 1))
        g = K.nhwc(det_tensor((N, Cout, Ho, Wo), 600 + i, -1, 1))
        wf = K.pack_w(det_tensor((Cout, Cin, k, k), 700 + i, -0.2, 0.2))
        bn = ()
        if i % 2 == 0:
            bn = tuple(det_tensor((Cout,), 800 + 3 * i + j, lo, hi, bf16=False).cuda()
                       for j, (lo, hi) in enumerate(((0.5, 1.5), (-0.2, 0.2), (0.7, 1.4))))
        it, dw, dg, db = ops.conv2d_wgrad_item(x, g, wf, k, s, k // 2, *bn)
        items.append(it)
        outs.append((dw, dg, db))
        keep.append((x, g, wf, bn))
    per, tot = ops.wgrad_group_plan(items)
    kinds = {p[0] for p in per}               # 0: tap-per-tile; 1, 2: the nine-tap kernel's 128- / 64-wide tiles
    assert 0 in kinds and kinds & {1, 2} and kinds <= {0, 1, 2}, "tap-per-tile and nine-tap members: %s" % kinds
    assert any(p[3] > 1 and p[5] == 0 for p in per) and any(p[5] == 1 for p in per), "split-K and direct members"
    assert tot[1] == 2, tot                                          # more than FIN_MAXI members: two finalize launches
    # more than WG_MAXI = 26 members in one gradient launch list: the 28 1x1 64->256 members share kernel and tile,
    # and the group without the last two of them needs exactly one gradient launch less
    tiles = collections.Counter((p[0], p[1], p[2]) for p in per)
    assert max(tiles.values()) > 26, tiles
    assert GROUP_MEMBERS[-1] == GROUP_MEMBERS[-2] and per[-1][:3] == per[-2][:3] == list(max(tiles, key=tiles.get))
    _, tot26 = ops.wgrad_group_plan(items[:-2])
    assert tot[0] == tot26[0] + 1, (tot, tot26, per)
    ops.wgrad_group(items, torch.bfloat16, torch.device("cuda"))
    (op, asked, given), = guard.ws_log                               # this call's workspace, nothing else
    assert op == "wgrad_group" and asked > 0 and 0 <= given - asked < 16, guard.ws_log
    guard.clean()
    for (x, g, wf, bn), (N, H, W, Cin, Cout, k, s) in zip(keep, GROUP_MEMBERS):
        singles.append(ops.conv2d_wgrad(x, g, wf, k, s, k // 2, *bn))
    guard.clean()
    for i, (a, b) in enumerate(zip(outs, singles)):
        for nm, u, v in zip(("dw", "dgamma", "dbeta"), a, b):
            assert (u is None) == (v is None)
            if u is not None:
                assert not bool(torch.isnan(u).any()), (i, nm)
                assert rel_l2(u.cpu(), v.cpu()) <= K.TOL, (i, GROUP_MEMBERS[i], nm)


@pytest.mark.parametrize("case", WP.WC.CASES, ids=WP.WC.IDS)
def test_wgrad_plan_case(ops, guard, case, monkeypatch):
    """Every forced plan of tests/wgrad_cases.py (tile shapes, split layouts with idle workgroup slots, the 256-split
    cap, stem / grouped / nine-tap members, one mixed group) with its own oracle checks, under poisoned, guard-banded
    dw / dgamma / dbeta and a NaN-filled workspace of exactly tdn_wgrad_group_workspace() bytes: a finalize pass that
    reads an idle slot's slab or colsum, or a split that writes past its region, is a NaN or a band hit."""
    WP.run_case(ops, case, monkeypatch)
    assert guard.ws_log, "no workspace was handed out"
    for op, asked, given in guard.ws_log:
        assert op == "wgrad_group" and asked > 0 and 0 <= given - asked < 16, guard.ws_log
    guard.clean()


@pytest.mark.parametrize("case", [(2, 12, 16, 128, 32, 3, 1), (1, 13, 21, 256, 32, 3, 2), (2, 9, 10, 512, 32, 3, 1),
                                  (1, 8, 8, 1024, 32, 3, 2), (1, 10, 12, 128, 2, 3, 1)])
def test_grouped_conv(ops, guard, case):
    K.test_grouped_conv(ops, case)
    guard.clean()


# ---- one-launch blocks ----------------------------------------------------------------------------------------
RAGGED = [s for s in BL.SHAPES if s[1] % 8 or s[2] % 16]
RAGGED_HEAD = [s for s in BL.HEAD_SHAPES if s[1] % 8 or s[2] % 16]
DTYPES = [torch.bfloat16, torch.float16]


def _generic_tiles(monkeypatch):
    monkeypatch.setenv("TDN_GEMM_CFG", "0")       # what test_gpu_block.py's generic_tiles fixture sets
    monkeypatch.setenv("TDN_HALO", "0")


def test_ragged_block_shapes_are_what_they_claim():
    assert len(RAGGED) == 4 and (1, 13, 21) in RAGGED and len(RAGGED_HEAD) == 3


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W", RAGGED)
def test_block_forward(ops, guard, monkeypatch, N, H, W, dtype, C):
    _generic_tiles(monkeypatch)
    BL.test_block_forward(ops, None, N, H, W, dtype, C)
    guard.clean()


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W", RAGGED)
@pytest.mark.parametrize("with_mask3", [True, False])
def test_block_dgrad(ops, guard, monkeypatch, N, H, W, dtype, with_mask3, C):
    _generic_tiles(monkeypatch)
    BL.test_block_dgrad(ops, None, N, H, W, dtype, with_mask3, C)
    guard.clean()


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W", [(1, 16, 32), (2, 13, 21), (1, 17, 40)])
def test_block_relu_bit_planes(ops, guard, monkeypatch, N, H, W, dtype, C):
    _generic_tiles(monkeypatch)
    BL.test_block_relu_bit_planes(ops, None, N, H, W, dtype, C)
    guard.clean()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W", RAGGED + [(1, 100, 168), (2, 100, 168), (1, 31, 50)])
@pytest.mark.parametrize("mode", ["masks", "nomask3", "bits"])
def test_block128_tall_tiles(ops, guard, monkeypatch, N, H, W, dtype, mode):
    _generic_tiles(monkeypatch)
    BL.test_block128_tall_tiles(ops, None, monkeypatch, N, H, W, dtype, mode)
    guard.clean()


def test_block128_layer2_geometry(ops, guard, monkeypatch):
    """100 x 168, one image, C = 128, the 8-row tile: H % 8 and W % 16 are both nonzero, so ragged tiles redirect
    their invalid pixels to the zero / sink pages of conv_block.hip at the second pass's offset."""
    _generic_tiles(monkeypatch)
    BL.test_block_baseline_geometry(ops, None, 0, 100, 168, 128)
    guard.clean()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,W", RAGGED_HEAD)
@pytest.mark.parametrize("with_bits", [False, True])
def test_head_block(ops, guard, monkeypatch, N, H, W, dtype, with_bits):
    _generic_tiles(monkeypatch)
    BL.test_head_block_forward_and_dgrad(ops, None, N, H, W, dtype, with_bits)
    guard.clean()


# ---- stem and elementwise -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 30, 44), (3, 64, 96), (2, 128, 160), (1, 226, 318)])
def test_stem_pool_fused(ops, guard, shape, dtype):
    K.test_stem_pool_fused_equals_two_launches(ops, shape, dtype)      # the uint8 index tensors lose their poison
    guard.clean()


@pytest.mark.parametrize("shape", [(1, 32, 48), (2, 64, 96)])
def test_stem(ops, guard, shape):
    K.test_stem(ops, shape)            # stage_image: the zero halo must really be written (the interior is NaN)
    guard.clean()


@pytest.mark.parametrize("shape", [(2, 16, 24, 64), (1, 15, 21, 64), (1, 8, 8, 128)])
def test_maxpool(ops, guard, shape):
    K.test_maxpool(ops, shape)
    guard.clean()


def test_subsample_and_mask(ops, guard):
    K.test_subsample_and_mask(ops)
    guard.clean()


def test_layout_converters(ops, guard):
    K.test_layout_converters(ops)
    guard.clean()


def test_pack_and_fold(ops, guard):
    K.test_pack_and_fold(ops)
    guard.clean()


# the oracle cases of test_gpu_elementwise.py: every output a poisoned, guard-banded tensor — an overrun at the far end
# of a grid-stride loop (the second-trip cases) lands in a band
@pytest.mark.parametrize("dtype", DTYPES, ids=EC.DT_IDS)
def test_elementwise_rounding(ops, guard, dtype):
    for fn in (EW.test_rounding_to_nhwc, EW.test_rounding_stage_image, EW.test_rounding_pack_conv_weight,
               EW.test_rounding_prepare_group, EW.test_rounding_pack_stem_and_gconv):
        fn(ops, dtype)
        guard.clean()


@pytest.mark.parametrize("dtype", DTYPES, ids=EC.DT_IDS)
def test_elementwise_layouts(ops, guard, dtype):
    for C, groups in EW.GCONV_CASES:
        for k in EW.GCONV_KS:
            for with_scale in (False, True):
                EW.test_pack_gconv_layout(ops, C, groups, k, with_scale, dtype)
    EW.test_pack_stem_layout(ops, dtype)
    for shape in EW.STAGE_SHAPES:
        EW.test_stage_image_every_element(ops, shape, dtype)
    guard.clean()
    for C, hw in EW.CONVERTER_CASES:
        EW.test_converters(ops, C, hw, dtype)
    guard.clean()


@pytest.mark.parametrize("dtype", DTYPES, ids=EC.DT_IDS)
@pytest.mark.parametrize("shape", EC.POOL_SHAPES)
def test_elementwise_maxpool(ops, guard, shape, dtype):
    """The 'special' recipe pools NaNs, and the guard's floating poison is a NaN pattern (guard_util.NAN_BYTE): a NaN
    the kernel stored cannot be told from an element it never wrote.  For that recipe the pool's ``y`` is banded but
    not checked for having been written (the reused test compares every element of it with the oracle anyway)."""
    for kind in EC.POOL_KINDS:
        guard.not_must_write = ("maxpool3x3s2_fwd: y@",) if kind == "special" else ()
        EW.test_maxpool(ops, shape, kind, dtype)
        guard.clean()


@pytest.mark.parametrize("dtype", DTYPES, ids=EC.DT_IDS)
def test_elementwise_subsample_add_clamp_mask(ops, guard, dtype):
    for shape in EW.SUBSAMPLE_SHAPES:
        EW.test_subsample_add_clamp_mask(ops, shape, dtype)
        guard.clean()


@pytest.mark.parametrize("dtype", DTYPES, ids=EC.DT_IDS)
def test_elementwise_channel_affine(ops, guard, dtype):
    for C in EW.AFFINE_FWD_C:
        for act in EW.AFFINE_ACTS:
            EW.test_channel_affine_fwd(ops, C, act, dtype)
        EW.test_channel_affine_relu6_knee(ops, C, dtype)
        guard.clean()
    for C, npix in EC.AFFINE_BWD_CASES:            # every thread layout in an exact-size, NaN-filled workspace
        EW.test_channel_affine_bwd_exact(ops, C, npix, dtype)
        EW.test_channel_affine_bwd_random(ops, C, npix, dtype)
        guard.clean()
    for C, npix in EW.BETA_CASES:                  # the C ABI's accumulate path onto seeded, banded dgamma / dbeta
        EW.test_channel_affine_bwd_beta(ops, C, npix, dtype, lambda t, label: guard.guard_copy(t.cuda(), label))
        guard.clean()


big = EW.big            # the module-scoped fixture of the large inputs and references


@pytest.mark.parametrize("dtype", DTYPES, ids=EC.DT_IDS)
@pytest.mark.parametrize("case", EW.SECOND_TRIP)
def test_elementwise_second_trip(ops, guard, big, case, dtype):
    getattr(EW, "test_second_trip_" + case)(ops, big, dtype)
    guard.clean()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_prepare_group(ops, guard, dtype):
    """The reused test allocates prepare_group's outputs with torch.empty of its own; here they are must-write,
    guard-banded buffers too."""
    K.test_prepare_group_equals_per_layer_calls(ops, dtype)
    guard.clean()
    dev = torch.device("cuda")
    entries, refs = [], []
    for i, (O, I, k) in enumerate([(128, 64, 3), (64, 256, 1), (192, 320, 3)] * 11):        # 33 members: two launches
        w = det_tensor((O, I, k, k), 900 + i, -1, 1, bf16=False).cuda()
        bn = tuple(det_tensor((O,), 950 + 4 * i + j, lo, hi, bf16=False).cuda()
                   for j, (lo, hi) in enumerate(((0.5, 1.5), (-1, 1), (-1, 1), (0.5, 1.5)))) + (1e-5,)
        sc, sh, inv = ops.bn_fold(*bn)
        refs.append((sc, sh, inv) + ops.pack_conv_weight(w, sc, True, dtype))
        entries.append((w, bn, guard.alloc((O, k, k, I), dtype, dev, label="prepare_group: w_fwd[%d]" % i),
                        guard.alloc((I, k, k, O), dtype, dev, label="prepare_group: w_dgrad[%d]" % i),
                        guard.alloc((3, O), torch.float32, dev, label="prepare_group: fold[%d]" % i)))
    ops.prepare_group(entries, dtype)
    guard.clean()
    for (w, bn, wf, wd, fold), (sc, sh, inv, rf, rd) in zip(entries, refs):
        assert torch.equal(fold, torch.stack([sc, sh, inv])) and torch.equal(wf, rf) and torch.equal(wd, rd)


def test_activation_pieces(ops, guard):
    """clamp_max_, act_mask, channel_affine_fwd / _bwd on a ragged pixel count against fp32 / fp64 on the CPU.  The
    16-bit results are one rounding of an fp32 value (2^-7 relative is the module's loose 1-ulp bound, test_gpu_kernels
    .py); dgamma / dbeta are fp32 sums over the pixels: rel-L2 <= 1e-3 like every other affine gradient there."""
    N, C, H, W = 3, 64, 13, 21
    x = det_tensor((N, C, H, W), 1001, -8, 8)
    y = K.nhwc(x)
    guard_y = guard.guard_copy(y, "clamp_max_: y")          # in place on a banded buffer
    assert ops.clamp_max_(guard_y, 6.0) is guard_y
    assert torch.equal(K.nchw(guard_y), x.clamp(max=6.0))
    g = det_tensor((N, C, H, W), 1002, -1, 1)
    for hi in (6.0, float("inf")):
        out = ops.act_mask(K.nhwc(g), y, hi)
        assert torch.equal(K.nchw(out), g * ((x > 0) & (x < hi)).float())
    scale = det_tensor((C,), 1003, 0.5, 1.5, bf16=False)
    shift = det_tensor((C,), 1004, -0.5, 0.5, bf16=False)
    mean = det_tensor((C,), 1005, -0.2, 0.2, bf16=False)
    invstd = det_tensor((C,), 1006, 0.7, 1.4, bf16=False)
    for act in (0, 1, 2):          # every element against the a-priori bound of the oracle (elementwise_ref.py)
        und = EW._affine_fwd_check(ops, x, scale, shift, act, torch.bfloat16, "channel_affine_fwd act %d" % act)[3]
        assert und <= 1e-3 * x.numel()                # elements within E of the ReLU6 knee: at most 0.1 %
    dx, dg, db = ops.channel_affine_bwd(K.nhwc(g), y, scale.cuda(), mean.cuda(), invstd.cuda())
    guard.clean()
    ref_dx, ref_db, ref_dg, _ = EWR.channel_affine_bwd(g, x, scale, mean, invstd, torch.bfloat16)
    EWR.assert_nchw(K.nchw(dx), ref_dx.bits, "dx = bf16(fl32(g * scale))")
    assert rel_l2(db.cpu(), ref_db.v.float()) <= K.TOL
    assert rel_l2(dg.cpu(), ref_dg.v.float()) <= K.TOL
    BU.assert_within(db.cpu(), ref_db, torch.float32, "dbeta")
    BU.assert_within(dg.cpu(), ref_dg, torch.float32, "dgamma")
    # caller buffers: poisoned, guard-banded dgamma / dbeta are overwritten (the C ABI call passes beta = 0)
    dev = torch.device("cuda")
    dg2 = guard.alloc((C,), torch.float32, dev, label="channel_affine_bwd: dgamma=")
    db2 = guard.alloc((C,), torch.float32, dev, label="channel_affine_bwd: dbeta=")
    dx2, _, _ = ops.channel_affine_bwd(K.nhwc(g), y, scale.cuda(), mean.cuda(), invstd.cuda(), dg2, db2)
    guard.clean()
    _same(dg2, dg, "dgamma=")
    _same(db2, db, "dbeta=")
    _same(dx2, dx, "dx")


def test_collate_and_stage(ops, guard, T):
    ST.test_collate_ragged_vs_oracle(T)
    guard.clean()
    # the staged layout: ragged images, flips, both 16-bit types — equal to stage_image of the float batch, whose zero
    # halo test_stem checks; every element of both outputs, halo included, must have lost its poison
    g = torch.Generator().manual_seed(5)
    imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).cuda() for h, w in ((33, 95), (64, 17), (1, 1))]
    means, stds = (102.9801, 115.9465, 122.7717), (58.395, 57.12, 57.375)
    batch = ops.collate_images(imgs, means, stds, [True, False, True])
    assert tuple(batch.shape) == (3, 3, 64, 96)
    for dt in DTYPES:
        st = ops.collate_images(imgs, means, stds, [True, False, True], staged=True, dtype=dt)
        ref = ops.stage_image(batch, dt)
        guard.clean()
        _same(st, ref, "staged collate")
        sc = st.float().cpu()
        assert float(sc[:, :3].abs().sum()) == 0 and float(sc[:, 67:].abs().sum()) == 0
        assert float(sc[:, :, :3].abs().sum()) == 0 and float(sc[:, :, 99:].abs().sum()) == 0
        assert float(sc[..., 3].abs().sum()) == 0


# ---- GroupNorm / BatchNorm with batch statistics --------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", GN.CASES)
def test_gn_fwd_bwd(ops, guard, case, dt):
    GN.test_gn_fwd_bwd(ops, case, dt)
    guard.clean()


def test_gn_bad_shapes(ops, guard):
    GN.test_gn_bad_shapes(ops)
    guard.clean()


@pytest.mark.parametrize("case", GN.BN_CASES)
def test_bn_train_fwd_bwd(ops, guard, case):
    GN.test_bn_train_fwd_bwd(ops, case)
    guard.clean()


def test_bn_cases_keep_their_first_members():
    assert GN.BN_CASES[:3] == [(2, 64, 13, 21), (3, 256, 8, 12), (1, 1024, 5, 4)]


# the 514 x 512 row stays in: with its poisoned copies it takes about a second
@pytest.mark.parametrize("case", GN.GEOM_CASES + [GN.BIG_CASE], ids=GN._gid)
def test_gn_geometry(ops, guard, case):
    if case is GN.BIG_CASE:
        GN.test_gn_grid_stride(ops)
    else:
        GN.test_gn_geometry(ops, case)
    guard.clean()


@pytest.mark.parametrize("case", GN.BN_GEOM_CASES + [GN.BN_BIG_CASE], ids=GN._gid)
def test_bn_train_geometry(ops, guard, case):
    if case is GN.BN_BIG_CASE:
        GN.test_bn_train_grid_stride(ops)
    else:
        GN.test_bn_train_geometry(ops, case)
    guard.clean()


@pytest.mark.parametrize("case", GN.COND_CASES, ids=GN._cid)
def test_norm_ill_conditioned(ops, guard, case):
    GN.test_gn_ill_conditioned(ops, case)
    GN.test_bn_train_ill_conditioned(ops, case)
    guard.clean()


@pytest.mark.parametrize("kind", ["gn", "bn"])
def test_norm_constant_and_opposite_groups(ops, guard, kind):
    for shape in GN.COND_SHAPES:
        GN.test_constant_group(ops, kind, shape)
        GN.test_opposite_pivots(ops, kind, shape)
    guard.clean()


def test_norm_options(ops, guard):
    for case in GN.BN_CASES:
        GN.test_bn_train_fp16(ops, case)
    for momentum in (0.25, 1.0):
        GN.test_bn_train_momentum(ops, momentum)
    GN.test_bn_train_no_running_stats(ops)
    GN.test_bn_train_up2x(ops)
    for kind in ("gn", "bn"):
        GN.test_eps(ops, kind)
        for dt in DTYPES:
            GN.test_relu6(ops, kind, dt)
        GN.test_accumulate_and_overwrite(ops, kind)
    guard.clean()


# ---- box operations -------------------------------------------------------------------------------------------
def test_anchors(ops, guard):
    BX.test_anchor_grid_pyramid(ops)
    guard.clean()
    BX.test_anchor_pyramid_one_launch(ops)          # an empty level in the middle
    guard.clean()
    BX.test_anchor_grid_edge(ops)
    guard.clean()


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("n,m", [(1000, 1000), (10000, 100), (37, 53), (1, 1), (0, 5), (5, 0)])
def test_iou(ops, guard, n, m, integer):
    BX.test_iou_bit_exact(ops, n, m, integer)
    guard.clean()


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("n", [10000, 1000, 65, 64, 63, 2, 1])
def test_nms(ops, guard, n, integer):
    BX.test_nms_bit_exact(ops, n, integer)
    guard.clean()


@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025, 2048 + 17, 5000])
def test_nms_both_scans(ops, guard, n, monkeypatch):
    """Both scans (TDN_NMS_ONEWAVE = 1 / 0) against each other and the C oracle, also on both sides of the 64-box chunk
    boundary, where the reused test does not go."""
    BX.test_nms_block_scan_equals_single_wave_scan(ops, n, monkeypatch)
    guard.clean()


def test_nms_edge_cases(ops, guard):
    BX.test_nms_edge_cases(ops)
    guard.clean()


def test_bbox_normalize_denormalize(ops, guard):
    BX.test_bbox_normalize_denormalize_vs_reference_golden()
    guard.clean()


def test_bbox_deltas(ops, guard, T):
    PR.test_bbox2delta_vs_oracle(T)
    guard.clean()
    PR.test_delta2bbox_vs_oracle(T)
    guard.clean()


@pytest.mark.parametrize("sizes", [[1500], [0, 1, 700], [300, 0, 1, 2, 2000, 64, 65, 129, 4096, 17], [0, 0]])
def test_batched_nms(ops, guard, T, sizes):
    PR.test_batched_nms_vs_oracle(T, sizes)
    guard.clean()


def test_rpn_proposals_small_levels(ops, guard, T):
    PR.test_rpn_proposals_small_levels_and_nms_pre_zero(T)      # proposals / anchor_idx / counts defined up to max_num
    guard.clean()


@pytest.mark.parametrize("B,dtype,cl,min_size,mode,cfg", [
    (2, torch.float32, False, 0, "normal", dict(nms_pre=2000, nms_post=2000, max_num=2000, nms_thr=0.7)),
    (2, torch.bfloat16, True, 16, "normal", dict(nms_pre=1000, nms_post=1000, max_num=1000, nms_thr=0.7)),
    (1, torch.bfloat16, False, 0, "ties", dict(nms_pre=2000, nms_post=1500, max_num=3000, nms_thr=0.6)),
    (4, torch.float32, True, 16, "saturated", dict(nms_pre=4096, nms_post=300, max_num=1000, nms_thr=0.5,
                                                   target_means=(0.0, 0.1, 0.0, -0.1),
                                                   target_stds=(0.1, 0.1, 0.2, 0.2))),
])
def test_rpn_proposals_c4(ops, guard, T, B, dtype, cl, min_size, mode, cfg):
    PR.test_rpn_proposals_c4_vs_oracle(T, B, dtype, cl, min_size, mode, cfg)
    guard.clean()


# ---- RoIAlign -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,sr", [(7, 2), (7, 0), (14, 2), (14, 0)])
def test_roi_align_forward(ops, guard, T, dtype, S, sr):
    RA.test_forward_bit_identical_to_oracle(T, dtype, S, sr)
    guard.clean()


def test_roi_align_forward_256_channels(ops, guard, T):
    RA.test_forward_bit_identical_256_channels(T)
    guard.clean()


def test_roi_map_levels(ops, guard, T):
    RA.test_map_roi_levels_bit_identical(T)
    guard.clean()


@pytest.mark.parametrize("dtype,S,sr", [(torch.bfloat16, 7, 2), (torch.float16, 14, 0)])
def test_roi_align_backward(ops, guard, T, dtype, S, sr):
    RA.test_backward_matches_float64_oracle(T, dtype, S, sr)
    guard.clean()


def test_roi_align_adjoint_empty_and_nchw(ops, guard, T):
    RA.test_adjoint_on_the_gpu(T)
    guard.clean()
    RA.test_empty_one_level_and_nchw_features(T)
    guard.clean()


def test_rois_from_proposals(ops, guard, T):
    """The eager part of test_proposals_to_extractor_in_one_graph (a graph capture cannot allocate through the
    guard): rows at or past counts[b] carry batch index -1, and the rois feed the extractor."""
    import numpy as np
    levels = [((50, 84), 4), ((25, 42), 8), ((13, 21), 16), ((7, 11), 32)]
    anchors = PR._pyramid(T, levels)
    B, M = 2, 200
    g = torch.Generator().manual_seed(15)
    cls = [torch.randn(B, 3, h, w, generator=g).bfloat16().cuda() for (h, w), _ in levels]
    reg = [(torch.randn(B, 12, h, w, generator=g) * 0.5).bfloat16().cuda() for (h, w), _ in levels]
    ish = torch.tensor([(200, 336), (180, 300)], dtype=torch.int32).cuda()
    fs = RA.feats_of(B, 64, [fs for fs, _ in levels], torch.bfloat16, 16)
    props, _, counts = T.rpn_proposals(cls, reg, anchors, ish, nms_pre=300, nms_post=300, max_num=M)
    rois = T.rois_from_proposals(props, counts)
    out = T.SingleRoIExtractor(out_channels=64)(fs, rois)
    guard.clean()
    p, c, r = props.cpu().numpy(), counts.cpu().numpy(), rois.cpu().numpy()
    assert r.shape == (B * M, 5)
    for b in range(B):
        rows = r[b * M:(b + 1) * M]
        assert np.array_equal(rows[:, 1:], p[b, :, :4])
        assert np.all(rows[:c[b], 0] == b) and np.all(rows[c[b]:, 0] == -1)
    ref = RA.to16(RA.R.roi_align_forward(RA.np_feats(fs), r, RA.STRIDES, 7, 2), torch.bfloat16)
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))


# ---- caller buffers: out=, outs=, bits=, dw=, dgamma=, dbeta= --------------------------------------------------
def _alloc_like(guard, t, label):
    return guard.alloc(tuple(t.shape), t.dtype, t.device, label=label)


def test_caller_buffers_conv_and_stem(ops, guard):
    dev = torch.device("cuda")
    N, H, W, Cin, Cout = 1, 13, 21, 128, 128
    x = K.nhwc(det_tensor((N, Cin, H, W), 1, -1, 1))
    w = det_tensor((Cout, Cin, 3, 3), 2, -0.2, 0.2)
    wf, wd = K.pack_w(w), K.pack_wd(w)
    for f32 in (False, True):
        y = ops.conv2d_fwd(x, wf, 3, 1, 1, relu=True, out_f32=f32)
        y2 = ops.conv2d_fwd(x, wf, 3, 1, 1, relu=True, out_f32=f32, out=_alloc_like(guard, y, "conv2d_fwd: out="))
        dx = ops.conv2d_dgrad(y if not f32 else y.bfloat16(), wd, (H, W), 3, 1, 1, out_f32=f32)
        dx2 = ops.conv2d_dgrad(y if not f32 else y.bfloat16(), wd, (H, W), 3, 1, 1, out_f32=f32,
                               out=_alloc_like(guard, dx, "conv2d_dgrad: out="))
        guard.clean()
        _same(y2, y, "conv2d_fwd out=")
        _same(dx2, dx, "conv2d_dgrad out=")
    # bn_fold out=, pack_conv_weight / pack_stem_weight / pack_gconv_weight out=
    g4 = [det_tensor((Cout,), 10 + j, lo, hi, bf16=False).cuda() for j, (lo, hi) in
          enumerate(((0.5, 1.5), (-1, 1), (-1, 1), (0.5, 1.5)))]
    ref = ops.bn_fold(*g4, 1e-5)
    got = ops.bn_fold(*g4, 1e-5, out=guard.alloc((3, Cout), torch.float32, dev, label="bn_fold: out="))
    wfp = ops.pack_conv_weight(w.cuda(), ref[0])
    wfp2 = ops.pack_conv_weight(w.cuda(), ref[0], out=tuple(_alloc_like(guard, t, "pack_conv_weight: out=") for t in wfp))
    ws = det_tensor((64, 3, 7, 7), 20, -0.2, 0.2).cuda()
    sp = ops.pack_stem_weight(ws)
    sp2 = ops.pack_stem_weight(ws, out=_alloc_like(guard, sp, "pack_stem_weight: out="))
    wg = det_tensor((128, 4, 3, 3), 21, -0.3, 0.3).cuda()
    gp = ops.pack_gconv_weight(wg, 32, ref[0])
    gp2 = ops.pack_gconv_weight(wg, 32, ref[0], out=tuple(_alloc_like(guard, t, "pack_gconv_weight: out=") for t in gp))
    guard.clean()
    for a, b in zip(got + wfp2 + (sp2,) + gp2, ref + wfp + (sp,) + gp):
        _same(a, b, "pack / fold out=")
    # stem_pool_fwd out=
    img = det_tensor((2, 3, 30, 44), 30, -2, 2)
    xp = ops.stage_image(img.cuda())
    sc, sh = (det_tensor((64,), 31 + j, 0.5, 1.5, bf16=False).cuda() for j in range(2))
    y, idx = ops.stem_pool_fwd(xp, sp, (30, 44), sc, sh)
    y2, idx2 = ops.stem_pool_fwd(xp, sp, (30, 44), sc, sh, out=(_alloc_like(guard, y, "stem_pool_fwd: out[0]"),
                                                                 _alloc_like(guard, idx, "stem_pool_fwd: out[1]")))
    guard.clean()
    _same(y2, y, "stem_pool_fwd out=")
    assert torch.equal(idx2, idx) and int(idx2.max()) <= 8


@pytest.mark.parametrize("C", [64, 128])
def test_caller_buffers_block(ops, guard, monkeypatch, C):
    """outs= and bits= of the one-launch blocks as must-write, guard-banded buffers on a ragged shape."""
    dev = torch.device("cuda")
    N, H, W, dtype = 2, 13, 21, torch.bfloat16
    x, w1, w2, w3, aff = BL._case(N, H, W, C, dtype, 4711)
    xg, w1g, w2g, w3g = (t.contiguous().to(dev) for t in (x, w1, w2, w3))
    affg = [a.to(dev) for a in aff]
    for th in ((None, "10") if C == 128 else (None,)):
        if th:
            monkeypatch.setenv("TDN_BLOCK128_TH", th)
        ref = ops.bottleneck_fwd(xg, w1g, w2g, w3g, affg)
        outs = tuple(_alloc_like(guard, t, "bottleneck_fwd: outs[%d]" % i) for i, t in enumerate(ref))
        bits = tuple(guard.alloc((N, H, W, ch // 32), torch.int32, dev, label="bottleneck_fwd: bits[%d]" % i)
                     for i, ch in enumerate((C, C, 4 * C)))
        got = ops.bottleneck_fwd(xg, w1g, w2g, w3g, affg, outs=outs, bits=bits)
        guard.clean()
        for a, b in zip(got, ref):
            _same(a, b, "bottleneck_fwd outs=")
        for b, src, ch in zip(bits, (ref[0], ref[1], xg), (C, C, 4 * C)):
            assert torch.equal(BL._unpack_bits(b, ch), src.float().cpu() > 0)
        w1d, w2d, w3d = (w.permute(3, 1, 2, 0).contiguous() for w in (w1g, w2g, w3g))
        g = torch.where(ref[2] > 0, (det_tensor((N, H, W, 4 * C), 991) * 0.1).to(dtype).to(dev),
                        torch.zeros((), device=dev, dtype=dtype)).contiguous()
        dref = ops.bottleneck_dgrad(g, w3d, w2d, w1d, (ref[1], ref[0], xg))
        douts = tuple(_alloc_like(guard, t, "bottleneck_dgrad: outs[%d]" % i) for i, t in enumerate(dref))
        dgot = ops.bottleneck_dgrad(g, w3d, w2d, w1d, None, outs=douts, bits=bits)
        guard.clean()
        for a, b in zip(dgot, dref):
            _same(a, b, "bottleneck_dgrad outs=")


def test_caller_buffers_wgrad_and_gn(ops, guard, monkeypatch):
    """dw= / dgamma= / dbeta=: with beta = 0 the poison must vanish (a kernel that forms beta * old + new would keep
    the NaN); with beta = 1 the result is the seeded value plus the gradient — one fp32 addition of the same gradient,
    so at most one rounding (2^-24 relative, possibly fused differently) apart from torch's own sum: rel-L2 <= 1e-6."""
    dev = torch.device("cuda")
    for case, t9 in (((1, 13, 21, 128, 128, 3, 1), "1"), ((2, 25, 42, 128, 128, 3, 2), None),
                     ((2, 40, 48, 64, 64, 3, 1), None)):
        if t9:
            monkeypatch.setenv("TDN_WGRAD9", t9)
        N, H, W, Cin, Cout, k, s = case
        Ho, Wo = ops.conv_out_size(H, k, s, k // 2), ops.conv_out_size(W, k, s, k // 2)
        x = K.nhwc(det_tensor((N, Cin, H, W), 31, -1, 1))
        g = K.nhwc(det_tensor((N, Cout, Ho, Wo), 32, -1, 1))
        wf = K.pack_w(det_tensor((Cout, Cin, k, k), 33, -0.2, 0.2))
        bn = tuple(det_tensor((Cout,), 34 + j, lo, hi, bf16=False).cuda()
                   for j, (lo, hi) in enumerate(((0.5, 1.5), (-0.2, 0.2), (0.7, 1.4))))
        ref = ops.conv2d_wgrad(x, g, wf, k, s, k // 2, *bn)
        bufs = [_alloc_like(guard, t, "conv2d_wgrad: %s=" % nm) for t, nm in zip(ref, ("dw", "dgamma", "dbeta"))]
        got = ops.conv2d_wgrad(x, g, wf, k, s, k // 2, *bn, dw=bufs[0], dgamma=bufs[1], dbeta=bufs[2], beta=0.0)
        guard.clean()
        for a, b in zip(got, ref):
            _same(a, b, "conv2d_wgrad beta=0 %s" % (case,))
        seeds = [det_tensor(tuple(t.shape), 40 + j, -1, 1, bf16=False).cuda() for j, t in enumerate(ref)]
        bufs = [guard.guard_copy(sd, "conv2d_wgrad: seeded") for sd in seeds]
        got = ops.conv2d_wgrad(x, g, wf, k, s, k // 2, *bn, dw=bufs[0], dgamma=bufs[1], dbeta=bufs[2], beta=1.0)
        guard.clean()
        for a, sd, b in zip(got, seeds, ref):
            assert rel_l2(a.cpu(), (sd + b).cpu()) <= 1e-6, case
        monkeypatch.delenv("TDN_WGRAD9", raising=False)
    # GroupNorm / BN-train backward: dgamma= / dbeta=, accumulate False (overwrite) and True
    N, C, H, W = 2, 64, 13, 21
    z = K.nhwc(det_tensor((N, C, H, W), 51, -2, 2))
    gg = K.nhwc(det_tensor((N, C, H, W), 52, -1, 1))
    gamma = det_tensor((C,), 53, 0.5, 1.5, bf16=False).cuda()
    beta = det_tensor((C,), 54, -0.5, 0.5, bf16=False).cuda()
    for name in ("gn", "bn"):
        if name == "gn":
            _, stats = ops.gn_fwd(z, gamma, beta, 32)
            bwd = lambda *a: ops.gn_bwd(gg, z, stats, gamma, 32, *a)      # noqa: E731
        else:
            _, stats = ops.bn_train_fwd(z, gamma, beta)
            bwd = lambda *a: ops.bn_train_bwd(gg, z, stats, gamma, *a)    # noqa: E731
        dz, dg, db = bwd()
        b1 = [guard.alloc((C,), torch.float32, dev, label="%s_bwd: %s=" % (name, nm)) for nm in ("dgamma", "dbeta")]
        dz1, dg1, db1 = bwd(b1[0], b1[1], False)
        guard.clean()
        _same(dg1, dg, name + " dgamma=")
        _same(db1, db, name + " dbeta=")
        _same(dz1, dz, name + " dz")
        seeds = [det_tensor((C,), 55 + j, -1, 1, bf16=False).cuda() for j in range(2)]
        b2 = [guard.guard_copy(sd, name + "_bwd: seeded") for sd in seeds]
        _, dg2, db2 = bwd(b2[0], b2[1], True)
        guard.clean()
        assert rel_l2(dg2.cpu(), (seeds[0] + dg).cpu()) <= 1e-6 and rel_l2(db2.cpu(), (seeds[1] + db).cpu()) <= 1e-6


def test_standalone_wgrad_workspace_sizes(ops, guard):
    """tdn_conv2d_wgrad_workspace / tdn_gconv2d_wgrad_workspace / tdn_stem_conv_wgrad_workspace promise the bytes of
    the single-layer calls; ops.py reaches those kernels through one-member groups.  The guarded one-member launches
    here run in exactly the bytes the single-layer functions name, and come back clean."""
    lib = ops._lib.load()

    def used(fn, *a, **kw):
        fn(*a, **kw)
        asked = guard.ws_log[-1][1]
        guard.clean()
        return asked

    N, H, W, Cin, Cout, k, s = 2, 40, 48, 64, 64, 3, 1
    x = K.nhwc(det_tensor((N, Cin, H, W), 61, -1, 1))
    g = K.nhwc(det_tensor((N, Cout, H, W), 62, -1, 1))
    wf = K.pack_w(det_tensor((Cout, Cin, k, k), 63, -0.2, 0.2))
    assert used(ops.conv2d_wgrad, x, g, wf, k, s, 1) == lib.tdn_conv2d_wgrad_workspace(N, H, W, Cin, Cout, k, s, 1) > 0
    C, G = 128, 32
    xg = K.nhwc(det_tensor((2, C, 12, 16), 64, -1, 1))
    gg = K.nhwc(det_tensor((2, C, 12, 16), 65, -1, 1))
    wg, _ = ops.pack_gconv_weight(det_tensor((C, C // G, 3, 3), 66, -0.3, 0.3).cuda(), G)
    assert used(ops.gconv2d_wgrad, xg, gg, wg, G, 3, 1, 1) == lib.tdn_gconv2d_wgrad_workspace(2, 12, 16, C, G, 3, 1, 1) > 0
    xp = ops.stage_image(det_tensor((2, 3, 64, 96), 67, -2, 2).cuda())
    wst = ops.pack_stem_weight(det_tensor((64, 3, 7, 7), 68, -0.2, 0.2).cuda())
    gs = K.nhwc(det_tensor((2, 64, 32, 48), 69, -1, 1))
    assert used(ops.stem_conv_wgrad, xp, gs, wst, (64, 96)) == lib.tdn_stem_conv_wgrad_workspace(2, 64, 96, 64) > 0


# ---- input-side bands for the tiled readers -------------------------------------------------------------------
def _input_banded(guard, fn, tensors):
    """fn(*tensors) with plain operands and again with every operand copied into a NaN-banded buffer: the outputs must
    be bit-identical (a read past an operand that reaches an output turns it into NaN).  Reads whose result is
    discarded are legal and invisible."""
    plain = fn(*tensors)
    banded = fn(*[guard.guard_copy(t, "input %d" % i) if t is not None else None for i, t in enumerate(tensors)])
    guard.clean()
    plain = plain if isinstance(plain, (tuple, list)) else (plain,)
    banded = banded if isinstance(banded, (tuple, list)) else (banded,)
    for i, (a, b) in enumerate(zip(plain, banded)):
        if a is not None:
            _same(b, a, "output %d with NaN-banded inputs" % i)


@pytest.mark.parametrize("tile", [None, 0, 3, 46])
def test_input_bands_conv(ops, guard, monkeypatch, tile):
    """Generic implicit GEMM: x, weights, scale / shift, addend, mask source — odd sizes, 3x3 and strided 1x1."""
    if tile is not None:
        monkeypatch.setenv("TDN_GEMM_CFG", str(tile))
    monkeypatch.setenv("TDN_HALO", "0")
    for (N, H, W, Cin, Cout, k, s) in [(1, 13, 21, 256, 256, 3, 1), (2, 25, 42, 256, 256, 3, 2), (1, 25, 43, 256, 256, 1, 2)]:
        Ho, Wo = ops.conv_out_size(H, k, s, k // 2), ops.conv_out_size(W, k, s, k // 2)
        x = K.nhwc(det_tensor((N, Cin, H, W), 1, -1, 1))
        w = det_tensor((Cout, Cin, k, k), 2, -0.2, 0.2)
        sc, sh = (det_tensor((Cout,), 3 + j, 0.5, 1.5, bf16=False).cuda() for j in range(2))
        res = K.nhwc(det_tensor((N, Cout, Ho, Wo), 5, -1, 1))
        _input_banded(guard, lambda x_, w_, sc_, sh_, r_: ops.conv2d_fwd(x_, w_, k, s, k // 2, sc_, sh_, r_, ops.ADD_SAME, True),
                      [x, K.pack_w(w), sc, sh, res])
        g = K.nhwc(det_tensor((N, Cout, Ho, Wo), 6, -1, 1))
        add, msk = (K.nhwc(det_tensor((N, Cin, H, W), 7 + j, -1, 1)) for j in range(2))
        _input_banded(guard, lambda g_, w_, a_, m_: ops.conv2d_dgrad(g_, w_, (H, W), k, s, k // 2, a_, ops.ADD_SAME, m_),
                      [g, K.pack_wd(w), add, msk])
    # FPN epilogues: nearest-2x addend (forward), 2x2 sum-pool addend (dgrad)
    N, H, W, C = 2, 10, 14, 256
    x = K.nhwc(det_tensor((N, C, H, W), 11, -1, 1))
    w = det_tensor((C, C, 3, 3), 12, -0.2, 0.2)
    coarse = K.nhwc(det_tensor((N, C, H // 2, W // 2), 13, -1, 1))
    fine = K.nhwc(det_tensor((N, C, 2 * H, 2 * W), 14, -1, 1))
    _input_banded(guard, lambda x_, w_, c_: ops.conv2d_fwd(x_, w_, 3, 1, 1, None, None, c_, ops.ADD_UP2X), [x, K.pack_w(w), coarse])
    _input_banded(guard, lambda g_, w_, f_: ops.conv2d_dgrad(g_, w_, (H, W), 3, 1, 1, f_, ops.ADD_SUMPOOL2), [x, K.pack_wd(w), fine])


def test_input_bands_halo(ops, guard, monkeypatch):
    ran = 0
    for cfg, (N, H, W, Cin, Cout) in [(c, s) for c in (0, 3, 5, 9, 11) for s in
                                      [(2, 13, 21, 128, 128), (1, 25, 42, 256, 256), (1, 33, 18, 320, 128)]]:
        monkeypatch.setenv("TDN_HALO_CFG3", str(cfg))
        if Cout % HL.CFG3[cfg] or Cin % HL.CFG3[cfg] or not HL.uses_halo(ops, 0, N, H, W, Cin, Cout, 3, 1, 1) \
                or not HL.uses_halo(ops, 1, N, H, W, Cin, Cout, 3, 1, 1):
            continue
        ran += 1
        x = K.nhwc(det_tensor((N, Cin, H, W), 1, -1, 1))
        w = det_tensor((Cout, Cin, 3, 3), 2, -0.2, 0.2)
        sc, sh = (det_tensor((Cout,), 3 + j, 0.5, 1.5, bf16=False).cuda() for j in range(2))
        res = K.nhwc(det_tensor((N, Cout, H, W), 5, -1, 1))
        _input_banded(guard, lambda x_, w_, sc_, sh_, r_: ops.conv2d_fwd(x_, w_, 3, 1, 1, sc_, sh_, r_, ops.ADD_SAME, True),
                      [x, K.pack_w(w), sc, sh, res])
        g = K.nhwc(det_tensor((N, Cout, H, W), 6, -1, 1))
        add, msk = (K.nhwc(det_tensor((N, Cin, H, W), 7 + j, -1, 1)) for j in range(2))
        _input_banded(guard, lambda g_, w_, a_, m_: ops.conv2d_dgrad(g_, w_, (H, W), 3, 1, 1, a_, ops.ADD_SAME, m_),
                      [g, K.pack_wd(w), add, msk])
    assert ran >= 3, "the forced halo configurations took %d of 15 shape / configuration pairs" % ran


@pytest.mark.parametrize("C,th", [(64, None), (128, None), (128, "10")])
def test_input_bands_block(ops, guard, monkeypatch, C, th):
    dev = torch.device("cuda")
    if th:
        monkeypatch.setenv("TDN_BLOCK128_TH", th)
    for (N, H, W) in [(2, 13, 21), (1, 17, 40), (3, 5, 7)]:
        x, w1, w2, w3, aff = BL._case(N, H, W, C, torch.bfloat16, 100 * H + W)
        xg, w1g, w2g, w3g = (t.contiguous().to(dev) for t in (x, w1, w2, w3))
        affg = [a.to(dev) for a in aff]
        h1, h2, out = ops.bottleneck_fwd(xg, w1g, w2g, w3g, affg)
        _input_banded(guard, lambda x_, a_, b_, c_, *af: ops.bottleneck_fwd(x_, a_, b_, c_, list(af)),
                      [xg, w1g, w2g, w3g] + affg)
        w1d, w2d, w3d = (w.permute(3, 1, 2, 0).contiguous() for w in (w1g, w2g, w3g))
        g = torch.where(out > 0, (det_tensor((N, H, W, 4 * C), 313) * 0.1).bfloat16().to(dev),
                        torch.zeros((), device=dev, dtype=torch.bfloat16)).contiguous()
        _input_banded(guard, lambda g_, a_, b_, c_, m2, m1, m3: ops.bottleneck_dgrad(g_, a_, b_, c_, (m2, m1, m3)),
                      [g, w3d, w2d, w1d, h2, h1, xg])
        bits = ops.bottleneck_bit_planes(N, H, W, C, dev)
        ops.bottleneck_fwd(xg, w1g, w2g, w3g, affg, bits=bits)
        _input_banded(guard, lambda g_, a_, b_, c_, p1, p2, p3: ops.bottleneck_dgrad(g_, a_, b_, c_, None, bits=(p1, p2, p3)),
                      [g, w3d, w2d, w1d] + list(bits))
    if C == 64:      # the head block: x has C channels, the downsample branch inside the launch
        N, H, W = 1, 13, 21
        x, w1, w2, w3, wd, aff = BL._head_case(N, H, W, torch.bfloat16, 7)
        xg, w1g, w2g, w3g, wdg = (t.contiguous().to(dev) for t in (x, w1, w2, w3, wd))
        affg = [a.to(dev) for a in aff]
        _input_banded(guard, lambda x_, a_, b_, c_, d_, *af: ops.bottleneck_head_fwd(x_, a_, b_, c_, list(af[:6]), None,
                                                                                   down=(d_, af[6], af[7])),
                      [xg, w1g, w2g, w3g, wdg] + affg)


def test_input_bands_gconv(ops, guard):
    for (N, H, W, C, G_, s) in [(2, 12, 16, 128, 32, 1), (1, 13, 21, 256, 32, 2), (1, 10, 12, 128, 2, 1)]:
        x = K.nhwc(det_tensor((N, C, H, W), 91, -1, 1))
        w = det_tensor((C, C // G_, 3, 3), 92, -0.3, 0.3).cuda()
        sc, sh = (det_tensor((C,), 93 + j, 0.5, 1.5, bf16=False).cuda() for j in range(2))
        wf, wd = ops.pack_gconv_weight(w, G_, sc)
        guard.clean()
        _input_banded(guard, lambda x_, w_, sc_, sh_: ops.gconv2d_fwd(x_, w_, G_, 3, s, 1, sc_, sh_, relu=True), [x, wf, sc, sh])
        Ho, Wo = ops.conv_out_size(H, 3, s, 1), ops.conv_out_size(W, 3, s, 1)
        g = K.nhwc(det_tensor((N, C, Ho, Wo), 95, -1, 1))
        _input_banded(guard, lambda g_, w_: ops.gconv2d_dgrad(g_, w_, G_, (H, W), 3, s, 1), [g, wd])
        _input_banded(guard, lambda x_, g_, w_: ops.gconv2d_wgrad(x_, g_, w_, G_, 3, s, 1), [x, g, wf])


def test_input_bands_roi_align(ops, guard):
    B, C, S = 2, 32, 7
    shapes = [(50, 84), (25, 42), (13, 21), (7, 11)]
    fs = [f.permute(0, 2, 3, 1).contiguous() for f in RA.feats_of(B, C, shapes, torch.bfloat16, 6)]     # NHWC memory
    rois = torch.from_numpy(RA.mixed_rois(300, B, 7, canvas=(200, 336))).cuda()
    scales = [1.0 / s for s in RA.STRIDES]
    _input_banded(guard, lambda r_, *f_: ops.roi_align_fwd([f.permute(0, 3, 1, 2) for f in f_], r_, S, scales, 2, 56.0),
                  [rois] + fs)
    dout = torch.randn(300, C, S, S, generator=torch.Generator().manual_seed(8)).bfloat16().cuda() \
        .contiguous(memory_format=torch.channels_last)
    _input_banded(guard, lambda r_, d_: ops.roi_align_bwd(d_.permute(0, 3, 1, 2), r_, shapes, B, C, torch.bfloat16, S,
                                                        scales, 2, 56.0),
                  [rois, dout.permute(0, 2, 3, 1).contiguous()])


def test_input_bands_gn(ops, guard):
    for (N, C, H, W) in [(2, 64, 13, 21), (1, 128, 25, 42), (1, 2048, 4, 5)]:
        z = K.nhwc(det_tensor((N, C, H, W), 1, -2, 2))
        res = K.nhwc(det_tensor((N, C, H, W), 4, -1, 1))
        gamma = det_tensor((C,), 2, 0.5, 1.5, bf16=False).cuda()
        beta = det_tensor((C,), 3, -0.5, 0.5, bf16=False).cuda()
        _input_banded(guard, lambda z_, g_, b_, r_: ops.gn_fwd(z_, g_, b_, 32, 1e-5, r_, True), [z, gamma, beta, res])
        _, stats = ops.gn_fwd(z, gamma, beta, 32)
        g = K.nhwc(det_tensor((N, C, H, W), 5, -1, 1))
        _input_banded(guard, lambda g_, z_, s_, ga_: ops.gn_bwd(g_, z_, s_, ga_, 32), [g, z, stats, gamma])
        if C > 1024:        # the BN-train cases of test_gpu_gn.py stop at 1024 channels
            continue
        _input_banded(guard, lambda z_, g_, b_, r_: ops.bn_train_fwd(z_, g_, b_, None, None, 0.1, 1e-5, r_, True),
                      [z, gamma, beta, res])
        _, bstats = ops.bn_train_fwd(z, gamma, beta)
        _input_banded(guard, lambda g_, z_, s_, ga_: ops.bn_train_bwd(g_, z_, s_, ga_), [g, z, bstats, gamma])


# ---- coverage of this run (keep these two last) ---------------------------------------------------------------
# public functions of ops.py that neither allocate device memory nor take a workspace nor launch anything
HOST_ONLY = {
    "dtype_code": "dtype -> enum code",
    "conv_out_size": "integer arithmetic",
    "make_epilogue": "fills a host struct from validated pointers",
    "bottleneck_supported": "host query of the build",
    "bottleneck_head_supported": "host query of the build",
    "wgrad_item": "fills a host struct",
    "wgrad_group_plan": "host-only plan",
    "roi_level_shapes": "host validation of shapes",
}


# launch kernels, but allocate nothing themselves: counted by their successful returns only
NO_ALLOCATION_OF_THEIR_OWN = {
    "conv2d_wgrad": "conv2d_wgrad_item allocates, wgrad_group takes the workspace",
    "stem_conv_wgrad": "stem_conv_wgrad_item allocates, wgrad_group takes the workspace",
    "gconv2d_wgrad": "gconv2d_wgrad_item allocates, wgrad_group takes the workspace",
    "clamp_max_": "in place",
    "bbox_normalize_": "in place",
    "prepare_group": "writes caller buffers only",
}


def test_every_entry_point_ran_under_the_guard(ops):
    """Every public function of ops.py that allocates or takes a workspace got at least one allocation / workspace
    from the proxy that was then checked (counted in the proxy, by the calling function's name), and returned at least
    once under the guard; the few that launch without allocating returned at least once."""
    public = _public(ops)
    assert set(HOST_ONLY) <= set(public), sorted(set(HOST_ONLY) - set(public))
    assert set(NO_ALLOCATION_OF_THEIR_OWN) <= set(public) and not set(NO_ALLOCATION_OF_THEIR_OWN) & set(HOST_ONLY)
    missing = [n for n in public if n not in HOST_ONLY and ENTERED[n] == 0]
    assert not missing, "never returned under the guard in this run: %s" % missing
    unseen = [n for n in public if n not in HOST_ONLY and n not in NO_ALLOCATION_OF_THEIR_OWN and PROXY_SEEN[n] == 0]
    assert not unseen, "no guarded allocation or workspace was made for: %s" % unseen


def test_every_workspace_function_ran_at_its_exact_size(ops):
    """Every tdn_*_workspace of include/tdn.h: some guarded call ran in a workspace of exactly that many bytes (rounded
    up only to the 16 / 256-byte alignment the header asks for) and came back with clean bands; the results of those
    calls were compared with their references, NaN-free, by the tests above."""
    hdr = open(os.path.join(ROOT, "include", "tdn.h")).read()
    fns = sorted(set(re.findall(r"\b(tdn_\w+_workspace)\s*\(", hdr)))
    via = {
        "tdn_wgrad_group_workspace": ["wgrad_group"],
        # the single-layer sizes are what one-member groups use: test_standalone_wgrad_workspace_sizes
        "tdn_conv2d_wgrad_workspace": ["wgrad_group"],
        "tdn_gconv2d_wgrad_workspace": ["wgrad_group"],
        "tdn_stem_conv_wgrad_workspace": ["wgrad_group"],
        "tdn_channel_affine_bwd_workspace": ["channel_affine_bwd"],
        "tdn_nms_workspace": ["nms"],
        "tdn_batched_nms_workspace": ["batched_nms"],
        "tdn_rpn_proposals_workspace": ["rpn_proposals"],
        "tdn_roi_align_bwd_workspace": ["roi_align_bwd"],
        "tdn_gn_workspace": ["gn_fwd", "gn_bwd", "bn_train_fwd", "bn_train_bwd"],
    }
    assert fns == sorted(via), "include/tdn.h has workspace functions this test does not know: %s" % (set(fns) ^ set(via))
    for fn, users in via.items():
        for op in users:
            assert op in WS_SEEN, "%s: no clean exact-size workspace through ops.%s in this run" % (fn, op)
            asked, given = WS_SEEN[op]
            assert 0 <= given - asked < 256, (fn, op, asked, given)
    assert ENTERED["stem_conv_wgrad"] and ENTERED["gconv2d_wgrad"] and ENTERED["conv2d_wgrad"]
