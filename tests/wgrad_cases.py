"""The case table of the weight-gradient plan tests (test_wgrad_oracle.py on the CPU, test_gpu_wgrad_plans.py and its
guarded reuse on the GPU): tiny members whose PLAN — kernel, tile shape, split count, last split's length, direct or
slab — is forced through the planner's test switches and asserted on the rows of ``ops.wgrad_group_plan`` before
anything is launched.  A case that stopped exercising its layout fails; it cannot pass by accident.

Plan row (include/tdn.h, tdn_wgrad_group_plan): [variant, tile co, tile ci, splits, pixels per split, direct,
workgroups, slab KiB]; variant 0: tap-per-tile kernel, 1 / 2: nine-tap kernel with the 128- / 64-channel tile.

``TDN_WGRAD_T`` (K-steps of 64 pixels per split) only reaches small values together with ``TDN_WGRAD_TMIN=1`` and
``TDN_WGRAD9_TMIN=1``; ``expected_split`` restates csrc/conv_wgrad.hip's split_member, and every expectation below was
derived with it, not read off a run.
"""
import collections

import torch

import wgrad_ref as R

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}

Case = collections.namedtuple("Case", "id members knobs dtype bn accumulate expect purpose seed")
# members: tuple of wgrad_ref.Member; bn: one flag per member; expect: one dict per member with any of
#   variant, tile (co, ci), splitk, last (pixels of the last split), direct, idle (workgroup slots without a split),
#   tiles (workgroups per split)


def expected_split(M, T):
    """(splits, pixels per split) of split_member(M, T)."""
    ksteps = -(-M // 64)
    T = max(T, 1)
    splitk = min(max((ksteps + T // 2) // T, 1), 256)
    if splitk >= 8:
        splitk = (splitk + 4) // 8 * 8
    mchunk = -(-(-(-M // splitk)) // 64) * 64
    return -(-M // mchunk), mchunk


def slots(splitk):
    return 8 * ((splitk + 7) // 8) if splitk >= 8 else splitk


def t_knobs(T, **more):
    k = {"TDN_WGRAD_T": T, "TDN_WGRAD_TMIN": 1, "TDN_WGRAD9_TMIN": 1}
    k.update(more)
    return k


# ---- pixel layouts: name -> (output grid (N, Ho, Wo), T, extra knobs, expected splits, last split's pixels, direct) ---
LAYOUTS = collections.OrderedDict([
    ("lt64",     ((1, 5, 9),     1,    {}, 1, 45, True)),       # fewer than 64 pixels
    ("direct3",  ((3, 5, 9),     1000, {}, 1, 135, True)),      # direct, ragged, three images
    ("slab1",    ((3, 5, 9),     1000, {"TDN_WGRAD_DIRECT": 0}, 1, 135, False)),
    ("plain3",   ((3, 5, 9),     1,    {}, 3, 7, None)),        # plain order, image wrap inside a split
    ("twostep",  ((2, 13, 21),   2,    {}, 5, 34, None)),       # two K-steps per split
    ("x8",       ((1, 16, 32),   1,    {}, 8, 64, None)),       # exactly 8: XCD map, no idle slot
    ("c9to5",    ((1, 9, 63),    1,    {}, 5, 55, None)),       # 9 requested collapse to 5 two-step splits
    ("s13of16",  ((1, 13, 63),   1,    {}, 13, 51, None)),      # 13 real splits in 16 slots
    ("s20of24",  ((1, 20, 63),   1,    {}, 20, 44, None)),      # 20 real splits in 24 slots, three rounds
    ("cap63",    ((1, 127, 129), 1,    {}, 256, 63, None)),     # the 256-split cap
    ("cap64",    ((1, 128, 128), 1,    {}, 256, 64, None)),
])
for _n, (_grid, _T, _k, _s, _last, _d) in LAYOUTS.items():       # the table above against the planner's arithmetic
    _M = _grid[0] * _grid[1] * _grid[2]
    _sk, _mc = expected_split(_M, _T)
    assert (_sk, _M - (_sk - 1) * _mc) == (_s, _last), (_n, _sk, _mc)

# tap-per-tile shape ids (TDN_TAP_SHAPES of conv_wgrad.hip): id -> (tile co, tile ci) and the smallest member (Cin, Cout)
TAP_SHAPES = {0: (64, 32), 1: (64, 64), 2: (64, 64), 3: (128, 64), 4: (128, 64), 5: (256, 64), 6: (256, 64),
              7: (128, 128), 8: (256, 128)}
SMALLEST = {1: (64, 64), 2: (64, 64), 3: (64, 128), 4: (64, 128), 5: (64, 256), 6: (64, 256), 7: (128, 128),
            8: (128, 256)}

CASES = []


def _in_size(out, k, stride):
    return out if stride == 1 else 2 * out - 1      # odd input size whose stride-2 "same" output is ``out``


def _add(cid, members, knobs, expect, purpose, dtype="bf16", bn=None, accumulate=False):
    i = len(CASES)
    if bn is None:
        bn = tuple((i + j) % 2 == 0 for j in range(len(members)))     # BN operands on about half the cases
    CASES.append(Case(cid, tuple(members), dict(knobs), dtype, tuple(bn), accumulate, tuple(expect), purpose,
                      1000 + 16 * i))


def _layout_case(cid, layout, make_member, knobs, expect, purpose, **kw):
    grid, T, extra, splitk, last, direct = LAYOUTS[layout]
    m = make_member(grid)
    assert (m.N,) + R.out_hw(m) == tuple(grid), (cid, m, grid)
    k = t_knobs(T, **extra)
    k.update(knobs)
    e = dict(expect, splitk=splitk, last=last)
    never_direct = m.kind != "conv"
    if direct is not None:
        e["direct"] = bool(direct) and not never_direct
    elif splitk > 1:
        e["direct"] = False
    if splitk >= 8:
        e["idle"] = slots(splitk) - splitk
    _add(cid, [m], k, [e], purpose + " [" + layout + "]", **kw)


def _conv_on(Cin, Cout, k, stride=1, pad=None):
    return lambda grid: R.conv(grid[0], _in_size(grid[1], k, stride), _in_size(grid[2], k, stride), Cin, Cout, k,
                               stride, pad)


# ---- tap-per-tile kernel: every selectable tile shape, 1x1 and 3x3 ------------------------------------------------------
for sid in range(1, 9):
    cin, cout = SMALLEST[sid]
    for k in (1, 3):
        for li, lay in enumerate(("plain3", "s13of16", "direct3")):
            # BN operands alternate so that every layout has them with 1x1 and with 3x3 (direct: 1 and 9 dot partials)
            _layout_case("tap-s%d-k%d-%s" % (sid, k, lay), lay, _conv_on(cin, cout, k),
                         {"TDN_WGRAD9": 0, "TDN_WGRAD_SHAPE": sid}, {"variant": 0, "tile": TAP_SHAPES[sid]},
                         "tile shape %d (%dx%d) forced on %d->%d %dx%d" % ((sid,) + TAP_SHAPES[sid] + (cin, cout, k, k)),
                         bn=((sid + k // 2 + li) % 2 == 0,))
# more than one tile per split under the XCD map: two co tiles x nine taps
_layout_case("tap-s2-k3-64to128-s13of16", "s13of16", _conv_on(64, 128, 3), {"TDN_WGRAD9": 0, "TDN_WGRAD_SHAPE": 2},
             {"variant": 0, "tile": (64, 64), "tiles": 18}, "18 tiles per split, 13 splits in 16 slots")
_layout_case("tap-s7-k3-128to256-s20of24", "s20of24", _conv_on(128, 256, 3), {"TDN_WGRAD9": 0, "TDN_WGRAD_SHAPE": 7},
             {"variant": 0, "tile": (128, 128), "tiles": 18}, "18 tiles per split, 20 splits in 24 slots")

# ---- default tile: strides, dilation, finalize passes ----------------------------------------------------------------------
_add("tap-k3s2-13x21", [R.conv(1, 13, 21, 64, 64, 3, 2)], t_knobs(1),
     [{"variant": 0, "tile": (64, 64), "splitk": 2, "last": 13, "direct": False}],
     "3x3 stride 2 at odd input 13x21 (output 7x11)")
_add("tap-k3s2-13x21-n3", [R.conv(3, 13, 21, 64, 128, 3, 2)], t_knobs(1),
     [{"variant": 0, "splitk": 4, "last": 39, "direct": False}], "3x3 stride 2, odd input, image wrap inside splits")
_add("tap-k1s2-25x43", [R.conv(1, 25, 43, 64, 128, 1, 2)], t_knobs(1),
     [{"variant": 0, "splitk": 5, "last": 30, "direct": False}], "1x1 stride 2 at odd input 25x43 (output 13x22)")
_add("tap-dil2-9x9", [R.conv(2, 9, 9, 64, 64, 3, 1, 2)], t_knobs(1),
     [{"variant": 0, "splitk": 3, "last": 34, "direct": False}], "dilated 3x3 (pad 2) at 9x9, two images")
for lay in ("slab1", "plain3", "s13of16"):
    _layout_case("tap-192to384-k3-%s" % lay, lay, _conv_on(192, 384, 3), {"TDN_WGRAD9": 0},
                 {"variant": 0, "tile": (128, 64)}, "Ktot = 1728: finalize K4 = 432 > K4P = 256, a second, partly active pass")
# Ktot = 64: finalize SL = 16 split lanes; 8, 13, 20 and 256 splits straddle the 4-way unroll (splitk > 3 * SL = 48)
for lay in LAYOUTS:
    _layout_case("tap-64to64-k1-%s" % lay, lay, _conv_on(64, 64, 1), {}, {"variant": 0, "tile": (64, 64)},
                 "1x1 64->64 on the default tile, finalize SL = 16")
for lay in ("lt64", "slab1", "twostep", "x8", "c9to5", "s20of24"):
    _layout_case("tap-64to64-k3-%s" % lay, lay, _conv_on(64, 64, 3), {"TDN_WGRAD9": 0},
                 {"variant": 0, "tile": (64, 64)}, "3x3 64->64 on the default tap tile")

# ---- nine-tap kernel: both variants, splits that start mid-row, mid-image, at H = 1 and H = 2 ------------------------------
T9_GRIDS = [(3, 5, 9), (2, 9, 8), (1, 3, 64), (1, 3, 65), (2, 3, 63), (5, 2, 8), (4, 1, 40), (2, 13, 21), (1, 13, 63),
            (1, 20, 63)]
for variant, cout in ((1, 128), (2, 64)):
    tile = (128 if variant == 1 else 64, 64)
    for grid in T9_GRIDS + ([(1, 127, 129)] if variant == 2 else []):
        M = grid[0] * grid[1] * grid[2]
        sk, mc = expected_split(M, 1)
        e = {"variant": variant, "tile": tile, "splitk": sk, "last": M - (sk - 1) * mc, "direct": sk == 1}
        if sk >= 8:
            e["idle"] = slots(sk) - sk
        _add("t9v%d-%dx%dx%d" % ((variant,) + grid), [R.conv(grid[0], grid[1], grid[2], 64, cout, 3)],
             t_knobs(1, TDN_WGRAD9=1), [e], "nine-tap 64->%d at T = 1: %d splits of %d px" % (cout, sk, mc))
    _layout_case("t9v%d-direct3" % variant, "direct3", _conv_on(64, cout, 3), {"TDN_WGRAD9": 1},
                 {"variant": variant, "tile": tile}, "nine-tap 64->%d, direct" % cout)
    _layout_case("t9v%d-slab1" % variant, "slab1", _conv_on(64, cout, 3), {"TDN_WGRAD9": 1},
                 {"variant": variant, "tile": tile}, "nine-tap 64->%d, one split through the slab" % cout)

# two ci tiles per co tile: column sums from tile_ci 0 only, one dot partial per ci tile on the direct path
for variant, cout in ((1, 128), (2, 64)):
    for lay in ("direct3", "plain3", "s13of16"):
        _layout_case("t9v%d-cin128-%s" % (variant, lay), lay, _conv_on(128, cout, 3), {"TDN_WGRAD9": 1},
                     {"variant": variant, "tile": (128 if variant == 1 else 64, 64)},
                     "nine-tap 128->%d: two ci tiles" % cout, bn=(True,))

# ---- stem: shape 0, map_mode 1, never direct ---------------------------------------------------------------------------------
_add("stem-n1-T1", [R.stem(1, 32, 48)], t_knobs(1), [{"variant": 0, "tile": (64, 32), "splitk": 6, "last": 64, "direct": False}],
     "stem 32x48, 6 splits")
_add("stem-n2-T1", [R.stem(2, 32, 48)], t_knobs(1),
     [{"variant": 0, "tile": (64, 32), "splitk": 12, "last": 64, "direct": False, "idle": 4}], "stem 2 x 32x48, 12 splits in 16 slots")
_add("stem-n1-default", [R.stem(1, 32, 48)], {}, [{"variant": 0, "tile": (64, 32), "direct": False}], "stem, default plan")
_add("stem-n2-default", [R.stem(2, 32, 48)], {}, [{"variant": 0, "tile": (64, 32), "direct": False}], "stem, default plan", bn=(True,))

# ---- grouped: map_mode 4 * cpg, never direct ---------------------------------------------------------------------------------
for groups in (32, 2):
    for stride in (1, 2):
        for lay in ("plain3", "s13of16"):
            _layout_case("gconv-g%d-s%d-%s" % (groups, stride, lay), lay,
                         (lambda G, S: lambda grid: R.gconv(grid[0], _in_size(grid[1], 3, S), _in_size(grid[2], 3, S),
                                                            128, G, 3, S))(groups, stride),
                         {}, {"variant": 0, "tile": (64, 64)}, "grouped 128 channels, %d groups, stride %d" % (groups, stride))

# ---- fp16: one case per kernel at a 2-7-split plan and at a plan with idle slots -----------------------------------------------
for lay in ("plain3", "s13of16"):
    _layout_case("f16-tap-s4-k3-%s" % lay, lay, _conv_on(64, 128, 3), {"TDN_WGRAD9": 0, "TDN_WGRAD_SHAPE": 4},
                 {"variant": 0, "tile": (128, 64)}, "fp16 tap-per-tile", dtype="f16")
    _layout_case("f16-t9v1-%s" % lay, lay, _conv_on(64, 128, 3), {"TDN_WGRAD9": 1}, {"variant": 1, "tile": (128, 64)},
                 "fp16 nine-tap, 128-channel tile", dtype="f16")
    _layout_case("f16-t9v2-%s" % lay, lay, _conv_on(64, 64, 3), {"TDN_WGRAD9": 1}, {"variant": 2, "tile": (64, 64)},
                 "fp16 nine-tap, 64-channel tile", dtype="f16")
    _layout_case("f16-gconv-g32-%s" % lay, lay, lambda grid: R.gconv(grid[0], grid[1], grid[2], 128, 32), {},
                 {"variant": 0, "tile": (64, 64)}, "fp16 grouped", dtype="f16")
_add("f16-stem-n1-T1", [R.stem(1, 32, 48)], t_knobs(1), [{"variant": 0, "tile": (64, 32), "splitk": 6, "direct": False}],
     "fp16 stem, 6 splits", dtype="f16", bn=(True,))
_add("f16-stem-n2-T1", [R.stem(2, 32, 48)], t_knobs(1), [{"variant": 0, "tile": (64, 32), "splitk": 12, "idle": 4, "direct": False}],
     "fp16 stem, 12 splits in 16 slots", dtype="f16", bn=(False,))

# ---- beta = 1 onto a known previous result ---------------------------------------------------------------------------------------
_layout_case("acc-direct", "direct3", _conv_on(64, 128, 1), {}, {"variant": 0}, "accumulate, direct member", bn=(True,),
             accumulate=True)
_layout_case("acc-slab-t9", "s13of16", _conv_on(64, 128, 3), {"TDN_WGRAD9": 1}, {"variant": 1}, "accumulate, slab member",
             bn=(True,), accumulate=True)
_add("acc-stem", [R.stem(2, 32, 48)], t_knobs(1), [{"variant": 0, "tile": (64, 32), "splitk": 12, "direct": False}],
     "accumulate, stem member", bn=(True,), accumulate=True)
_layout_case("acc-gconv", "plain3", lambda grid: R.gconv(grid[0], grid[1], grid[2], 128, 32), {}, {"variant": 0},
             "accumulate, grouped member", bn=(True,), accumulate=True)

# ---- one group call: every kernel in one launch list set, workgroup counts rounded for the XCD map ------------------------------------
_GROUP = [R.stem(2, 32, 48), R.gconv(1, 13, 63, 128, 32), R.conv(1, 13, 63, 64, 128, 3), R.conv(2, 13, 21, 64, 64, 3),
          R.conv(1, 13, 63, 64, 64, 1), R.conv(1, 20, 63, 64, 256, 1), R.conv(3, 5, 9, 64, 64, 1)]
_add("group-all-kernels", _GROUP, t_knobs(1),
     [{"variant": 0, "tile": (64, 32), "splitk": 12, "idle": 4, "direct": False},
      {"variant": 0, "tile": (64, 64), "splitk": 13, "idle": 3, "direct": False},
      {"variant": 1, "tile": (128, 64), "splitk": 13, "idle": 3},
      {"variant": 2, "tile": (64, 64), "splitk": 5, "last": 34},
      {"variant": 0, "tile": (64, 64), "splitk": 13, "idle": 3},
      {"variant": 0, "tile": (256, 64), "splitk": 20, "idle": 4},
      {"variant": 0, "tile": (64, 64), "splitk": 3, "last": 7}],
     "stem + grouped + both nine-tap variants + tap members of two shapes in one tdn_wgrad_group call",
     bn=(True, False, True, False, True, False, True))

IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def plan_problems(case, per):
    """The case's predicate on the rows of wgrad_group_plan: a list of what does not hold (empty: the plan is the one
    the case is for)."""
    bad = []
    assert len(per) == len(case.members)
    for i, (m, e, row) in enumerate(zip(case.members, case.expect, per)):
        variant, bmw, bnw, splitk, mchunk, direct, blocks = row[:7]
        M = R.pixels(m)

        def want(name, got, exp):
            if got != exp:
                bad.append("member %d (%s): %s is %s, the case needs %s (row %s)" % (i, m.kind, name, got, exp, row))
        if "variant" in e:
            want("variant", variant, e["variant"])
        if "tile" in e:
            want("tile", (bmw, bnw), tuple(e["tile"]))
        if "splitk" in e:
            want("splits", splitk, e["splitk"])
        if "last" in e:
            want("last split's pixels", M - (splitk - 1) * mchunk, e["last"])
        if "direct" in e:
            want("direct", bool(direct), e["direct"])
        if "idle" in e:
            want("idle slots", slots(splitk) - splitk, e["idle"])
        if "tiles" in e and splitk > 0:
            want("tiles per split", blocks // max(slots(splitk), 1), e["tiles"])
        if not (splitk >= 1 and mchunk % 64 == 0 and (splitk - 1) * mchunk < M <= splitk * mchunk):
            bad.append("member %d: splits %d x %d px do not cover %d pixels" % (i, splitk, mchunk, M))
    return bad


def shape_only_items(case):
    """tdn_wgrad_item structs for the host-only planner (it never dereferences the tensors)."""
    from torch_detection_amd import _lib
    kinds = {"conv": 0, "stem": 1, "gconv": 2}
    items = []
    for m, bn in zip(case.members, case.bn):
        it = _lib.WgradItem()
        it.x = it.g = it.w_fwd = it.dw = 256
        it.scale = it.mean = it.invstd = it.dgamma = (256 if bn else None)
        it.dbeta = 256
        it.beta = 1.0 if case.accumulate else 0.0
        it.kind = kinds[m.kind]
        it.N, it.H, it.W, it.Cin, it.Cout, it.k, it.stride, it.pad, it.groups = \
            m.N, m.H, m.W, m.Cin, m.Cout, m.k, m.stride, m.pad, m.groups
        items.append(it)
    return items
