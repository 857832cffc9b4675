"""CPU: the oracle and bounds of tests/pyramid_conv_ref.py pinned to torch's own float64 autograd, the host side of
``pyramid_ops`` (refusals before any GPU is touched, the plan's invariants, the ctypes struct against the header) and
``RetinaHead``'s constructor, state dict, initialisation and ``_check_supported``."""
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import pyramid_conv_ref as R

BF16, F16 = torch.bfloat16, torch.float16
FWD, DGRAD, WGRAD = 0, 1, 2
WORKLOAD = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


def _tiny(dtype=BF16, B=2, sizes=((5, 4), (3, 2), (1, 1)), Cin=8, Cout=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: R.round16(torch.randn(*s, generator=g), dtype)
    xs = [r(B, H, W, Cin) for H, W in sizes]
    gs = [r(B, H, W, Cout) for H, W in sizes]
    ms = [r(B, H, W, Cin) for H, W in sizes]
    ad = [r(B, H, W, Cin) for H, W in sizes]
    for m in ms:
        m[torch.rand(m.shape, generator=g) < 0.3] = 0
    return xs, gs, ms, ad, r(Cout, Cin, 3, 3) / 4, torch.randn(Cout, generator=g)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
def test_oracle_is_float64_autograd_of_conv2d(relu):
    xs, gs, ms, ad, w, b = _tiny()
    xv = [R.nchw(x).double().requires_grad_(True) for x in xs]
    wv, bv = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ys = [F.conv2d(x, wv, bv, 1, 1) for x in xv]
    ys = [y.clamp(min=0) for y in ys] if relu else ys
    for y, mine in zip(ys, R.fwd(xs, w, b, relu)):
        assert torch.equal(R.nhwc(y.detach()), mine)
    # cotangents masked like a ReLU's own backward, so that autograd of the plain conv gives the unmasked products
    lin = [F.conv2d(x, wv, bv, 1, 1) for x in xv]
    grads = torch.autograd.grad(lin, xv + [wv, bv], [R.nchw(g).double() for g in gs])
    dxs = R.dgrad(gs, w)
    for d, mine in zip(grads[:len(xs)], dxs):
        assert torch.allclose(R.nhwc(d), mine, rtol=1e-13, atol=1e-13)
    dw, db = R.wgrad(xs, gs)
    assert torch.allclose(grads[-2], dw, rtol=1e-13, atol=1e-13) and torch.allclose(grads[-1], db, rtol=1e-13, atol=1e-13)
    # mask and addend: added before the mask, exact zeros where the mask source is <= 0
    full = R.dgrad(gs, w, ms, ad)
    for d, plain, m, a in zip(full, dxs, ms, ad):
        assert torch.allclose(d, (plain + a.double()) * (m > 0).double(), rtol=1e-13, atol=1e-13)
        assert (d[m <= 0] == 0).all() and (m <= 0).any()
    some = R.dgrad(gs, w, [ms[0], None, None], [None, ad[1], None])
    assert torch.equal(some[2], dxs[2]) and torch.allclose(some[1], dxs[1] + ad[1].double(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_bounds_admit_an_fp32_evaluation_of_the_same_sums(dtype):
    xs, gs, ms, ad, w, b = _tiny(dtype, Cin=16, Cout=7, seed=3)
    for relu in (False, True):
        for x, bd in zip(xs, R.fwd_bounds(xs, w, b, relu)):
            y = F.conv2d(R.nchw(x), w, b, 1, 1)
            r = R.within((y.clamp(min=0) if relu else y).to(dtype), bd, dtype, "fp32 forward")
            assert r["T"] == 16 * 9 + 1
    for g, m, a, bd in zip(gs, ms, ad, R.dgrad_bounds(gs, w, ms, ad)):
        d = (F.conv_transpose2d(R.nchw(g), w, None, 1, 1) + R.nchw(a)) * (R.nchw(m) > 0)
        r = R.within(d.to(dtype), bd, dtype, "fp32 dgrad")
        assert r["T"] == 7 * 9 + 1
    # the level sum: fp32 per-level weight gradients added in level order
    dw = sum(torch.nn.grad.conv2d_weight(R.nchw(x), w.shape, R.nchw(g), 1, 1) for x, g in zip(xs, gs))
    bd = R.wgrad_bound(xs, gs)
    assert bd.T == sum(x.shape[0] * x.shape[1] * x.shape[2] for x in xs)
    assert torch.allclose(bd.v, R.wgrad(xs, gs)[0], rtol=1e-13, atol=1e-13)
    R.within(dw, bd, torch.float32, "fp32 wgrad")
    R.within(sum(g.sum((0, 1, 2)) for g in gs), R.dbias_bound(gs), torch.float32, "fp32 dbias")
    # and a wrong element is seen
    dw[3, 2, 1, 0] += 0.05 * float(bd.S[3, 2, 1, 0])
    with pytest.raises(AssertionError):
        R.within(dw, bd, torch.float32, "perturbed wgrad")


# ---- host refusals --------------------------------------------------------------------------------------------------------
def _cl(B, C, H, W, dtype=BF16):
    return torch.zeros(B, H, W, C, dtype=dtype).permute(0, 3, 1, 2)


def test_wrappers_refuse_before_any_gpu_is_touched():
    from torch_detection_amd import pyramid_ops as P
    w_fwd = torch.zeros(64, 3, 3, 64, dtype=BF16)
    b = torch.zeros(36)
    ok = [_cl(2, 64, 4, 4), _cl(2, 64, 2, 2)]
    cases = [
        (lambda: P.pyramid_conv_fwd([_cl(2, 64, 4, 4, torch.float32)], w_fwd, b, 36), r"xs\[0\]"),          # dtype
        (lambda: P.pyramid_conv_fwd([torch.zeros(2, 64, 4, 4, dtype=BF16)], w_fwd, b, 36), r"xs\[0\].*channels_last"),
        (lambda: P.pyramid_conv_fwd([_cl(2, 96, 4, 4)], w_fwd, b, 36), r"Cin"),
        (lambda: P.pyramid_conv_fwd(ok, w_fwd, None, 0), r"Cout"),
        (lambda: P.pyramid_conv_fwd(ok, w_fwd, None, 1025), r"Cout"),
        (lambda: P.pyramid_conv_fwd([_cl(1, 64, 1, 1)] * 9, w_fwd, b, 36), r"xs must be a list of 1\.\.8"),
        (lambda: P.pyramid_conv_fwd([], w_fwd, b, 36), r"xs must be a list of 1\.\.8"),
        (lambda: P.pyramid_conv_fwd([ok[0], _cl(3, 64, 2, 2)], w_fwd, b, 36), r"xs\[1\]"),                  # mismatched B
        (lambda: P.pyramid_conv_fwd([ok[0], _cl(2, 128, 2, 2)], w_fwd, b, 36), r"xs\[1\]"),
        (lambda: P.pyramid_conv_fwd(ok, w_fwd, torch.zeros(35), 36), r"bias"),
        (lambda: P.pyramid_conv_fwd(ok, torch.zeros(64, 3, 3, 64, dtype=F16), b, 36), r"w_fwd"),
        (lambda: P.pyramid_conv_fwd(ok, torch.zeros(36, 3, 3, 64, dtype=BF16), b, 36), r"w_fwd"),
        (lambda: P.pyramid_conv_wgrad(ok, [_cl(2, 36, 4, 4)]), r"gs must have one entry per level"),        # missing level
        (lambda: P.pyramid_conv_wgrad(ok, [_cl(2, 36, 4, 4), _cl(2, 36, 2, 3)]), r"gs\[1\]"),
        (lambda: P.pyramid_conv_dgrad([_cl(2, 36, 4, 4)], torch.zeros(64, 3, 3, 128, dtype=BF16)), r"w_dgrad"),
        (lambda: P.pyramid_conv_dgrad([_cl(2, 36, 4, 4)], torch.zeros(64, 3, 3, 64, dtype=BF16), [ok[0], ok[1]]),
         r"mask_src must have one entry per level"),
        (lambda: P.pyramid_conv_dgrad([_cl(2, 36, 4, 4)], torch.zeros(64, 3, 3, 64, dtype=BF16), None, [_cl(2, 64, 4, 5)]),
         r"addend\[0\]"),
        (lambda: P.pack_pyramid_weight(torch.zeros(36, 64, 3, 3, dtype=torch.float64)), r"^w must"),
        (lambda: P.pack_pyramid_weight(torch.zeros(36, 96, 3, 3)), r"Cin"),
        (lambda: P.pack_pyramid_weight(torch.zeros(1025, 64, 3, 3)), r"Cout"),
        (lambda: P.pack_pyramid_weight(torch.zeros(36, 64, 1, 1)), r"^w must"),
        (lambda: P.pack_pyramid_weight(torch.zeros(36, 64, 3, 3), dtype=torch.float32), r"compute dtype"),
        (lambda: P.pyramid_conv_plan(3, 1, [(1, 1)], 64, 1), r"kind"),
        (lambda: P.pyramid_conv_plan(0, 1, [(1, 1)] * 9, 64, 1), r"sizes must be a list of 1\.\.8"),
        (lambda: P.pyramid_conv_plan(0, 1, [(0, 1)], 64, 1), r"sizes\[0\]"),
        (lambda: P.pyramid_conv_plan(0, -1, [(1, 1)], 64, 1), r"^B "),
        (lambda: P.pyramid_conv_plan(0, 1 << 12, [(1 << 10, 1 << 10)], 64, 1), r"B\*H\*W"),
    ]
    for i, (call, pat) in enumerate(cases):
        with pytest.raises(ValueError, match=pat):
            call()
    # every size and dtype in order: the only thing left to refuse is the device
    with pytest.raises(ValueError, match="must be a CUDA tensor"):
        P.pyramid_conv_fwd(ok, w_fwd, b, 36)
    with pytest.raises(ValueError, match="must be a CUDA tensor"):
        P.pyramid_conv_wgrad(ok, [_cl(2, 36, 4, 4).float().contiguous(), _cl(2, 36, 2, 2)])    # a cotangent is copied, then refused
    with pytest.raises(ValueError, match="must be a CUDA tensor"):
        P.pack_pyramid_weight(torch.zeros(36, 64, 3, 3))


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


@pytest.mark.parametrize("B,sizes", [(2, WORKLOAD), (1, [(1, 1)]), (3, [(9, 8), (5, 4), (3, 2), (1, 1)]), (0, [(4, 4), (2, 2)]),
                                     (1, [(1, 1)] * 8)])
@pytest.mark.parametrize("Cin,Cout", [(256, 256), (256, 720), (256, 36), (64, 1), (512, 1024), (64, 65)])
def test_plan_invariants(B, sizes, Cin, Cout):
    from torch_detection_amd import pyramid_ops as P
    rows = [B * H * W for H, W in sizes]
    Cp = _cdiv(Cout, 64) * 64
    for kind in (FWD, DGRAD):
        pl = P.pyramid_conv_plan(kind, B, sizes, Cin, Cout)
        assert pl.pixels_per_workgroup == 128 and pl.cols_per_workgroup == 64 and pl.Cp == Cp
        # the tiles cover every pixel of every level exactly once: a level's tiles are its own, whole and in order
        assert pl.pixel_tiles == sum(_cdiv(r, pl.pixels_per_workgroup) for r in rows)
        assert pl.col_tiles == (Cp if kind == FWD else Cin) // 64
        assert pl.workgroups == pl.pixel_tiles * pl.col_tiles
        assert pl.Kp == (Cin if kind == FWD else Cp) and pl.Kp % 64 == 0
        assert pl.launches == (1 if sum(rows) else 0) and pl.slices == 0 and pl.workspace_bytes == 0
        assert pl.lds_bytes == 2 * 64 * 64 * 2
    pl = P.pyramid_conv_plan(WGRAD, B, sizes, Cin, Cout)
    units = (Cp // 64) * 9 * (Cin // 64)
    target = min(64, _cdiv(1024, units))
    per = max(128, _cdiv(_cdiv(sum(rows), target), 128) * 128)
    assert pl.col_tiles == units and pl.pixels_per_slice == per
    assert pl.slices == sum(_cdiv(r, per) for r in rows) and pl.workgroups == pl.slices * units
    assert pl.launches == (2 if sum(rows) else 1)
    assert pl.slab_bytes == pl.slices * Cp * 9 * Cin * 4
    a256 = lambda n: _cdiv(n, 256) * 256
    assert pl.workspace_bytes == (a256(pl.slab_bytes) + a256(pl.slices * Cp * 4) if pl.slices else 0)
    # the slices depend on the shapes alone: the same answer again, and nothing about a device went in
    again = P.pyramid_conv_plan(WGRAD, B, sizes, Cin, Cout)
    assert all(getattr(pl, s) == getattr(again, s) for s in pl.__slots__)


def test_workload_slabs_stay_beside_the_operands():
    from torch_detection_amd import pyramid_ops as P
    pl = P.pyramid_conv_plan(WGRAD, 2, WORKLOAD, 256, 720)
    pixels = 2 * sum(H * W for H, W in WORKLOAD)
    operands = pixels * (256 + 720) * 2
    assert pixels == 44800 and pl.slices == 7 and pl.slab_bytes == 7 * 768 * 2304 * 4 < operands


def test_struct_mirror_matches_the_header():
    from torch_detection_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "include", "tdn.h")).read()
    body = re.search(r"typedef struct tdn_pyr_level \{(.*?)\} tdn_pyr_level;", src, re.S).group(1)
    fields = [re.match(r"\s*(.*?)\s*(\w+);", line).groups() for line in body.strip().splitlines()]
    assert [n for _, n in fields] == [n for n, _ in _lib.PyrLevel._fields_] == ["x", "y", "dx", "mask_src", "addend", "H", "W"]
    for (ctype, name), (_, mirror) in zip(fields, _lib.PyrLevel._fields_):
        assert (mirror is ctypes.c_void_p) == ctype.endswith("*") and (mirror is ctypes.c_int32) == (ctype == "int32_t"), name
    assert ctypes.sizeof(_lib.PyrLevel) == 5 * 8 + 2 * 4 and _lib.PyrLevel.H.offset == 40 and _lib.PyrLevel.W.offset == 44
    assert "#define TDN_PYR_MAX_LEVELS %d" % _lib.PYR_MAX_LEVELS in src


# ---- RetinaHead -----------------------------------------------------------------------------------------------------------
def test_retina_head_constructor_state_dict_and_init():
    import torch_detection_amd as T
    assert T.HEADS.module_dict["RetinaHead"] is T.RetinaHead
    torch.manual_seed(0)
    head = T.RetinaHead(num_classes=81, in_channels=256)
    assert (head.cls_out_channels, head.feat_channels, head.stacked_convs, head.num_anchors) == (80, 256, 4, 9)
    assert head.anchor_scales == [4 * 2 ** (i / 3) for i in range(3)] and head.anchor_strides == [8, 16, 32, 64, 128]
    assert len(head.anchor_generators) == 5 and head.anchor_base_sizes == head.anchor_strides
    want = {}
    for tower in ("cls_convs", "reg_convs"):
        for i in range(4):
            want["%s.%d.conv.weight" % (tower, i)] = (256, 256, 3, 3)
            want["%s.%d.conv.bias" % (tower, i)] = (256,)
    want.update({"retina_cls.weight": (720, 256, 3, 3), "retina_cls.bias": (720,), "retina_reg.weight": (36, 256, 3, 3),
                 "retina_reg.bias": (36,)})
    sd = head.state_dict()
    assert list(sd.keys()) == list(want.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert [n for n, _ in head.named_parameters()] == list(want.keys())
    # normal(0, 0.01) weights, zero biases, the focal prior on the classification bias
    for k, v in sd.items():
        if k.endswith("weight"):
            assert abs(float(v.mean())) < 1e-3 and 0.009 < float(v.std()) < 0.011, k
            assert v.permute(0, 2, 3, 1).is_contiguous(), k                   # K-major, like the conv modules
        elif k != "retina_cls.bias":
            assert not v.any(), k
    assert torch.equal(sd["retina_cls.bias"], torch.full((720,), -math.log((1 - 0.01) / 0.01)))
    small = T.RetinaHead(4, 64, feat_channels=128, stacked_convs=1, scales_per_octave=2, anchor_ratios=(1.0,),
                         anchor_strides=(8, 16))
    assert tuple(small.retina_cls.weight.shape) == (6, 128, 3, 3) and tuple(small.retina_reg.weight.shape) == (8, 128, 3, 3)
    assert tuple(small.cls_convs[0].conv.weight.shape) == (128, 64, 3, 3)
    none = T.RetinaHead(2, 64, stacked_convs=0)
    assert tuple(none.retina_cls.weight.shape) == (9, 64, 3, 3) and len(none.cls_convs) == 0
    # a state dict built by hand in mmdetection's naming loads
    by_hand = {k: torch.full(s, 0.5) for k, s in want.items()}
    head.load_state_dict(by_hand)
    assert float(head.reg_convs[3].conv.weight.detach().min()) == 0.5
    with pytest.raises(ValueError):
        T.RetinaHead(1, 64)
    with pytest.raises(ValueError):
        T.RetinaHead(4, 64, anchor_base_sizes=(8,))


def test_retina_head_refuses_what_is_not_on_the_hip_path():
    import torch_detection_amd as T
    x = [torch.zeros(1, 64, 2, 2)]
    for kw, pat in ((dict(in_channels=64, norm_cfg=dict(type="GN")), "norm_cfg"), (dict(in_channels=64, conv_cfg=dict()), "conv_cfg"),
                    (dict(in_channels=96), "in_channels=96"), (dict(in_channels=64, feat_channels=576), "feat_channels=576"),
                    (dict(in_channels=64, feat_channels=100), "feat_channels=100"),
                    (dict(in_channels=64, num_classes=200), r"A \* cls_out_channels = 1791"),
                    (dict(in_channels=64, scales_per_octave=90), "4A = 1080")):
        args = dict(num_classes=4)
        args.update(kw)
        head = T.RetinaHead(**args)                                           # accepted by the constructor
        with pytest.raises(NotImplementedError, match=pat):
            head(x)
    head = T.RetinaHead(4, 64, anchor_strides=(8,) * 9)
    with pytest.raises(NotImplementedError, match="1..8 levels"):
        head([torch.zeros(1, 64, 1, 1)] * 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # everything else in order: no CPU path
        T.RetinaHead(4, 64)(x)
