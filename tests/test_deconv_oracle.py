"""CPU: the oracle of the 2x2 stride-2 transposed convolution (tests/deconv_ref.py) against ``F.conv_transpose2d`` and its
autograd in fp64 — which pins the column order (a, b, o) and the pixel shuffle independently of any GPU —, ``FCNMaskHead``'s
construction and state dict, the refusals of deconv_ops.py that need no device, and the host-only plan query."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import deconv_ref as R

BF16, F16 = torch.bfloat16, torch.float16
FWD, DGRAD, WGRAD = 0, 1, 2


@pytest.fixture(scope="module")
def T():
    import torch_detection_amd as T
    return T


@pytest.fixture(scope="module")
def D():
    from torch_detection_amd import deconv_ops
    return deconv_ops


def close(a, b):
    scale = b.abs().max().item() or 1.0
    return (a.double() - b.double()).abs().max().item() <= 1e-12 * scale


@pytest.mark.parametrize("shape", [(2, 3, 5, 8, 6), (1, 1, 1, 4, 4)], ids=str)
@pytest.mark.parametrize("relu", [False, True])
def test_oracle_is_conv_transpose2d(shape, relu):
    Rr, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(Rr, H, W, Cin, generator=g)
    w = torch.randn(Cin, Cout, 2, 2, generator=g)
    b = torch.randn(Cout, generator=g)
    gy = torch.randn(Rr, 2 * H, 2 * W, Cout, generator=g)
    xt = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = w.double().requires_grad_(True)
    bt = b.double().requires_grad_(True)
    z = F.conv_transpose2d(xt, wt, bt, stride=2)
    yt = z.clamp(min=0) if relu else z
    y = R.fwd(x, w, b, relu)
    assert tuple(y.shape) == (Rr, 2 * H, 2 * W, Cout) and y.dtype == torch.float64
    assert close(y, yt.detach().permute(0, 2, 3, 1))
    ge = gy * (z.detach().permute(0, 2, 3, 1) > 0) if relu else gy       # the cotangent behind the ReLU
    yt.backward(gy.double().permute(0, 3, 1, 2))
    assert close(R.dgrad(ge, w), xt.grad.permute(0, 2, 3, 1))
    dw, db = R.wgrad(x, ge)
    assert tuple(dw.shape) == (Cin, Cout, 2, 2) and close(dw, wt.grad)
    assert tuple(db.shape) == (Cout,) and close(db, bt.grad)


def test_shuffle_and_weight_views_are_inverses():
    y = torch.arange(2 * 6 * 10 * 3, dtype=torch.float32).view(2, 6, 10, 3)
    Y = R.unshuffle(y)
    assert tuple(Y.shape) == (2 * 3 * 5, 12)
    # row (r, i, j) = (1, 2, 4), column (a, b, o) = (1, 0, 2)
    assert Y[(1 * 3 + 2) * 5 + 4, (1 * 2 + 0) * 3 + 2] == y[1, 2 * 2 + 1, 2 * 4 + 0, 2]
    assert torch.equal(R.shuffle(Y, 2, 3, 5), y)
    w = torch.arange(4 * 3 * 2 * 2, dtype=torch.float32).view(4, 3, 2, 2)
    m = R.w2d(w)
    assert tuple(m.shape) == (12, 4) and m[(1 * 2 + 0) * 3 + 2, 1] == w[1, 2, 1, 0]
    assert torch.equal(R.w4d(m), w)


# ---- FCNMaskHead on the CPU ---------------------------------------------------------------------------------------------
def test_mask_head_state_dict_and_registry(T):
    head = T.FCNMaskHead()
    want = {"upsample.weight": (256, 256, 2, 2), "upsample.bias": (256,),
            "conv_logits.weight": (81, 256, 1, 1), "conv_logits.bias": (81,)}
    for i in range(4):
        want["convs.%d.conv.weight" % i] = (256, 256, 3, 3)
        want["convs.%d.conv.bias" % i] = (256,)
    got = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert got == want
    assert not head.upsample.bias.abs().sum().item() and not head.conv_logits.bias.abs().sum().item()
    assert T.FCNMaskHead(class_agnostic=True).conv_logits.weight.shape[0] == 1

    class Reference(nn.Module):
        def __init__(self):
            super().__init__()
            self.convs = nn.ModuleList(T.ConvModule(256, 256, 3, padding=1) for _ in range(4))
            self.upsample = nn.ConvTranspose2d(256, 256, 2, stride=2)
            self.conv_logits = nn.Conv2d(256, 81, 1)

    sd = Reference().state_dict()
    assert head.load_state_dict(sd, strict=True) is not None
    assert torch.equal(head.upsample.weight, sd["upsample.weight"])
    assert T.HEADS.module_dict["FCNMaskHead"] is T.FCNMaskHead
    built = T.HEADS.build(dict(type="FCNMaskHead", num_convs=1, in_channels=64, conv_out_channels=64, num_classes=5))
    assert isinstance(built, T.FCNMaskHead) and len(built.convs) == 1


@pytest.mark.parametrize("kwargs", [dict(upsample_method="nearest"), dict(in_channels=100, conv_out_channels=100),
                                    dict(upsample_ratio=4)], ids=str)
def test_mask_head_refuses_at_forward_only(T, kwargs):
    head = T.FCNMaskHead(num_convs=1, **kwargs)                     # construction succeeds
    with pytest.raises(NotImplementedError):
        head(torch.zeros(1, head.in_channels, 14, 14, dtype=BF16))


# ---- refusals of the raw ops that need no device ---------------------------------------------------------------------------
def cl(*shape, dtype=BF16):
    return torch.zeros(*shape, dtype=dtype).contiguous(memory_format=torch.channels_last)


def test_host_refusals_name_the_argument(D):
    x, wf, wd = cl(2, 64, 3, 5), torch.zeros(256, 64, dtype=BF16), torch.zeros(64, 256, dtype=BF16)
    g = cl(2, 64, 6, 10)
    with pytest.raises(ValueError, match=r"^x must be"):                               # a wrong dtype
        D.deconv2x2_fwd(cl(2, 64, 3, 5, dtype=torch.float32), wf)
    with pytest.raises(ValueError, match=r"^x must be .*channels_last"):               # NCHW-contiguous memory
        D.deconv2x2_fwd(torch.zeros(2, 64, 3, 5, dtype=BF16), wf)
    with pytest.raises(ValueError, match=r"^w_fwd must be"):                           # the other 16-bit dtype
        D.deconv2x2_fwd(x, wf.to(F16))
    with pytest.raises(ValueError, match=r"^Cin must be a multiple of 64"):
        D.deconv2x2_fwd(cl(2, 96, 3, 5), torch.zeros(256, 96, dtype=BF16))
    with pytest.raises(ValueError, match=r"^Cin must be a multiple of 64"):
        D.pack_deconv_weight(torch.zeros(96, 64, 2, 2))
    with pytest.raises(ValueError, match=r"^weight must be"):
        D.pack_deconv_weight(torch.zeros(64, 64, 3, 3))
    with pytest.raises(ValueError, match=r"^bias must be"):
        D.deconv2x2_fwd(x, wf, torch.zeros(63))
    with pytest.raises(ValueError, match=r"^g must be"):                               # 2W is 10, not 9
        D.deconv2x2_wgrad(x, cl(2, 64, 6, 9))
    with pytest.raises(ValueError, match=r"^g must be"):
        D.deconv2x2_dgrad(cl(2, 64, 5, 10), wd)
    with pytest.raises(ValueError, match=r"^w_dgrad must be"):
        D.deconv2x2_dgrad(g, torch.zeros(64, 128, dtype=BF16))
    with pytest.raises(ValueError, match=r"^splits must be in 0\.\.1"):                # M = 30: one chunk of 64 pixels
        D.deconv2x2_wgrad(x, g, splits=2)
    with pytest.raises(ValueError, match=r"^dw must be"):
        D.deconv2x2_wgrad(x, g, dw=torch.zeros(64, 64, 4))
    with pytest.raises(ValueError, match=r"^dw must be given"):
        D.deconv2x2_wgrad(x, g, beta=1.0)
    with pytest.raises(ValueError, match=r"^x must be a CUDA tensor"):                 # everything else is fine: the device
        D.deconv2x2_fwd(x, wf)


def test_conv_transpose2x2_checks_its_parameters_first(T):
    x = cl(2, 64, 3, 5)
    with pytest.raises(ValueError, match=r"^weight must be"):
        T.conv_transpose2x2(x, torch.zeros(32, 64, 2, 2))
    with pytest.raises(ValueError, match=r"^bias must be"):
        T.conv_transpose2x2(x, torch.zeros(64, 64, 2, 2), torch.zeros(65))


# ---- the plan (host only) ----------------------------------------------------------------------------------------------
def test_plan_of_the_heads_own_geometry(D):
    pl = D.deconv2x2_plan(FWD, 2, 14, 14, 256, 256)
    assert (pl.bm, pl.bn, pl.bk) == (128, 128, 64)
    assert (pl.tiles_r, pl.tiles_c, pl.tiles, pl.workgroups) == (4, 8, 32, 32)
    assert (pl.slices, pl.chunks, pl.launches, pl.workspace_bytes) == (1, 4, 1, 0)
    pl = D.deconv2x2_plan(DGRAD, 2, 14, 14, 256, 256)
    assert (pl.tiles_r, pl.tiles_c, pl.chunks, pl.launches, pl.workspace_bytes) == (4, 2, 16, 1, 0)
    # wgrad: 4 Cout x Cin = 8 x 2 tiles; 7 chunks of 64 pixels are too few to cut (at least 4 per slice)
    pl = D.deconv2x2_plan(WGRAD, 2, 14, 14, 256, 256)
    assert (pl.tiles_r, pl.tiles_c, pl.chunks, pl.slices, pl.launches) == (8, 2, 7, 1, 2)
    assert pl.workspace_bytes == 4 * (1024 * 256 + 1024)
    # the training batch: 392 chunks over 16 tiles -> 16 slices of 25 chunks, 256 workgroups
    pl = D.deconv2x2_plan(WGRAD, 128, 14, 14, 256, 256)
    assert (pl.chunks, pl.slices, pl.chunks_per_slice, pl.workgroups) == (392, 16, 25, 256)
    assert pl.slab_bytes == 16 * 1024 * 256 * 4
    assert D.deconv2x2_plan(WGRAD, 3, 5, 7, 128, 64, splits=2).slices == 2            # M = 105: two chunks
    assert D.deconv2x2_plan(WGRAD, 2, 14, 14, 256, 256, splits=3).slices == 3
    # the empty batch: only wgrad's finalize runs
    assert D.deconv2x2_plan(FWD, 0, 14, 14, 64, 64).launches == 0
    pl = D.deconv2x2_plan(WGRAD, 0, 14, 14, 64, 64)
    assert (pl.slices, pl.launches, pl.workspace_bytes) == (0, 1, 0)


def test_plan_refusals_come_through_tdn_last_error(D):
    from torch_detection_amd import _lib
    with pytest.raises(ValueError, match="Cout=100 must be a multiple of 64"):
        D.deconv2x2_plan(FWD, 2, 14, 14, 256, 100)
    assert b"Cout=100" in _lib.load().tdn_last_error()
    assert _lib.load().tdn_deconv2x2_workspace_bytes(WGRAD, 2, 14, 14, 96, 64, 0) == -1
    assert b"Cin=96" in _lib.load().tdn_last_error()
    with pytest.raises(ValueError, match="must be below 2\\^31"):
        D.deconv2x2_plan(FWD, 1 << 14, 14, 14, 256, 256)
    with pytest.raises(ValueError, match="splits=8 out of range 0..7"):
        D.deconv2x2_plan(WGRAD, 2, 14, 14, 256, 256, splits=8)
    with pytest.raises(ValueError, match="H=0"):
        D.deconv2x2_plan(FWD, 2, 0, 14, 64, 64)
