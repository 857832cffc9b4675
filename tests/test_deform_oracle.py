"""CPU: the deformable-convolution oracle (tests/deform_ref.py) pinned independently of the library — against
``F.conv2d``, shifted inputs and float64 autograd through ``F.grid_sample`` —, and the library's CPU surface: modules,
state-dict keys, argument refusals before any launch, the workspace size."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deform_cases as DC
import deform_ref as R

BF16, F16 = torch.bfloat16, torch.float16


def _rand(shape, seed, scale=1.0):
    return np.random.default_rng(seed).standard_normal(shape) * scale


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dil", [1, 2])
def test_zero_offsets_and_unit_mask_are_a_plain_convolution(stride, dil):
    N, C, H, W, Cout = 2, 16, 9, 11, 8
    x, w, b = _rand((N, C, H, W), 1), _rand((Cout, C, 3, 3), 2), _rand((Cout,), 3)
    Ho, Wo = R.out_size(H, stride, dil), R.out_size(W, stride, dil)
    for dg in (1, 2):
        off = np.zeros((N, 18 * dg, Ho, Wo), dtype=np.float32)
        for mask in (None, np.ones((N, 9 * dg, Ho, Wo), dtype=np.float32)):
            y = R.forward64(x, off, w, b, mask, stride, dil, dg)
            ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride, dil, dil)
            assert tuple(y.shape) == tuple(ref.shape)
            assert np.abs(y - ref.numpy()).max() < 1e-12


def test_integer_offsets_are_a_convolution_over_the_shifted_input():
    N, C, H, W, Cout = 1, 8, 9, 11, 4
    x, w = _rand((N, C, H, W), 4), _rand((Cout, C, 3, 3), 5)
    for sy, sx in ((2, -3), (-1, 0), (0, 5), (-9, 2), (3, 11)):
        off = np.zeros((N, 9, 2, H, W), dtype=np.float32)
        off[:, :, 0], off[:, :, 1] = sy, sx
        y = R.forward64(x, off.reshape(N, 18, H, W), w, None, None, 1, 1, 1)
        # x[p + s + k - 1] with zeros outside the map: a 'valid' conv over x zero padded by M on every side, read at
        # the window that starts at M - 1 + s
        M = 13
        full = F.conv2d(F.pad(torch.from_numpy(x), (M, M, M, M)), torch.from_numpy(w)).numpy()
        ref = full[:, :, M - 1 + sy:M - 1 + sy + H, M - 1 + sx:M - 1 + sx + W]
        assert np.abs(y - ref).max() < 1e-12, (sy, sx)


@pytest.mark.parametrize("stride,pad,dg", [(1, 1, 1), (2, 1, 2), (1, 2, 4), (2, 2, 1)])
def test_forward_and_gradients_equal_float64_autograd_through_grid_sample(stride, pad, dg):
    """Random non-integer positions; the offsets are multiples of 2^-10, so that the float32 position of the spec is the
    exact sum and the two formulations see the same point."""
    N, C, H, W, Cout = 2, 16 * dg, 13, 19, 8
    Ho, Wo = R.out_size(H, stride, pad), R.out_size(W, stride, pad)
    x, w, b = _rand((N, C, H, W), 6), _rand((Cout, C, 3, 3), 7), _rand((Cout,), 8)
    off = np.round(_rand((N, 18 * dg, Ho, Wo), 9, 4.0) * 1024.0) / 1024.0 + 2.0 ** -11      # never an integer
    mask = np.random.default_rng(10).uniform(0.1, 1.0, (N, 9 * dg, Ho, Wo)).astype(np.float32).astype(np.float64)
    P = R.Positions(off, H, W, stride, pad, dg)
    assert 0.3 < P.in_range_share() < 0.95 and not np.any(P.ly[P.valid] == 0) and not np.any(P.lx[P.valid] == 0)
    ts = [torch.from_numpy(a).requires_grad_() for a in (x, off, mask)]
    y = R.deform_conv_autograd(ts[0], ts[1], torch.from_numpy(w), torch.from_numpy(b), ts[2], stride, pad, dg)
    y64 = R.forward64(x, off, w, b, mask, stride, pad, dg)
    assert np.abs(y.detach().numpy() - y64).max() < 1e-10
    gy = torch.from_numpy(_rand(tuple(y.shape), 11))
    y.backward(gy)
    wk = torch.from_numpy(w).reshape(Cout, C, 9).permute(0, 2, 1)
    dcol = torch.einsum("nohw,okc->nhwkc", gy, wk).numpy()
    G = R.Grads(x, off, dcol, mask, stride, pad, dg)
    assert np.abs(G.dx - ts[0].grad.numpy()).max() < 1e-10
    assert np.abs(G.doffset - ts[1].grad.numpy()).max() < 1e-10
    assert np.abs(G.dmask - ts[2].grad.numpy()).max() < 1e-10
    # the logit's gradient is the mask's times s (1 - s)
    logit = np.log(mask / (1.0 - mask + 1e-3)).astype(np.float32)
    s = 1.0 / (1.0 + np.exp(-logit.astype(np.float64)))
    GL = R.Grads(x, off, dcol, logit, stride, pad, dg, mask_is_logit=True)
    GM = R.Grads(x, off, dcol, s, stride, pad, dg)          # (s as float32: the values differ by 2^-24 relative)
    assert np.abs(GL.dmask - GM.dmask * s * (1 - s)).max() < 1e-5 * np.abs(GL.dmask).max()


def test_validity_rule_at_the_borders_and_for_non_finite_offsets():
    H, W = 5, 7
    x = np.ones((1, 8, H, W), dtype=np.float32)
    # tap 4 (the centre) of output pixel (0, 0) sits at (0, 0): its offset IS the position
    def at(dy, dx):
        off = np.zeros((1, 18, H, W), dtype=np.float32)
        off[0, 8, 0, 0], off[0, 9, 0, 0] = dy, dx
        P = R.Positions(off, H, W, 1, 1, 1)
        cols = R.sample(x, off, None, 1, 1, 1, BF16)
        return bool(P.valid[0, 0, 4, 0, 0]), float(cols[0, 0, 0, 4, 0])
    assert at(0.0, 0.0) == (True, 1.0)
    assert at(-1.0, 0.0) == (False, 0.0) and at(0.0, -1.0) == (False, 0.0)
    assert at(float(H), 0.0) == (False, 0.0) and at(0.0, float(W)) == (False, 0.0)
    assert at(-1.0 + 2.0 ** -20, 0.0) == (True, float(torch.tensor(2.0 ** -20).bfloat16()))
    assert at(H - 0.5, 0.0) == (True, 0.5) and at(H - 1.0, W - 1.0) == (True, 1.0)
    for bad in (float("nan"), float("inf"), float("-inf"), 1e30, -1e30):
        assert at(bad, 0.0) == (False, 0.0) and at(0.0, bad) == (False, 0.0)
    # an invalid sample has no gradient anywhere
    off = np.zeros((1, 18, H, W), dtype=np.float32)
    off[0, 8, 0, 0] = np.nan
    dcol = np.zeros((1, H, W, 9, 8))
    dcol[0, 0, 0, 4] = 1.0
    G = R.Grads(x, off, dcol, None, 1, 1, 1)
    assert not G.dx.any() and not G.doffset.any() and np.isfinite(G.dx).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_gpu_cases_keep_their_in_range_share(seed):
    for hw, stride, pad in DC.GEOMETRIES:
        for C, dg in DC.CHANNELS:
            c = DC.make(seed, hw, stride, pad, C, dg, BF16)
            share = R.Positions(c.offset, c.H, c.W, stride, pad, dg).in_range_share()
            assert DC.SHARE[0] < share < DC.SHARE[1], (hw, stride, pad, C, dg, share)


# ---- the library's CPU surface ----------------------------------------------------------------------------------------
def test_modules_construct_with_mmdetection_parameter_names_and_zero_offset_convs():
    import torch_detection_amd as tda
    want = {tda.DeformConv: ["weight"], tda.ModulatedDeformConv: ["weight", "bias"],
            tda.DeformConvPack: ["weight", "conv_offset.weight", "conv_offset.bias"],
            tda.ModulatedDeformConvPack: ["weight", "bias", "conv_offset_mask.weight", "conv_offset_mask.bias"]}
    for cls, keys in want.items():
        m = cls(64, 128, 3, stride=2, padding=2, dilation=2, deformable_groups=2, bias="bias" in keys)
        assert list(m.state_dict().keys()) == keys, cls.__name__
        assert tuple(m.weight.shape) == (128, 64, 3, 3) and m.weight.dtype == torch.float32
        if "bias" in keys:
            assert tuple(m.bias.shape) == (128,)
        else:
            assert m.bias is None
    p = tda.DeformConvPack(64, 64, 3, padding=1, deformable_groups=4)
    assert tuple(p.conv_offset.weight.shape) == (72, 64, 3, 3) and p.conv_offset.bias is not None
    assert not p.conv_offset.weight.any() and not p.conv_offset.bias.any()
    q = tda.ModulatedDeformConvPack(64, 64, 3, stride=2, padding=2, dilation=2, deformable_groups=2, bias=True)
    co = q.conv_offset_mask
    assert tuple(co.weight.shape) == (54, 64, 3, 3) and co.stride == (2, 2) and co.padding == (2, 2) and \
        co.dilation == (2, 2)
    assert not co.weight.any() and not co.bias.any()
    # unsupported configurations construct, and refuse in forward
    x = torch.zeros(1, 64, 8, 8, dtype=BF16).contiguous(memory_format=torch.channels_last)
    for kw in (dict(kernel_size=5, padding=2), dict(kernel_size=3, padding=1, groups=2),
               dict(kernel_size=3, padding=0), dict(kernel_size=3, padding=1, stride=3),
               dict(kernel_size=3, padding=1, deformable_groups=16)):
        m = tda.DeformConvPack(64, 64, **kw)
        with pytest.raises(NotImplementedError):
            m(x)


def test_every_bad_argument_is_a_value_error_before_any_launch():
    import torch_detection_amd as tda
    cl = torch.channels_last
    x = torch.zeros(2, 64, 13, 19, dtype=BF16).contiguous(memory_format=cl)
    w = torch.zeros(64, 64, 3, 3)
    off = torch.zeros(2, 13, 19, 18).permute(0, 3, 1, 2)
    msk = torch.zeros(2, 13, 19, 9).permute(0, 3, 1, 2)

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            tda.deform_conv2d(*args, **kw)

    refused("CUDA", x, off, w)                                                  # everything fine but the device
    refused("CUDA", x, off, w, mask=msk)
    refused("bfloat16 / float16", x.float(), off, w)                            # fp32 x
    refused("channels_last", torch.zeros(2, 64, 13, 19, dtype=BF16), off, w)    # NCHW memory
    refused("kernel_size", x, off, torch.zeros(64, 64, 5, 5), padding=2, dilation=2)
    refused("kernel_size", x, off, torch.zeros(64, 64, 1, 1))
    refused("padding must equal dilation", x, off, w, padding=2, dilation=1)
    refused("padding must equal dilation", x, off, w, padding=0)
    refused("stride", x, off, w, stride=3)
    refused("multiple of 64", torch.zeros(2, 48, 13, 19, dtype=BF16).contiguous(memory_format=cl), off,
            torch.zeros(64, 48, 3, 3))
    refused("Cout", x, off, torch.zeros(40, 64, 3, 3))
    refused("deformable_groups", x, torch.zeros(2, 13, 19, 54).permute(0, 3, 1, 2), w, deformable_groups=3)
    refused("deformable_groups", x, torch.zeros(2, 13, 19, 288).permute(0, 3, 1, 2), w, deformable_groups=16)
    refused("weight", x, off, torch.zeros(64, 128, 3, 3))                       # channels of x and weight differ
    refused("offset", x, torch.zeros(2, 13, 19, 36).permute(0, 3, 1, 2), w)     # 36 channels for dg = 1
    refused("offset", x, torch.zeros(2, 7, 10, 18).permute(0, 3, 1, 2), w)      # the stride-2 size at stride 1
    refused("offset", x, torch.zeros(2, 18, 13, 19), w)                         # NCHW memory
    refused("offset", x, off.double(), w)
    refused("offset", x, off.half(), w)                                         # 16-bit, but not the compute dtype
    refused("mask", x, off, w, mask=torch.zeros(2, 13, 19, 18).permute(0, 3, 1, 2))
    refused("bias", x, off, w, bias=torch.zeros(32))
    # a pitched view of a wider buffer is accepted as far as the layout goes (the device is what is refused)
    wide = torch.zeros(2, 13, 19, 64, dtype=BF16).permute(0, 3, 1, 2)
    refused("CUDA", x, wide[:, :18], w, mask=wide[:, 18:27])


def test_workspace_bytes_are_the_documented_layout():
    from torch_detection_amd import deform_ops

    def want(N, H, W, stride, pad, dg):
        Ho, Wo = R.out_size(H, stride, pad), R.out_size(W, stride, pad)
        chunks = -(-Ho * Wo * dg * 9 // 256)
        up = lambda b: -(-b // 256) * 256
        return up(N * chunks * 256 * 16) + up(N * chunks * 16)

    for args in ((2, 13, 19, 1, 1, 1), (2, 13, 19, 2, 1, 4), (2, 26, 37, 2, 2, 2), (1, 9, 11, 1, 1, 1),
                 (2, 100, 168, 1, 1, 1), (3, 1, 1, 1, 1, 1)):
        assert deform_ops.deform_workspace_bytes(*args) == want(*args), args
    assert want(2, 13, 19, 1, 1, 1) == 74240
    for bad in ((2, 13, 19, 3, 1, 1), (2, 13, 19, 1, 0, 1), (0, 13, 19, 1, 1, 1), (2, 40000, 19, 1, 1, 1)):
        with pytest.raises(ValueError):
            deform_ops.deform_workspace_bytes(*bad)
