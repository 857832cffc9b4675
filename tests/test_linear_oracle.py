"""CPU: the oracle of the fully connected layers (tests/linear_ref.py), the host-only plan of csrc/linear.hip, every
refusal of the wrappers that needs no device, and BBoxHead's parameters."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import linear_ref as R

HEAD_LAYERS = {"fc6": (1024, 12544), "fc7": (1024, 1024), "fc_cls": (81, 1024), "fc_reg": (324, 1024)}


def test_ref_with_the_permutation_is_f_linear_on_a_channels_last_input():
    g = torch.Generator().manual_seed(1)
    Rr, C, S, O = 5, 16, 3, 7
    x = torch.randn(Rr, C, S, S, generator=g, dtype=torch.float64).contiguous(memory_format=torch.channels_last)
    w = torch.randn(O, C * S * S, generator=g, dtype=torch.float64)
    b = torch.randn(O, generator=g, dtype=torch.float64)
    x_mem = x.permute(0, 2, 3, 1).reshape(Rr, -1)              # the buffer as the kernel reads it
    want = F.linear(x.reshape(Rr, -1), w, b)
    assert torch.equal(R.fwd(x_mem, w, b, C=C), want) or torch.allclose(R.fwd(x_mem, w, b, C=C), want, rtol=0, atol=1e-12)
    assert torch.equal(R.unpack_w(R.pack_w(w, C), C), w)
    # gradients: the reference's autograd on the logical tensors
    xl = x.clone().requires_grad_(True)
    wl = w.clone().requires_grad_(True)
    gy = torch.randn(Rr, O, generator=g, dtype=torch.float64)
    F.linear(xl.reshape(Rr, -1), wl, b).backward(gy)
    dx_mem = R.dgrad(gy, w, C=C)
    assert torch.allclose(dx_mem.view(Rr, S, S, C).permute(0, 3, 1, 2), xl.grad, rtol=0, atol=1e-12)
    dw, db = R.wgrad(x_mem, gy, C=C)
    assert torch.allclose(dw, wl.grad, rtol=0, atol=1e-12) and torch.allclose(db, gy.sum(0), rtol=0, atol=1e-12)


def _plan(kind, M, O, K, splits=0):
    from torch_detection_amd import linear_ops
    return linear_ops.linear_plan(kind, M, O, K, splits)


@pytest.mark.parametrize("layer", sorted(HEAD_LAYERS))
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_plan_slices_cover_the_reduction_once(layer, kind):
    O, K = HEAD_LAYERS[layer]
    M = 1024
    pl = _plan(kind, M, O, K)
    red = {0: K // 64, 1: (O + 63) // 64, 2: (M + 63) // 64}[kind]
    assert pl.chunks == red and pl.bk == 64
    # slice s owns chunks [s * cps, min((s + 1) * cps, chunks)): disjoint by construction; none is empty, all are covered
    assert pl.slices * pl.chunks_per_slice >= pl.chunks > (pl.slices - 1) * pl.chunks_per_slice
    assert pl.workgroups == pl.tiles * pl.slices
    assert pl.launches == 1 + (pl.slices > 1) + pl.pad
    assert pl.pad == (1 if kind != 0 and O % 64 else 0)
    assert (pl.slab_bytes > 0) == (pl.slices > 1) and pl.workspace_bytes >= pl.slab_bytes
    # routing: the unsplit forward / dgrad of a layer with O % 64 == 0 is handed to the conv GEMM; nothing else is
    assert pl.conv == (1 if kind != 2 and O % 64 == 0 and pl.slices == 1 else 0)
    assert _plan(kind, M, O, K, 1).conv == 0
    if layer == "fc7" and kind != 2:
        assert pl.slices == 1 and pl.conv == 1
    if layer == "fc6":
        assert (pl.slices > 1) == (kind == 0), "fc6: the forward is split, dgrad and wgrad are not"


def test_plan_forced_splits_and_empty_batch():
    pl = _plan(0, 130, 81, 448, 3)          # 7 chunks in 3 slices: 3 + 3 + 1
    assert (pl.chunks, pl.slices, pl.chunks_per_slice) == (7, 3, 3)
    assert _plan(0, 130, 81, 448, 7).slices == 7 and _plan(0, 130, 81, 448, 1).slices == 1
    assert _plan(2, 130, 81, 448, 3).slices == 3
    assert _plan(0, 0, 81, 64).launches == 0 and _plan(1, 0, 81, 64).launches == 0
    assert _plan(2, 0, 81, 64).launches == 1          # dw = beta * old still has to be written


@pytest.mark.parametrize("args, text", [((0, 128, 81, 100, 0), b"multiple of 64"), ((0, 128, 81, 448, 8), b"splits"),
                                        ((2, 130, 81, 448, 4), b"splits"), ((0, 128, 0, 448, 0), b"O=0"),
                                        ((3, 128, 81, 448, 0), b"kind")])
def test_plan_reports_bad_arguments(args, text):
    from torch_detection_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int32 * 16)()
    assert lib.tdn_linear_plan(*args, out) != 0
    assert text in lib.tdn_last_error()
    assert lib.tdn_linear_workspace_bytes(*args) < 0
    with pytest.raises(ValueError):
        _plan(*args)


def test_wrapper_refusals_need_no_device():
    import torch_detection_amd as T
    from torch_detection_amd import linear_ops as L
    bf = torch.bfloat16
    w = torch.zeros(81, 448)
    with pytest.raises(ValueError, match="x must"):
        T.linear(torch.zeros(4, 448), w)                                   # float32 activations
    with pytest.raises(ValueError, match="x must"):
        T.linear(torch.zeros(4, 896, dtype=bf)[:, ::2], w)                  # not contiguous
    with pytest.raises(ValueError, match="weight must"):
        T.linear(torch.zeros(4, 512, dtype=bf), w)                          # K mismatch
    with pytest.raises(ValueError, match="weight must"):
        T.linear(torch.zeros(4, 8, 7, 7, dtype=bf), w)                      # 4-D: C * S * S = 392 != 448
    with pytest.raises(ValueError, match="x must"):
        T.linear(torch.zeros(4, 7, 8, 8, dtype=bf).permute(0, 2, 1, 3), torch.zeros(81, 448))   # neither layout
    with pytest.raises(ValueError, match="weight must"):
        T.linear(torch.zeros(4, 448, dtype=bf), w.to(bf))                   # 16-bit parameters
    with pytest.raises(ValueError, match="bias must"):
        T.linear(torch.zeros(4, 448, dtype=bf), w, torch.zeros(80))
    # the 2-D wrappers
    x, wf, wd = torch.zeros(4, 448, dtype=bf), torch.zeros(128, 448, dtype=bf), torch.zeros(448, 128, dtype=bf)
    g = torch.zeros(4, 81, dtype=bf)
    with pytest.raises(ValueError, match="x must"):
        L.linear_fwd(x.float(), wf, 81)
    with pytest.raises(ValueError, match="w_fwd must"):
        L.linear_fwd(x, wf.half(), 81)
    with pytest.raises(ValueError, match="w_fwd must"):
        L.linear_fwd(x, wf[:81], 81)                                        # not padded to 64 rows
    with pytest.raises(ValueError, match="K must"):
        L.linear_fwd(torch.zeros(4, 100, dtype=bf), torch.zeros(128, 100, dtype=bf), 81)
    with pytest.raises(ValueError, match="splits must"):
        L.linear_fwd(x, wf, 81, splits=8)
    with pytest.raises(ValueError, match="mask_src must"):
        L.linear_dgrad(g, wd, mask_src=torch.zeros(4, 447, dtype=bf))
    with pytest.raises(ValueError, match="g must"):
        L.linear_wgrad(x, torch.zeros(5, 81, dtype=bf))
    with pytest.raises(ValueError, match="C must"):
        L.linear_wgrad(x, g, C=12)
    with pytest.raises(ValueError, match="dw must"):
        L.linear_wgrad(x, g, beta=1.0)
    with pytest.raises(ValueError, match="weight must"):
        L.pack_linear_weight(torch.zeros(81, 448, dtype=bf))
    # everything in order except the device: refused last, still without a launch
    with pytest.raises(ValueError, match="CUDA"):
        L.linear_fwd(x, wf, 81)


KEYS = {"shared_fcs.0.weight": (1024, 12544), "shared_fcs.0.bias": (1024,), "shared_fcs.1.weight": (1024, 1024),
        "shared_fcs.1.bias": (1024,), "fc_cls.weight": (81, 1024), "fc_cls.bias": (81,), "fc_reg.weight": (324, 1024),
        "fc_reg.bias": (324,)}


@pytest.fixture(scope="module")
def head():
    import torch_detection_amd as T
    torch.manual_seed(0)
    return T.BBoxHead()


def test_bbox_head_state_dict_is_mmdetections(head):
    import torch_detection_amd as T
    sd = head.state_dict()
    assert list(sd) == list(KEYS)
    assert {k: tuple(v.shape) for k, v in sd.items()} == KEYS
    other = {k: torch.full(s, float(i)) for i, (k, s) in enumerate(KEYS.items())}
    small = T.BBoxHead()
    small.load_state_dict(other)
    back = small.state_dict()
    assert list(back) == list(KEYS) and all(torch.equal(back[k], other[k]) for k in KEYS)
    assert tuple(T.BBoxHead(reg_class_agnostic=True, in_channels=8, fc_out_channels=64).fc_reg.weight.shape) == (4, 64)
    assert T.HEADS.module_dict["BBoxHead"] is T.BBoxHead


def test_bbox_head_init_weights_statistics(head):
    for fc in head.shared_fcs:
        a = math.sqrt(6.0 / (fc.in_features + fc.out_features))       # xavier uniform on (-a, a): std a / sqrt(3)
        w = fc.weight.detach()
        assert float(w.abs().max()) <= a and float(w.abs().max()) > 0.99 * a
        assert abs(float(w.std()) / (a / math.sqrt(3.0)) - 1.0) < 0.01 and abs(float(w.mean())) < 0.01 * a
    for fc, std in ((head.fc_cls, 0.01), (head.fc_reg, 0.001)):
        w = fc.weight.detach()
        assert abs(float(w.std()) / std - 1.0) < 0.02 and abs(float(w.mean())) < 0.02 * std
    assert all(float(fc.bias.detach().abs().max()) == 0.0 for fc in list(head.shared_fcs) + [head.fc_cls, head.fc_reg])
