"""CPU: the oracle of the dense head predictors (tests/dense_head_ref.py) pinned to torch's float64 autograd of the RPN
head it stands for; the host side of csrc/dense_head.hip — refusals of ``dense_ops`` that need no device, the plan, the
level-table struct — and ``RPNHead``'s parameters, state dict and unsupported configurations."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dense_head_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16 = torch.bfloat16, torch.float16
CL = torch.channels_last


def test_oracle_is_float64_autograd_of_conv_relu_and_two_1x1_predictors():
    """Three levels: h = relu(conv3x3(x)), cls = conv1x1(h), reg = conv1x1(h) in float64; the oracle's forward,
    masked input gradient and weight gradients are autograd's (the mask through the ReLU that made h)."""
    g = torch.Generator().manual_seed(1)
    B, C, A = 2, 64, 3
    sizes = [(6, 5), (3, 3), (1, 2)]
    w3 = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64) / 24
    b3 = torch.randn(C, generator=g, dtype=torch.float64)
    wc = torch.randn(A, C, generator=g, dtype=torch.float64).requires_grad_(True)
    wr = torch.randn(4 * A, C, generator=g, dtype=torch.float64).requires_grad_(True)
    bc = torch.randn(A, generator=g, dtype=torch.float64).requires_grad_(True)
    br = torch.randn(4 * A, generator=g, dtype=torch.float64).requires_grad_(True)
    xs = [torch.randn(B, C, h, w, generator=g, dtype=torch.float64) for h, w in sizes]
    zs = [F.conv2d(x, w3, b3, padding=1).requires_grad_(True) for x in xs]       # pre-activations: leaves
    hs = [z.relu() for z in zs]
    cls = [F.conv2d(h, wc.view(A, C, 1, 1), bc) for h in hs]
    reg = [F.conv2d(h, wr.view(4 * A, C, 1, 1), br) for h in hs]
    gc = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in cls]
    gr = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in reg]
    torch.autograd.backward(cls + reg, gc + gr)
    nhwc = lambda ts: [t.detach().permute(0, 2, 3, 1).contiguous() for t in ts]
    hn, gcn, grn = nhwc(hs), nhwc(gc), nhwc(gr)
    assert any((h == 0).any() for h in hn) and all((h > 0).any() for h in hn)
    oc, orr = R.fwd(hn, wc.detach(), bc.detach(), wr.detach(), br.detach())
    for a, b in zip(oc + orr, nhwc(cls) + nhwc(reg)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    for a, z in zip(R.dgrad(gcn, grn, wc.detach(), wr.detach(), hn), zs):
        torch.testing.assert_close(a, z.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    dwc, dbc, dwr, dbr = R.wgrad(hn, gcn, grn)
    for a, b in zip((dwc, dbc, dwr, dbr), (wc.grad, bc.grad, wr.grad, br.grad)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-11)
    # the bounds are the linear layer's on the concatenated rows, shaped for the stacked results
    M = sum(B * h * w for h, w in sizes)
    f32 = lambda ts: [t.float() for t in ts]
    assert tuple(R.fwd_bound(f32(hn), wc.detach().float(), bc.detach().float(), wr.detach().float(),
                             br.detach().float()).v.shape) == (M, 5 * A, 1, 1)
    assert tuple(R.dgrad_bound(f32(gcn), f32(grn), wc.detach().float(), wr.detach().float(), f32(hn)).v.shape) == (M, C, 1, 1)
    assert tuple(R.wgrad_bound(f32(hn), f32(gcn), f32(grn)).v.shape) == (5 * A, C, 1, 1)
    assert tuple(R.dbias_bound(f32(gcn), f32(grn)).v.shape) == (5 * A, 1, 1, 1)


def _cl(B, ch, H, W, dtype=BF16):
    return torch.zeros(B, H, W, ch, dtype=dtype).permute(0, 3, 1, 2)


def test_refusals_are_value_errors_that_name_the_argument_without_a_device():
    from torch_detection_amd import dense_ops as D
    A, C = 3, 64
    hs = [_cl(2, C, 4, 4), _cl(2, C, 2, 2)]
    w_fwd = torch.zeros(16, C, dtype=BF16)
    w_dgrad = torch.zeros(C, 32, dtype=BF16)
    bc, br = torch.zeros(A), torch.zeros(4 * A)
    gc = [_cl(2, A, 4, 4), _cl(2, A, 2, 2)]
    gr = [_cl(2, 4 * A, 4, 4), _cl(2, 4 * A, 2, 2)]

    def refuses(fn, word):
        with pytest.raises(ValueError) as e:
            fn()
        assert word in str(e.value), str(e.value)

    # wrong dtype
    refuses(lambda: D.pred_fwd([hs[0].float(), hs[1]], w_fwd, bc, br), "hs[0]")
    refuses(lambda: D.pred_fwd([hs[0], hs[1].to(F16)], w_fwd, bc, br), "hs[1]")
    refuses(lambda: D.pred_fwd(hs, w_fwd.to(F16), bc, br), "w_fwd")
    refuses(lambda: D.pred_fwd(hs, w_fwd, bc.double(), br), "bias_cls")
    # not channels_last
    refuses(lambda: D.pred_fwd([hs[0], torch.zeros(2, C, 2, 2, dtype=BF16)], w_fwd, bc, br), "hs[1]")
    refuses(lambda: D.pred_dgrad(gc, gr, w_dgrad, [torch.zeros(2, C, 4, 4, dtype=BF16), hs[1]]), "hs[0]")
    refuses(lambda: D.pred_wgrad([hs[0], torch.zeros(2, C, 2, 2, dtype=BF16)], gc, gr), "hs[1]")
    # C = 96, A = 13
    refuses(lambda: D.pred_fwd([_cl(2, 96, 4, 4)], torch.zeros(16, 96, dtype=BF16), bc, br), "C ")
    refuses(lambda: D.pred_fwd(hs, torch.zeros(80, C, dtype=BF16), torch.zeros(13), torch.zeros(52)), "A ")
    refuses(lambda: D.pack_pred_weight(torch.zeros(13, C), torch.zeros(52, C)), "A ")
    refuses(lambda: D.pack_pred_weight(torch.zeros(A, 96), torch.zeros(4 * A, 96)), "C ")
    refuses(lambda: D.pack_pred_weight(torch.zeros(A, C), torch.zeros(4 * A + 1, C)), "w_reg")
    # nine levels, none
    refuses(lambda: D.pred_fwd([hs[1]] * 9, w_fwd, bc, br), "hs")
    refuses(lambda: D.pred_fwd([], w_fwd, bc, br), "hs")
    refuses(lambda: D.pred_wgrad(hs, gc + gc, gr), "g_cls")
    # mismatched B, mismatched shapes
    refuses(lambda: D.pred_fwd([hs[0], _cl(3, C, 2, 2)], w_fwd, bc, br), "hs[1]")
    refuses(lambda: D.pred_dgrad([gc[0], _cl(3, A, 2, 2)], gr, w_dgrad, hs), "g_cls[1]")
    refuses(lambda: D.pred_wgrad(hs, gc, [gr[0], _cl(2, 4 * A, 2, 3)]), "g_reg[1]")
    refuses(lambda: D.pred_dgrad(gc, gr, torch.zeros(C, 64, dtype=BF16), hs), "w_dgrad")
    # everything right but the device: refused last
    refuses(lambda: D.pred_fwd(hs, w_fwd, bc, br), "CUDA")
    refuses(lambda: D.pred_dgrad(gc, gr, w_dgrad, hs), "CUDA")
    refuses(lambda: D.pred_wgrad(hs, gc, gr), "CUDA")
    refuses(lambda: D.pack_pred_weight(torch.zeros(A, C, 1, 1), torch.zeros(4 * A, C, 1, 1)), "CUDA")


def test_plan_rows_workgroups_slices_and_library_refusals():
    from torch_detection_amd import _lib
    from torch_detection_amd import dense_ops as D
    rows = [2 * 200 * 336, 2 * 100 * 168, 2 * 50 * 84, 2 * 25 * 42, 2 * 13 * 21]
    f = D.pred_plan(D.FWD, rows, 256, 3)
    RT = f.rows_per_workgroup
    assert RT == 128 and f.workgroups == sum(-(-r // RT) for r in rows) and f.launches == 1
    assert (f.Op, f.Kp) == (16, 32) and f.workspace_bytes == 0 and f.lds_bytes == 16 * 256 * 2
    d = D.pred_plan(D.DGRAD, rows, 256, 3)
    assert d.workgroups == f.workgroups and d.launches == 1 and d.workspace_bytes == 0 and d.lds_bytes == 256 * 32 * 2
    w = D.pred_plan(D.WGRAD, rows, 256, 3)
    # the slice rule: ceil(total / 64) rounded up to whole 128-row steps, each level cut on its own
    sr = -(-(-(-sum(rows) // 64)) // RT) * RT
    assert w.rows_per_slice == sr and w.slices == sum(-(-r // sr) for r in rows)
    assert w.channel_tiles == 4 and w.workgroups == w.slices * 4 and w.launches == 2
    assert w.slab_bytes == w.slices * 16 * 256 * 4
    assert w.workspace_bytes == w.slab_bytes + -(-w.slices * 16 * 4 // 256) * 256 and w.workspace_bytes % 256 == 0
    # P2 at batch 4 exceeds the linear kernels' 2^18 rows; the row count is 64-bit
    big = D.pred_plan(D.FWD, [4 * 200 * 336], 256, 3)
    assert big.workgroups == 2100
    assert D.pred_plan(D.FWD, [(1 << 31) - 1], 64, 1).workgroups == 1 << 24
    # O = 5, 15, 20, 45, 60 cross every 16-column block and the 32-column reduction step
    assert [(D.pred_plan(D.FWD, [1], 64, A).Op, D.pred_plan(D.FWD, [1], 64, A).Kp) for A in (1, 3, 4, 9, 12)] == \
        [(16, 32), (16, 32), (32, 32), (48, 64), (64, 64)]
    # an empty batch: nothing but wgrad's finalize
    for kind, launches in ((D.FWD, 0), (D.DGRAD, 0), (D.WGRAD, 1)):
        e = D.pred_plan(kind, [0, 0], 64, 3)
        assert (e.workgroups, e.slices, e.launches, e.workspace_bytes) == (0, 0, launches, 0)
    # small levels keep their own slices
    s = D.pred_plan(D.WGRAD, [144, 40, 12, 2], 64, 3)
    assert s.rows_per_slice == 128 and s.slices == 2 + 1 + 1 + 1
    # refusals come back through tdn_last_error, as ValueErrors here
    for bad in (lambda: D.pred_plan(D.FWD, [1], 96, 3), lambda: D.pred_plan(D.FWD, [1], 576, 3),
                lambda: D.pred_plan(D.FWD, [1], 64, 13), lambda: D.pred_plan(D.FWD, [1], 64, 0),
                lambda: D.pred_plan(3, [1], 64, 3)):
        with pytest.raises(ValueError):
            bad()
    lib = _lib.load()
    out = (ctypes.c_int32 * 16)()
    nine = (ctypes.c_int64 * 9)(*([1] * 9))
    assert lib.tdn_pred_plan(0, nine, 9, 64, 3, out) != 0 and b"num_levels" in lib.tdn_last_error()
    assert lib.tdn_pred_workspace_bytes(2, nine, 8, 96, 3) == -1 and b"multiple of 64" in lib.tdn_last_error()
    assert lib.tdn_pred_fwd(None, 1, None, None, None, 64, 3, 0, None) != 0 and b"NULL" in lib.tdn_last_error()


def test_level_table_struct_matches_the_header(tmp_path):
    """sizeof / offsetof of tdn_pred_level as gcc lays it out == the ctypes mirror."""
    from torch_detection_amd import _lib
    cls = _lib.PredLevel
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(tdn_pred_level));', 'printf("levels %d\\n", TDN_PRED_MAX_LEVELS);']
    for fname, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(tdn_pred_level, %s));' % (fname, fname))
    lines.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().split("\n") if ln)
    assert int(got.pop("sizeof")) == ctypes.sizeof(cls)
    assert int(got.pop("levels")) == _lib.PRED_MAX_LEVELS
    assert {k: int(v) for k, v in got.items()} == {f: getattr(cls, f).offset for f, _ in cls._fields_}
    assert len(got) == 5


class _TorchRPNHead(nn.Module):
    """mmdetection v1's RPNHead as plain torch: the names and shapes a checkpoint carries."""

    def __init__(self, in_channels, feat_channels, A):
        super().__init__()
        self.rpn_conv = nn.Conv2d(in_channels, feat_channels, 3, padding=1)
        self.rpn_cls = nn.Conv2d(feat_channels, A, 1)
        self.rpn_reg = nn.Conv2d(feat_channels, A * 4, 1)


def test_rpn_head_parameters_are_mmdetections_and_load_its_state_dict():
    import torch_detection_amd as T
    assert T.HEADS.module_dict["RPNHead"] is T.RPNHead
    torch.manual_seed(0)
    head = T.RPNHead(128, 64, anchor_scales=(8, 16), anchor_ratios=(0.5, 1.0, 2.0), anchor_strides=(4, 8, 16))
    ref = _TorchRPNHead(128, 64, 6)
    sd, rd = head.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rd.keys()) == ["rpn_conv.weight", "rpn_conv.bias", "rpn_cls.weight", "rpn_cls.bias",
                                                  "rpn_reg.weight", "rpn_reg.bias"]
    assert all(sd[k].shape == rd[k].shape and sd[k].dtype == rd[k].dtype for k in sd)
    assert head.num_anchors == 6 and len(head.anchor_generators) == 3
    # init: normal(0, 0.01) weights, zero biases
    for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
        assert not m.bias.abs().sum().item() and 0.005 < m.weight.std().item() < 0.02
    head.load_state_dict(rd)
    assert all(torch.equal(head.state_dict()[k], rd[k]) for k in rd)
    built = T.HEADS.build(dict(type="RPNHead", in_channels=64, feat_channels=64))
    assert built.num_anchors == 3 and built.anchor_strides == [4, 8, 16, 32, 64] and built.anchor_base_sizes == [4, 8, 16, 32, 64]


@pytest.mark.parametrize("kw", [dict(use_sigmoid_cls=False), dict(anchor_scales=(2, 4, 8, 16, 32)),
                                dict(in_channels=96), dict(feat_channels=80), dict(feat_channels=576),
                                dict(in_channels=1024)],
                         ids=["softmax", "15-anchors", "cin-96", "feat-80", "feat-576", "cin-1024"])
def test_unsupported_configurations_construct_and_raise_only_in_forward(kw):
    import torch_detection_amd as T
    args = dict(in_channels=64, feat_channels=64)
    args.update(kw)
    head = T.RPNHead(**args)                               # constructs, with mmdetection's shapes
    assert head.rpn_reg.weight.shape[0] == 4 * head.num_anchors
    assert head.rpn_cls.weight.shape[0] == head.num_anchors * (1 if head.use_sigmoid_cls else 2)
    with pytest.raises(NotImplementedError):
        head([torch.zeros(1, args["in_channels"], 4, 4)])
