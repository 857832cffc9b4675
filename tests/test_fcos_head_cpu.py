"""CPU: ``FCOSHead`` as a module — registry, parameter names and shapes, initialisation, mmdetection's
``.gn.`` state-dict keys, the refusals that need no GPU."""
import math
import types

import pytest
import torch

INF = 1e8


def _T():
    import torch_detection_amd as T
    return T


def _expected(num_classes, Cin, C, stacked, gn, levels=5):
    want = []
    for tower in ("cls_convs", "reg_convs"):
        for i in range(stacked):
            want.append(("%s.%d.conv.weight" % (tower, i), (C, Cin if i == 0 else C, 3, 3)))
            if gn:
                want += [("%s.%d.norm.weight" % (tower, i), (C,)), ("%s.%d.norm.bias" % (tower, i), (C,))]
            else:
                want.append(("%s.%d.conv.bias" % (tower, i), (C,)))
    last = C if stacked else Cin
    want += [("fcos_cls.weight", (num_classes - 1, last, 3, 3)), ("fcos_cls.bias", (num_classes - 1,)),
             ("fcos_reg.weight", (4, last, 3, 3)), ("fcos_reg.bias", (4,)),
             ("fcos_centerness.weight", (1, last, 3, 3)), ("fcos_centerness.bias", (1,))]
    want += [("scales.%d.scale" % l, ()) for l in range(levels)]
    return want


def test_registry_builds_the_head_from_a_config_dict():
    T = _T()
    from torch_detection_amd.registry import HEADS
    cfg = dict(type="FCOSHead", num_classes=81, in_channels=256)
    head = HEADS.build(cfg)
    assert type(head) is T.FCOSHead
    assert head.feat_channels == 256 and head.stacked_convs == 4 and head.strides == [8, 16, 32, 64, 128]
    assert head.regress_ranges == [(-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)]
    assert head.norm_cfg == dict(type="GN", num_groups=32, requires_grad=True)
    assert head.cls_out_channels == 80 and len(head.scales) == 5
    assert all(m.norm.num_groups == 32 and m.conv.bias is None for m in list(head.cls_convs) + list(head.reg_convs))


@pytest.mark.parametrize("gn", [True, False], ids=["GN", "no-norm"])
def test_parameter_names_and_shapes(gn):
    T = _T()
    head = T.FCOSHead(4, 128, feat_channels=64, stacked_convs=2, strides=(8, 16, 32),
                      regress_ranges=((-1, 64), (64, 128), (128, INF)),
                      norm_cfg=dict(type="GN", num_groups=16, requires_grad=True) if gn else None)
    got = [(n, tuple(p.shape)) for n, p in head.named_parameters()]
    assert got == _expected(4, 128, 64, 2, gn, 3)
    assert [k for k in head.state_dict()] == [n for n, _ in got]
    if gn:
        assert head.cls_convs[1].norm.num_groups == 16 and head.cls_convs[0].conv.bias is None
    # what the autograd node is handed: every parameter but the scales, once
    handed = head._params()
    assert len(handed) == len(got) - 3 and len(set(map(id, handed))) == len(handed)
    assert all(any(p is q for q in head.parameters()) for p in handed)
    # 3x3 weights live in channels_last memory
    assert head.fcos_reg.weight.permute(0, 2, 3, 1).is_contiguous()
    assert head.cls_convs[0].conv.weight.permute(0, 2, 3, 1).is_contiguous()
    assert float(head.scales[0].scale.detach()) == 1.0 and head.scales[0].scale.dtype == torch.float32
    assert tuple(head.scale_vector().shape) == (3,) and head.scale_vector().requires_grad


def test_frozen_affine_is_marked_on_the_parameters():
    T = _T()
    head = T.FCOSHead(4, 64, 64, 1, norm_cfg=dict(type="GN", num_groups=32, requires_grad=False))
    for m in list(head.cls_convs) + list(head.reg_convs):
        assert not m.norm.weight.requires_grad and not m.norm.bias.requires_grad and m.conv.weight.requires_grad


def test_init_weights_gives_the_prior_probability_bias():
    T = _T()
    torch.manual_seed(0)
    head = T.FCOSHead(81, 256)
    assert torch.allclose(head.fcos_cls.bias, torch.full((80,), -math.log(99.0)))
    assert (head.fcos_reg.bias == 0).all() and (head.fcos_centerness.bias == 0).all()
    w = head.cls_convs[0].conv.weight.detach()
    assert abs(float(w.std()) - 0.01) < 1e-3 and abs(float(w.mean())) < 1e-3
    assert abs(float(head.fcos_cls.weight.detach().std()) - 0.01) < 1e-3
    assert (head.cls_convs[0].norm.weight == 1).all() and (head.cls_convs[0].norm.bias == 0).all()


def test_state_dict_with_mmdetection_gn_keys_loads():
    T = _T()
    torch.manual_seed(1)
    src = T.FCOSHead(4, 64, 64, 2)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(torch.randn_like(p))
    sd = {k.replace(".norm.", ".gn."): v.clone() for k, v in src.state_dict().items()}
    assert "cls_convs.1.gn.weight" in sd and not any(".norm." in k for k in sd)
    dst = T.FCOSHead(4, 64, 64, 2)
    res = dst.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    for (k, a), (_, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert torch.equal(a, b), k
    # its own spelling still loads, and under a prefix too
    dst.load_state_dict(src.state_dict())
    holder = torch.nn.Module()
    holder.bbox_head = T.FCOSHead(4, 64, 64, 2)
    holder.load_state_dict({"bbox_head." + k: v for k, v in sd.items()})
    assert torch.equal(holder.bbox_head.reg_convs[1].norm.bias, src.reg_convs[1].norm.bias)


def test_forward_on_cpu_tensors_names_the_missing_fallback():
    T = _T()
    head = T.FCOSHead(4, 64, 64, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head([torch.zeros(2, 64, 4, 4)])


def _refusal(head, text, feats=None):
    with pytest.raises(NotImplementedError, match=text):
        if feats is None:
            head._check_supported()
        else:
            head(feats)


def test_check_supported_names_each_limit():
    T = _T()
    _refusal(T.FCOSHead(4, 64, 64, 2, conv_cfg=dict(type="DCN")), "conv_cfg")
    _refusal(T.FCOSHead(4, 64, 64, 2, norm_cfg=dict(type="BN")), "norm type 'BN'")
    _refusal(T.FCOSHead(4, 96, 64, 2), "in_channels=96 must be a multiple of 64")
    _refusal(T.FCOSHead(4, 64, 1024, 2), "feat_channels=1024 must be a multiple of 64, at most 512")
    _refusal(T.FCOSHead(4, 64, 192, 2), r"GroupNorm\(32 groups, feat_channels=192\)")
    with pytest.raises(ValueError):                                      # nn.GroupNorm's own refusal
        T.FCOSHead(4, 64, 64, 2, norm_cfg=dict(type="GN", num_groups=48))
    _refusal(T.FCOSHead(4, 64, 512, 2, norm_cfg=dict(type="GN", num_groups=1)), "at most 256 channels per group")
    T.FCOSHead(4, 64, 192, 2, norm_cfg=None)._check_supported()          # without GroupNorm 192 channels are fine
    T.FCOSHead(4, 64, 128, 2, norm_cfg=dict(type="GN", num_groups=2))._check_supported()
    head = T.FCOSHead(4, 64, 64, 2)
    _refusal(head, "1..8 levels", [torch.zeros(1, 64, 2, 2)] * 9)
    _refusal(head, "1..8 levels", [])
    # a gradient bucket on a shared weight
    head.__dict__["_hip_units"] = {("fcos_cls.composed", torch.bfloat16): types.SimpleNamespace(sink=(None,) * 3)}
    with pytest.raises(NotImplementedError, match="gradient bucket"):
        head._chains(torch.bfloat16)


def test_constructor_refuses_inconsistent_arguments():
    T = _T()
    with pytest.raises(ValueError):
        T.FCOSHead(1, 64)
    with pytest.raises(ValueError):
        T.FCOSHead(4, 64, strides=(8, 16), regress_ranges=((-1, 64),))


def test_retina_head_keeps_its_norm_cfg_refusal():
    T = _T()
    with pytest.raises(NotImplementedError, match="norm_cfg"):
        T.RetinaHead(4, 64, norm_cfg=dict(type="GN", num_groups=32))._check_supported()
