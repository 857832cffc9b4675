"""CPU: the CARAFE oracle (tests/carafe_ref.py) against float64 autograd of the plain F.unfold / F.pixel_shuffle / softmax
composition, the case list, and everything ``carafe_ops``, ``CARAFEPack`` and ``FPN_CARAFE`` refuse or build without a
device."""
import inspect

import numpy as np
import pytest
import torch

import carafe_cases as CC
import carafe_ref as R

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SMALL = [c for c in CC.CASES if c.H * c.W <= 63]


def t64(a, grad=False):
    t = torch.from_numpy(np.asarray(a, dtype=np.float64))
    return t.requires_grad_() if grad else t


def test_case_list_covers_what_it_claims():
    cs = CC.CASES
    assert 20 <= len(cs) <= 40 and len({c.id for c in cs}) == len(cs)
    assert {(c.H, c.W) for c in cs if (c.k, c.s) == (5, 2)} == set(CC.SIZES)
    for k, s in CC.KS[1:]:
        assert {(c.H, c.W) for c in cs if (c.k, c.s) == (k, s)} == {(2, 3), (13, 17)}
    assert {(c.C, c.g) for c in cs} == set(CC.CHANNELS)
    assert all(c.N == 2 for c in cs if (c.H, c.W) == (7, 9))
    assert {c.dtype for c in cs} == {BF16, F16} and {c.w32 for c in cs} == {True, False}
    crops = {(c.H * c.s - c.out_size[0], c.W * c.s - c.out_size[1], c.with_addend) for c in cs if c.s > 1}
    assert crops == {(a, b, w) for a, b in ((0, 0), (1, 0), (1, 1)) for w in (False, True)}
    c = CC.make(cs[0])
    l = c.logits.reshape(c.N, c.g, c.k * c.k, -1)
    assert 3.0 < l.max() <= 4.0 and -4.0 <= l.min() < -3.0
    m = c.masks.reshape(c.N, c.g, c.k * c.k, -1)
    assert 0.05 < m.max(axis=2).mean() < 0.9                       # neither flat (1 / 25) nor one-hot


@pytest.mark.parametrize("c", SMALL, ids=repr)
def test_oracle_against_float64_autograd(c):
    CC.make(c)
    k, g, s = c.k, c.g, c.s
    # the normaliser's channel rule
    want = R.normalize_autograd(t64(c.logits), k, s).numpy()
    assert np.abs(R.normalize(c.logits, k, g, s) - want).max() < 1e-14
    # forward: from masks and from logits
    for kw, m in ((dict(masks=c.masks), t64(c.masks)), (dict(logits=c.logits), R.normalize_autograd(t64(c.logits), k, s))):
        ref = R.carafe_autograd(t64(c.x), m, k, g, s, c.out_size, None if c.addend is None else t64(c.addend)).numpy()
        f = R.Forward64(c.x, k, g, s, out_size=c.out_size, addend=c.addend, **kw)
        assert f.v.shape == ref.shape and np.abs(f.v - ref).max() < 1e-12
        assert (f.S >= np.abs(f.v) - 1e-12).all()
    # the float32 evaluation lies within its own bound of the exact value
    got = R.forward(c.x, c.masks, k, g, s, c.dtype, c.out_size, c.addend).astype(np.float64)
    f = R.Forward64(c.x, k, g, s, masks=c.masks, out_size=c.out_size, addend=c.addend)
    assert (np.abs(got - f.v) <= R.allowance(f.v, f.S, f.T, c.dtype)).all()
    # gradients
    x, m, l = t64(c.x, True), t64(c.masks, True), t64(c.logits, True)
    R.carafe_autograd(x, m, k, g, s, c.out_size).backward(t64(c.gout))
    G = R.Grads(c.x, c.gout, k, g, s, masks=c.masks)
    assert np.abs(G.dx - x.grad.numpy()).max() < 1e-11 and np.abs(G.dmasks - m.grad.numpy()).max() < 1e-11
    assert (G.S_dx >= np.abs(G.dx) - 1e-11).all() and (G.S_dmasks >= np.abs(G.dmasks) - 1e-11).all()
    x.grad = None
    R.carafe_autograd(x, R.normalize_autograd(l, k, s), k, g, s, c.out_size).backward(t64(c.gout))
    G = R.Grads(c.x, c.gout, k, g, s, logits=c.logits)
    assert np.abs(G.dx - x.grad.numpy()).max() < 1e-11 and np.abs(G.dlogits - l.grad.numpy()).max() < 1e-11
    assert (G.S_dlogits >= np.abs(G.dlogits) - 1e-11).all()
    assert G.T_dlogits > G.T_dmasks and G.T_dx > k * k * s * s


def test_forward_is_reproducible_and_skips_taps_outside():
    c = CC.custom(1, 64, 1, (2, 3), 5, 2, BF16, seed=3)
    a = R.forward(c.x, c.masks, 5, 1, 2, BF16)
    assert np.array_equal(R.bits16(a, BF16), R.bits16(R.forward(c.x, c.masks, 5, 1, 2, BF16), BF16))
    # an infinite weight on a tap outside the map does not reach the output: the tap is skipped, not multiplied by zero
    m = c.masks.copy()
    m[:, 0] = np.inf                                  # tap (0, 0): source (h - 2, w - 2), outside a 2 x 3 map everywhere
    assert np.array_equal(R.bits16(R.forward(c.x, m, 5, 1, 2, BF16), BF16), R.bits16(a, BF16))
    # one-hot centre masks: nearest upsampling
    m = np.zeros_like(c.masks)
    m[:, 12] = 1.0
    assert np.array_equal(R.forward(c.x, m, 5, 1, 2, BF16), c.x.repeat(2, axis=2).repeat(2, axis=3))


def test_allowance_counts():
    c = CC.custom(1, 64, 1, (2, 3), 3, 2, BF16, seed=4)
    ops = R.softmax_ops(c.logits, 3, 1, 2)
    assert 9 + 2 * R.EXP_OPS + 1 < ops <= 9 + 2 * R.EXP_OPS + 1 + 8          # D <= 8 for logits in [-4, 4]
    f = R.Forward64(c.x, 3, 1, 2, logits=c.logits, addend=np.zeros((1, 64, 4, 6)))
    assert f.T == 9 + 1 + ops + 1
    G = R.Grads(c.x, c.gout, 3, 1, 2, logits=c.logits)
    assert (G.T_dx, G.T_dmasks, G.T_dlogits) == (36 + 1 + ops, 65, 64 + 9 + 4 + ops)
    a = R.allowance(np.array([1.0, 0.0]), np.array([1.0, 0.0]), 10, BF16)
    assert a[0] == 10 * 2.0 ** -23 + 2.0 ** -8 and a[1] == 2.0 ** -134


# ---- refusals, without a device ----------------------------------------------------------------------------------------
def _cl(shape, dtype=BF16):
    N, C, H, W = shape
    return torch.zeros((N, H, W, C), dtype=dtype).permute(0, 3, 1, 2)


def test_ops_refuse_bad_arguments_before_any_launch():
    from torch_detection_amd import carafe_ops as D
    x, lg, mk = _cl((1, 64, 4, 5)), _cl((1, 100, 4, 5)), _cl((1, 25, 8, 10), F32)
    fwd = lambda **kw: D.carafe_forward(kw.pop("x", x), kw.pop("k", 5), kw.pop("g", 1), kw.pop("s", 2), **kw)
    bad = [
        ("x", dict(x=torch.zeros(1, 64, 4, 5, dtype=BF16), logits=lg)),              # not channels_last
        ("x", dict(x=_cl((1, 64, 4, 5), F32), logits=lg)),
        ("C", dict(x=_cl((1, 96, 4, 5)), logits=lg)),
        ("kernel_size", dict(k=4, logits=lg)),
        ("kernel_size", dict(k=9, logits=lg)),
        ("scale_factor", dict(s=5, logits=lg)),
        ("group_size", dict(g=3, logits=lg)),
        ("group_size", dict(g=16, logits=lg)),                                          # 4 channels per group
        ("group_size * kernel_size", dict(k=7, g=8, logits=lg)),
        ("exactly one", dict()),
        ("exactly one", dict(logits=lg, masks=mk)),
        ("logits", dict(logits=_cl((1, 99, 4, 5)))),
        ("logits", dict(logits=torch.zeros(1, 100, 4, 5, dtype=BF16))),                 # NCHW memory
        ("logits", dict(logits=_cl((1, 100, 4, 5), F16))),                              # neither float32 nor x's dtype
        ("masks", dict(masks=_cl((1, 25, 8, 9), F32))),
        ("out_size[0]", dict(logits=lg, out_size=(6, 10))),
        ("out_size[1]", dict(logits=lg, out_size=(8, 11))),
        ("out_size", dict(logits=lg, out_size=8)),
        ("addend", dict(logits=lg, out_size=(7, 10), addend=_cl((1, 64, 8, 10)))),
        ("addend", dict(logits=lg, addend=_cl((1, 64, 8, 10), F16))),
        ("CUDA", dict(logits=lg)),                                                      # everything else is fine: the device, last
        ("CUDA", dict(masks=mk, out_size=(7, 9), addend=_cl((1, 64, 7, 9)))),
    ]
    for word, kw in bad:
        with pytest.raises(ValueError) as e:
            fwd(**kw)
        assert word in str(e.value), (word, str(e.value))
    g = _cl((1, 64, 7, 10))
    for word, call in [
        ("in_shape", lambda: D.carafe_feature_grad(g, (64, 4, 5), 5, 1, 2, logits=lg)),
        ("gout", lambda: D.carafe_feature_grad(_cl((1, 128, 7, 10)), (1, 64, 4, 5), 5, 1, 2, logits=lg)),
        ("out_size[0]", lambda: D.carafe_feature_grad(_cl((1, 64, 6, 10)), (1, 64, 4, 5), 5, 1, 2, logits=lg)),
        ("CUDA", lambda: D.carafe_feature_grad(g, (1, 64, 4, 5), 5, 1, 2, logits=lg)),
        ("gout", lambda: D.carafe_mask_grad(_cl((1, 64, 7, 10), F16), x, 5, 1, 2, logits=lg)),
        ("out must", lambda: D.carafe_mask_grad(g, x, 5, 1, 2, logits=lg, out=_cl((1, 128, 4, 5))[:, :100])),
        ("CUDA", lambda: D.carafe_mask_grad(g, x, 5, 1, 2, masks=mk)),
    ]:
        with pytest.raises(ValueError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))
    # a channel slice of a wider buffer is read through the pitch: accepted up to the device check
    wide = _cl((1, 128, 4, 5))
    with pytest.raises(ValueError, match="CUDA"):
        fwd(logits=wide[:, :100])
    q = D.geometry(2, 128, 7, 9, 5, 2, 2, (13, 18))
    assert (q.sH, q.sW, q.Ho, q.Wo, q.channels(True), q.channels(False)) == (14, 18, 13, 18, 200, 50)
    with pytest.raises(ValueError, match="N\\*sH\\*sW"):
        D.geometry(1, 64, 32766, 32766, 5, 1, 2)


def test_carafe_pack_constructor_state_dict_and_init():
    import torch_detection_amd as T
    sig = inspect.signature(T.CARAFEPack.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[3:]] == [
        ("up_kernel", 5), ("up_group", 1), ("encoder_kernel", 3), ("encoder_dilation", 1), ("compressed_channels", 64)]
    torch.manual_seed(0)
    m = T.CARAFEPack(256, 2)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        "channel_compressor.weight": (64, 256, 1, 1), "channel_compressor.bias": (64,),
        "content_encoder.weight": (100, 64, 3, 3), "content_encoder.bias": (100,)}
    assert tuple(T.CARAFEPack(128, 3, up_kernel=3, up_group=2, compressed_channels=128).content_encoder.weight.shape) == \
        (3 * 3 * 2 * 9, 128, 3, 3)
    # init_weights: xavier-uniform compressor (bound sqrt(6 / (256 + 64))), encoder N(0, 0.001), biases 0
    w = m.channel_compressor.weight.detach()
    bound = (6.0 / (256 + 64)) ** 0.5
    assert float(w.abs().max()) <= bound and abs(float(w.std()) - bound / 3 ** 0.5) < 0.05 * bound
    e = m.content_encoder.weight.detach()
    assert abs(float(e.std()) - 1e-3) < 5e-5 and abs(float(e.mean())) < 2e-5
    assert not m.channel_compressor.bias.any() and not m.content_encoder.bias.any()
    for kw, err in [(dict(encoder_kernel=5), NotImplementedError), (dict(encoder_dilation=2), NotImplementedError),
                    (dict(compressed_channels=48), ValueError), (dict(compressed_channels=96), ValueError),
                    (dict(up_kernel=4), ValueError), (dict(up_group=3), ValueError)]:
        with pytest.raises(err):
            T.CARAFEPack(256, 2, **kw)
    with pytest.raises(ValueError):
        T.CARAFEPack(100, 2)
    with pytest.raises(ValueError):
        T.CARAFEPack(256, 5)
    x = _cl((1, 256, 4, 5))
    for call in (lambda: m(_cl((1, 128, 4, 5))), lambda: m(x.float()), lambda: m(x, out_size=(6, 10)),
                 lambda: m(x, addend=_cl((1, 256, 8, 9)))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError, match="HIP path only"):
        m(x)
    with pytest.raises(ValueError):
        T.carafe(x, torch.zeros(1, 25, 8, 10), 4, 1, 2)
    with pytest.raises(ValueError, match="CUDA"):
        T.carafe(x, torch.zeros(1, 25, 8, 10), 5, 1, 2)


def test_fpn_carafe_registry_keys_refusals_and_mmdetection_state_dict():
    import torch_detection_amd as T
    assert T.NECKS.module_dict["FPN_CARAFE"] is T.FPN_CARAFE
    sig = inspect.signature(T.FPN_CARAFE.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[4:]] == [
        ("start_level", 0), ("end_level", -1), ("norm_cfg", None), ("activation", None), ("order", ("conv", "norm", "act")),
        ("upsample_cfg", dict(type="carafe", up_kernel=5, up_group=1, encoder_kernel=3, encoder_dilation=1))]
    n = T.NECKS.build(dict(type="FPN_CARAFE", in_channels=[64, 128, 256], out_channels=64, num_outs=5))
    shapes = {k: tuple(v.shape) for k, v in n.state_dict().items()}
    want = {}
    for i, cin in enumerate((64, 128, 256)):
        want["lateral_convs.%d.conv.weight" % i] = (64, cin, 1, 1)
    want["lateral_convs.3.conv.weight"] = (64, 256, 3, 3)
    want["lateral_convs.4.conv.weight"] = (64, 64, 3, 3)
    for i in range(5):
        want["lateral_convs.%d.conv.bias" % i] = (64,)
        want["fpn_convs.%d.conv.weight" % i] = (64, 64, 3, 3)
        want["fpn_convs.%d.conv.bias" % i] = (64,)
    for i in range(4):
        want["upsample_modules.%d.channel_compressor.weight" % i] = (64, 64, 1, 1)
        want["upsample_modules.%d.channel_compressor.bias" % i] = (64,)
        want["upsample_modules.%d.content_encoder.weight" % i] = (100, 64, 3, 3)
        want["upsample_modules.%d.content_encoder.bias" % i] = (100,)
    assert shapes == want
    assert n.lateral_convs[3].conv.stride == (2, 2) and n.lateral_convs[3].conv.padding == (1, 1)
    three = T.FPN_CARAFE([64, 128, 256], 64, 3)
    assert len(three.lateral_convs) == 3 and len(three.upsample_modules) == 2
    part = T.FPN_CARAFE([64, 128, 256, 512], 64, 2, start_level=1, end_level=3)
    assert [m.conv.in_channels for m in part.lateral_convs] == [128, 256] and len(part.upsample_modules) == 1
    up = T.FPN_CARAFE([64, 128], 64, 2, upsample_cfg=dict(type="carafe", up_kernel=3, up_group=2, encoder_kernel=3,
                                                        encoder_dilation=1, compressed_channels=128))
    assert tuple(up.upsample_modules[0].content_encoder.weight.shape) == (72, 128, 3, 3)
    for kw in (dict(norm_cfg=dict(type="BN")), dict(activation="relu"), dict(order=("act", "conv", "norm")),
               dict(upsample_cfg=dict(type="nearest")), dict(upsample_cfg=dict(type="deconv")),
               dict(upsample_cfg=dict(type="carafe", encoder_kernel=5)),
               dict(upsample_cfg=dict(type="carafe", encoder_dilation=2))):
        with pytest.raises(NotImplementedError):
            T.FPN_CARAFE([64, 128, 256], 64, 3, **kw)
    for args, kw in ((([64, 128, 256], 64, 2), {}), (([64, 128], 64, 2), dict(end_level=3)),
                     (([64, 128], 64, 2), dict(upsample_cfg=dict(type="carafe", up_kernal=5))), ((64, 64, 1), {})):
        with pytest.raises(ValueError):
            T.FPN_CARAFE(*args, **kw)
    # init_weights: xavier everywhere, then the encoders' N(0, 0.001)
    torch.manual_seed(1)
    n.init_weights()
    assert abs(float(n.upsample_modules[2].content_encoder.weight.detach().std()) - 1e-3) < 5e-5
    assert float(n.fpn_convs[0].conv.weight.detach().abs().max()) <= (6.0 / (64 * 9 * 2)) ** 0.5
    # a state dict written under mmdetection's key names loads and round-trips
    g = torch.Generator().manual_seed(2)
    sd = {k: torch.randn(s, generator=g) for k, s in want.items()}
    other = T.FPN_CARAFE([64, 128, 256], 64, 5)
    missing, unexpected = other.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    back = other.state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    assert other.upsample_modules[0].content_encoder.weight.permute(0, 2, 3, 1).is_contiguous()
    with pytest.raises(ValueError, match="expected 3 inputs"):
        other([torch.zeros(1)])
