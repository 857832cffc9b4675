"""CPU: the GHM oracle tests/ghm_ref.py against an independent torch float64 restatement written the way
mmdetection v1 writes GHMC / GHMR (per-level loop over bins, boolean masks, expanded one-hot targets,
``F.binary_cross_entropy_with_logits(weight=, reduction='sum') / tot``, ``sqrt(d^2 + mu^2) - mu``, autograd), on inputs
whose gradient norms are placed away from the edges; hand values; the boundary inputs; the struct mirror; every host
refusal by its message.

Tolerance of the float32 oracle against float64: every compared quantity is a chain of at most 12 correctly rounded
float32 operations and one soft_exp (4u), u = 2^-24: 16u relative, taken twice over = 32u."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ghm_cases as GC
import ghm_ref as R
from loss_ref import flatten_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RTOL = 32 * R.U


# ---- mmdetection's form, float64 ------------------------------------------------------------------------------------
def _weights(g, valid, bins, last_edge, momentum, acc_sum):
    edges = torch.arange(bins + 1, dtype=torch.float64) / bins
    edges[-1] = last_edge
    weights = torch.zeros_like(g)
    tot = max(float(valid.sum().item()), 1.0)
    n = 0
    for i in range(bins):
        inds = (g >= edges[i]) & (g < edges[i + 1]) & valid
        num_in_bin = inds.sum().item()
        if num_in_bin > 0:
            if momentum > 0:
                acc_sum[i] = momentum * acc_sum[i] + (1 - momentum) * num_in_bin
                weights[inds] = tot / acc_sum[i]
            else:
                weights[inds] = tot / num_in_bin
            n += 1
    if n > 0:
        weights = weights / n
    return weights, tot


def ghmc_torch(pred, target, label_weight, bins, momentum, acc_sum):
    g = torch.abs(pred.sigmoid().detach() - target)
    weights, tot = _weights(g, label_weight > 0, bins, 1 + 1e-6, momentum, acc_sum)
    return F.binary_cross_entropy_with_logits(pred, target, weights, reduction='sum') / tot


def ghmr_torch(pred, target, label_weight, mu, bins, momentum, acc_sum):
    diff = pred - target
    loss = torch.sqrt(diff * diff + mu * mu) - mu
    g = torch.abs(diff / torch.sqrt(mu * mu + diff * diff)).detach()
    weights, tot = _weights(g, label_weight > 0, bins, 1e3, momentum, acc_sum)
    return (loss * weights).sum() / tot


def torch_head_loss(cls, reg, labels, lw, bt, bw, acc_cls, acc_reg, C, bins_cls, bins_reg, m_cls, m_reg, mu, scope):
    """-> (losses (2,) float64 tensor, the float64 leaves the losses hang on)."""
    A = cls[0].shape[1] // C
    leaves, flat_c, flat_r, n0, spans = [], [], [], 0, []
    for c, r in zip(cls, reg):
        tc = torch.from_numpy(c.astype(np.float64)).requires_grad_(True)
        tr = torch.from_numpy(r.astype(np.float64)).requires_grad_(True)
        leaves += [tc, tr]
        B, _, H, W = tc.shape
        flat_c.append(tc.reshape(B, A, C, H, W).permute(0, 3, 4, 1, 2).reshape(B, H * W * A, C))
        flat_r.append(tr.reshape(B, A, 4, H, W).permute(0, 3, 4, 1, 2).reshape(B, H * W * A, 4))
        spans.append((n0, n0 + H * W * A))
        n0 += H * W * A
    if scope == "batch":
        flat_c, flat_r, spans = [torch.cat(flat_c, 1)], [torch.cat(flat_r, 1)], [(0, n0)]
    lab, lwt = torch.from_numpy(labels), torch.from_numpy(lw.astype(np.float64))
    btt, bwt = torch.from_numpy(bt.astype(np.float64)), torch.from_numpy(bw.astype(np.float64))
    total = torch.zeros(2, dtype=torch.float64)
    for fc, fr, (a, b) in zip(flat_c, flat_r, spans):
        onehot = F.one_hot(lab[:, a:b], C + 1)[..., 1:].to(torch.float64).reshape(-1, C)      # expanded (N, C) targets
        lwe = lwt[:, a:b, None].expand(-1, -1, C).reshape(-1, C)
        lc = ghmc_torch(fc.reshape(-1, C), onehot, lwe, bins_cls, m_cls, acc_cls)
        lr = ghmr_torch(fr.reshape(-1, 4), btt[:, a:b].reshape(-1, 4), bwt[:, a:b].reshape(-1, 4), mu, bins_reg, m_reg,
                        acc_reg)
        total = total + torch.stack([lc, lr])
    return total, leaves


def _screened(cls, reg, labels, lw, bt, bw, C, bins_cls, bins_reg, mu):
    """No float64 gradient norm of a valid element within MARGIN of an edge (the case is built so; asserted, not filtered)."""
    A = cls[0].shape[1] // C
    n0 = 0
    for c, r in zip(cls, reg):
        H, W = c.shape[2:]
        n1 = n0 + H * W * A
        x = flatten_head(c, A, C).astype(np.float64)
        t = labels[:, n0:n1, None] == np.arange(1, C + 1)
        g = np.abs(1 / (1 + np.exp(-x)) - t)[lw[:, n0:n1] > 0]
        assert np.abs(g[..., None] - np.arange(bins_cls + 1) / bins_cls).min(initial=1.0) > GC.MARGIN
        d = flatten_head(r, A, 4).astype(np.float64) - bt[:, n0:n1]
        v = bw[:, n0:n1] > 0
        g = np.abs(d[v]) / np.sqrt(d[v] ** 2 + mu * mu)
        assert np.abs(g[..., None] - np.arange(bins_reg + 1) / bins_reg).min(initial=1.0) > GC.MARGIN
        n0 = n1


@pytest.mark.parametrize("scope", ["level", "batch"])
@pytest.mark.parametrize("A,C,B", [(3, 1, 1), (2, 5, 3), (9, 20, 2)])
def test_oracle_matches_the_mmdetection_form_in_float64(A, C, B, scope):
    bins_cls, bins_reg, m_cls, m_reg = 30, 10, 0.75, 0.7
    mu = float(f32(0.02))
    acc = [np.zeros(bins_cls, f32), np.zeros(bins_reg, f32)]
    acc64 = [torch.zeros(bins_cls, dtype=torch.float64), torch.zeros(bins_reg, dtype=torch.float64)]
    cot = (1.5, 0.75)
    for step in range(3):                                    # the running averages carry over
        case = GC.case(B, A, C, GC.LEVELS, 100 * A + step, bins_cls, bins_reg, mu, poison=False)
        _screened(*case, C, bins_cls, bins_reg, mu)
        ref = R.ghm_head_loss(*case, acc[0], acc[1], C, bins_cls, bins_reg, m_cls, m_reg, mu, scope, cot)
        total, leaves = torch_head_loss(*case, acc64[0], acc64[1], C, bins_cls, bins_reg, m_cls, m_reg, mu, scope)
        (total * torch.tensor(cot, dtype=torch.float64)).sum().backward()
        assert np.allclose(ref["losses64"], total.detach().numpy(), rtol=RTOL, atol=0), (ref["losses64"], total)
        for k in range(2):
            assert np.allclose(acc[k], acc64[k].numpy(), rtol=RTOL, atol=0), (step, k)
        for l in range(len(GC.LEVELS)):
            for got, leaf in ((ref["dcls"][l], leaves[2 * l]), (ref["dreg"][l], leaves[2 * l + 1])):
                want = leaf.grad.numpy()
                assert np.array_equal(got == 0, want == 0)
                assert np.allclose(got, want, rtol=RTOL, atol=0), (step, l, np.abs(got - want).max())


def test_cancellation_free_regression_loss():
    """l = d^2 / (q + mu) against sqrt(d^2 + mu^2) - mu in float64, down to |d| << mu where the float32 difference form
    has no digit left: five float32 operations, 5u (asserted with the file's 32u)."""
    mu = float(f32(0.02))
    d = (f32(10.0) ** np.linspace(-12, 3, 400)).astype(f32)
    g, l, dl = R.elem_reg(d, np.zeros_like(d), mu)
    d64 = d.astype(np.float64)
    want = d64 * d64 / (np.sqrt(d64 * d64 + mu * mu) + mu)          # the same quantity, evaluated in float64
    assert np.allclose(l, want, rtol=RTOL, atol=0)
    big = d64 > 1e-3                                                 # where float64's difference form still has 9 digits
    assert np.allclose(l[big], (np.sqrt(d64 * d64 + mu * mu) - mu)[big], rtol=1e-6, atol=0)


# ---- hand values ---------------------------------------------------------------------------------------------------
def _one_level(x, labels, lw, reg=None, bt=None, bw=None, C=1):
    """A = 1, H = 1, W = n: x (n, C) logits of one image."""
    x = np.asarray(x, f32).reshape(-1, C)
    n = x.shape[0]
    cls = x.T.reshape(1, C, 1, n).copy()
    reg = np.zeros((n, 4), f32) if reg is None else np.asarray(reg, f32)
    return ([cls], [reg.T.reshape(1, 4, 1, n).copy()], np.asarray(labels, np.int64).reshape(1, n),
            np.asarray(lw, f32).reshape(1, n), np.zeros((1, n, 4), f32) if bt is None else np.asarray(bt, f32)[None],
            np.zeros((1, n, 4), f32) if bw is None else np.asarray(bw, f32)[None])


def _run(case, C=1, **kw):
    cfg = dict(bins_cls=10, bins_reg=10, momentum_cls=0.0, momentum_reg=0.0, mu=0.02, scope="level")
    cfg.update(kw)
    return R.ghm_head_loss(*case, cfg.pop("acc_cls", None), cfg.pop("acc_reg", None), C, **cfg)


def test_one_valid_element_is_plain_bce():
    ref = _run(_one_level([0.0, 5.0], [0, 0], [1, 0]))
    assert ref["tot"][0, 0] == 1 and ref["n"][0, 0] == 1 and ref["beta"][0, 0, 5] == 1 and ref["cnt"][0, 0, 5] == 1
    assert abs(ref["losses64"][0] - np.log(2.0)) < 1e-15 and ref["losses"][0] == f32(np.log(2.0))
    assert ref["dcls"][0].ravel().tolist() == [0.5, 0.0]
    assert ref["losses"][1] == 0 and ref["tot"][1, 0] == 1                  # no valid box element: 0 / max(0, 1)


def test_the_number_of_bins_cancels():
    """Two elements in one bin and two in two bins weigh the same: beta = tot / cnt / n is 1 either way."""
    same = _run(_one_level([0.1, 0.12], [0, 0], [1, 1]))
    apart = _run(_one_level([0.1, 2.0], [0, 0], [1, 1]))
    assert same["n"][0, 0] == 1 and apart["n"][0, 0] == 2
    assert set(same["beta"][0, 0][same["cnt"][0, 0] > 0]) == {f32(1)} == set(apart["beta"][0, 0][apart["cnt"][0, 0] > 0])
    assert same["dcls"][0].ravel()[0] == apart["dcls"][0].ravel()[0]


def test_momentum_over_two_calls_and_the_empty_bin():
    acc = np.zeros(10, f32)
    acc[9] = f32(7.0)                                                       # a bin that stays empty keeps its value
    _run(_one_level([0.1, 0.12, 0.13], [0, 0, 0], [1, 1, 1]), momentum_cls=0.75, acc_cls=acc)
    assert acc[5] == f32(0.25) * f32(3) and acc[9] == f32(7.0) and np.count_nonzero(acc) == 2
    _run(_one_level([0.1, 0.12], [0, 0], [1, 1]), momentum_cls=0.75, acc_cls=acc)
    assert acc[5] == f32(f32(0.75) * f32(0.75) + f32(0.25) * f32(2)) and acc[9] == f32(7.0)


def test_scope_level_advances_acc_once_per_level():
    case = GC.case(1, 1, 1, [(1, 2), (1, 2)], 5, 10, 10, poison=False, valid=1.0)
    for c in case[0]:
        c[...] = 0.1                                                         # every class element in bin 5
    case[2][...] = 0
    a_level, a_batch = np.zeros(10, f32), np.zeros(10, f32)
    _run(case, momentum_cls=0.5, acc_cls=a_level)
    _run(case, momentum_cls=0.5, acc_cls=a_batch, scope="batch")
    assert a_level[5] == f32(0.5 * (0.5 * 2) + 0.5 * 2) and a_batch[5] == f32(0.5 * 4)


def test_all_weights_zero():
    ref = _run(_one_level([np.nan, 1.0], [1, 0], [0, 0]))
    assert ref["losses"].tolist() == [0.0, 0.0] and ref["tot"].tolist() == [[1], [1]]
    assert not ref["dcls"][0].any() and not ref["dreg"][0].any()


def test_nan_under_zero_weight_is_ignored_under_positive_weight_it_spreads():
    quiet = _run(_one_level([np.nan, np.inf, 0.3], [0, 1, 0], [0, -1.0, 1]))
    assert np.isfinite(quiet["losses"]).all() and quiet["tot"][0, 0] == 1 and quiet["dcls"][0].ravel()[:2].tolist() == [0, 0]
    loud = _run(_one_level([np.nan, 0.3], [0, 0], [1, 1]))
    assert np.isnan(loud["losses"][0]) and loud["tot"][0, 0] == 2 and loud["nan"][0, 0] == 1 and loud["cnt"][0].sum() == 1
    d = loud["dcls"][0].ravel()
    assert np.isnan(d[0]) and d[1] == f32(f32(f32(2.0) * R.elem_cls(f32(0.3), False)[2]) * f32(0.5))
    box = _run(_one_level([0, 0], [1, 1], [1, 1], reg=[[np.nan, 1, np.nan, 0]] * 2, bw=[[1, 1, 0, 0]] * 2))
    assert np.isnan(box["losses"][1]) and box["tot"][1, 0] == 4 and box["nan"][1, 0] == 2
    assert np.array_equal(np.isnan(box["dreg"][0].ravel()), [True, True, False, False, False, False, False, False])


# ---- the boundary inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(GC.KINDS))
def test_every_interior_edge_has_a_clean_crossing(dt):
    for t in (False, True):
        x = GC.cls_crossings(30, dt, t)
        assert x.shape == (2, 29) and np.array_equal(x, GC.from_key([GC.to_key(v, dt) for v in x.ravel()], dt).reshape(2, 29))
    for sign in (1, -1):
        d = GC.reg_crossings(10, dt, 0.02, sign)
        assert d.shape == (2, 9) and np.all(np.sign(d) == sign)
    assert R.bin_of(R.elem_cls(f32(0), False)[0], 30) == 15 and R.bin_of(R.elem_cls(f32(0), True)[0], 10) == 5
    g = R.elem_reg(f32(8192.0), f32(0), 0.02)[0]
    assert g == 1 and R.bin_of(g, 10, True) == 9


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_ghm_config_mirror_matches_the_header(tmp_path):
    from torch_detection_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(tdn_ghm_config));']
    for fname, _ in _lib.GhmConfig._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(tdn_ghm_config, %s));' % (fname, fname))
    lines += ['printf("bins %d stride %d scopes %d %d\\n", TDN_GHM_MAX_BINS, TDN_GHM_TABLE_STRIDE, TDN_GHM_SCOPE_LEVEL, '
              'TDN_GHM_SCOPE_BATCH);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().strip().split("\n")
    assert out[0] == "sizeof %d" % ctypes.sizeof(_lib.GhmConfig)
    for ln, (fname, _) in zip(out[1:], _lib.GhmConfig._fields_):
        assert ln == "%s %d" % (fname, getattr(_lib.GhmConfig, fname).offset)
    assert out[-1] == "bins %d stride %d scopes %d %d" % (_lib.GHM_MAX_BINS, _lib.GHM_TABLE_STRIDE, _lib.GHM_SCOPE_LEVEL,
                                                         _lib.GHM_SCOPE_BATCH)
    assert (R.MAX_BINS, R.TABLE_STRIDE) == (_lib.GHM_MAX_BINS, _lib.GHM_TABLE_STRIDE)


# ---- refusals ------------------------------------------------------------------------------------------------------
def _cpu_args(B=1, A=1, C=2, levels=((2, 2),)):
    N = sum(h * w for h, w in levels) * A
    cls = [torch.zeros(B, A * C, h, w) for h, w in levels]
    reg = [torch.zeros(B, 4 * A, h, w) for h, w in levels]
    return [cls, reg, torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N), torch.zeros(B, N, 4),
            torch.zeros(B, N, 4)]


def test_python_refusals_need_no_gpu():
    from torch_detection_amd import ghm_ops
    ok = dict(acc_cls=torch.zeros(30), acc_reg=torch.zeros(10), num_classes=2, bins_cls=30, bins_reg=10,
              momentum_cls=0.75, momentum_reg=0.7, mu=0.02, scope="level")

    def refused(match, args=None, **kw):
        cfg = dict(ok)
        cfg.update(kw)
        with pytest.raises(ValueError, match=match):
            ghm_ops.ghm_head_loss_fwd(*(args or _cpu_args()), **cfg)

    refused(r"bins_cls must be in 1\.\.64, got 0", bins_cls=0)
    refused(r"bins_reg must be in 1\.\.64, got 65", bins_reg=65)
    refused(r"momentum_cls must lie in \[0, 1\), got 1\.0", momentum_cls=1.0)
    refused(r"momentum_reg must lie in \[0, 1\), got -0\.1", momentum_reg=-0.1)
    refused(r"momentum_cls must be finite", momentum_cls=float("nan"))
    refused(r"mu must be finite and > 0, got 0\.0", mu=0.0)
    refused(r"mu must be > 0 as a float32", mu=1e-60)
    refused(r"scope must be 'level' or 'batch', got 'image'", scope="image")
    refused(r"acc_cls may be None only when its momentum is 0", acc_cls=None)
    refused(r"acc_reg must be a contiguous float32 \(10,\) tensor", acc_reg=torch.zeros(30))
    refused(r"num_classes must be in 1\.\.1024", num_classes=1025)
    refused(r"no multiple of num_classes = 3", num_classes=3)
    refused(r"takes 1\.\.8 levels", args=_cpu_args(levels=((1, 1),) * 9))
    refused(r"batch size: the number of images must be in 1\.\.64, got 65", args=_cpu_args(B=65))
    a = _cpu_args()
    a[2] = a[2][:, :3]
    refused(r"labels must be a contiguous int64 \(1, 4\) tensor.*N = 4 anchors", args=a)
    a = _cpu_args()
    a[1][0] = a[1][0].double()
    refused(r"bbox_preds\[0\] must be a float32 \(1, 4, 2, 2\) tensor", args=a)
    a = _cpu_args()
    a[0][0] = torch.zeros(1, 2, 2, 4)[..., ::2]
    refused(r"cls_scores\[0\] must be NCHW-contiguous or channels_last", args=a)
    refused(r"anchors per image \(max 1048576\)", args=_cpu_args(A=1, C=1, levels=((1024, 1025),)), num_classes=1)
    refused(r"cls_scores\[0\] must be a CUDA tensor")                           # the device is checked last
    ok0 = dict(ok, acc_cls=None, acc_reg=None, momentum_cls=0, momentum_reg=0)
    with pytest.raises(ValueError, match="must be a CUDA tensor"):              # None is fine with momentum 0
        ghm_ops.ghm_head_loss_fwd(*_cpu_args(), **ok0)
    with pytest.raises(ValueError, match=r"table must be a contiguous float32 \(2, 8, 136\) tensor"):
        ghm_ops.ghm_head_loss_bwd(*_cpu_args(), torch.zeros(2), torch.zeros(2, 8, 100), 2, 30, 10, 0.75, 0.7, 0.02, "level")
    with pytest.raises(ValueError, match=r"g must be a contiguous float32 \(2,\) tensor"):
        ghm_ops.ghm_head_loss_bwd(*_cpu_args(), torch.zeros(3), torch.zeros(2, 8, 136), 2, 30, 10, 0.75, 0.7, 0.02, "level")


def test_library_refusals_need_no_gpu():
    """The same limits as the library states them: the size query is host code."""
    from torch_detection_amd import _lib
    lib = _lib.load()

    def query(L=1, B=1, H=2, W=2, **kw):
        cfg = _lib.GhmConfig()
        vals = dict(dtype=_lib.TDN_F32, num_anchors=1, num_classes=2, bins_cls=30, bins_reg=10, scope=0,
                    momentum_cls=0.75, momentum_reg=0.7, mu=0.02)
        vals.update(kw)
        for k, v in vals.items():
            setattr(cfg, k, v)
        levels = (_lib.LossLevel * max(L, 1))()
        for lv in levels:
            lv.H, lv.W = H, W
        n = lib.tdn_ghm_workspace_bytes(levels, L, B, ctypes.byref(cfg))
        return n, lib.tdn_last_error().decode()

    n, _ = query()
    assert n > 0 and n % 256 == 0
    for kw, msg in ((dict(bins_cls=0), "bins_cls=0, bins_reg=10 (1..64 each)"), (dict(bins_reg=65), "bins_reg=65"),
                    (dict(momentum_cls=1.0), "each in [0, 1)"), (dict(momentum_reg=-0.5), "each in [0, 1)"),
                    (dict(mu=0.0), "mu must be finite and > 0"), (dict(mu=float("inf")), "mu must be finite and > 0"),
                    (dict(scope=2), "scope 2 is neither level (0) nor batch (1)"), (dict(L=9), "9 levels (1..8)"),
                    (dict(L=0), "0 levels (1..8)"), (dict(B=65), "B=65 out of 1..64"), (dict(dtype=7), "dtype 7"),
                    (dict(num_classes=1025), "C=1025 (C in 1..1024)"), (dict(H=0), "level 0 is 0 x 2"),
                    (dict(H=1024, W=1025), "more than 1048576 anchors per image"),
                    (dict(H=1024, W=1024, B=64, num_classes=32), "elements (2^31 or more)")):
        n, err = query(**kw)
        assert n == -1 and msg in err, (kw, n, err)


def test_modules_and_the_retina_head_hook():
    import torch_detection_amd as T
    c, r = T.GHMC(bins=30, momentum=0.75), T.GHMR(mu=0.02, bins=10, momentum=0.7, loss_weight=2.0)
    assert (c.bins, c.momentum, c.loss_weight, c.use_sigmoid) == (30, 0.75, 1.0, True) and c.acc_sum.shape == (30,)
    assert (r.mu, r.bins, r.momentum, r.loss_weight) == (0.02, 10, 0.7, 2.0) and r.acc_sum.dtype == torch.float32
    assert T.GHMC().acc_sum is None and T.GHMC().bins == 10 and T.GHMR().momentum == 0          # mmdetection's defaults
    assert not c.state_dict() and not r.state_dict()
    with pytest.raises(NotImplementedError, match="use_sigmoid"):
        T.GHMC(use_sigmoid=False)
    with pytest.raises(ValueError, match=r"bins must be in 1\.\.64"):
        T.GHMR(bins=100)
    with pytest.raises(ValueError, match=r"momentum must lie in \[0, 1\)"):
        T.GHMC(momentum=1)
    plain = T.RetinaHead(6, 64, feat_channels=64, stacked_convs=1)
    head = T.RetinaHead(6, 64, feat_channels=64, stacked_convs=1, loss_cls=dict(type='GHMC', bins=30, momentum=0.75),
                        loss_bbox=r)
    assert isinstance(head.loss_cls, T.GHMC) and head.loss_bbox is r and head.loss_cls.bins == 30
    assert sorted(head.state_dict()) == sorted(plain.state_dict()) and not hasattr(plain, "loss_cls")
    assert len(list(head.parameters())) == len(list(plain.parameters()))
    for kw in (dict(loss_cls=c), dict(loss_bbox=r), dict(loss_cls=dict(type='FocalLoss'), loss_bbox=r),
               dict(loss_cls=c, loss_bbox=dict(type='SmoothL1Loss', beta=0.11)), dict(loss_cls=r, loss_bbox=c)):
        with pytest.raises(NotImplementedError, match="RetinaHead: loss_(cls|bbox) must be a GHM"):
            T.RetinaHead(6, 64, **kw)
