"""CPU: the NumPy oracle of the Libra R-CNN losses (tests/libra_ref.py) against torch float64 autograd of
mmdetection's balanced L1, and the host-side refusals of the new keywords."""
import numpy as np
import pytest
import torch

import libra_ref as R

PARAMS = [(1.0, 0.5, 1.5), (1.0 / 9.0, 0.5, 1.5), (0.75, 0.25, 1.0)]        # (beta, alpha, gamma)


def _mmdet_balanced_l1(pred, target, beta, alpha, gamma):
    """mmdetection's ``balanced_l1_loss`` (reduction 'none')"""
    diff = torch.abs(pred - target)
    b = np.e ** (gamma / alpha) - 1
    return torch.where(diff < beta, alpha / b * (b * diff + 1) * torch.log(b * diff / beta + 1) - alpha * diff,
                       gamma * diff + gamma / b - alpha * beta)


def _f(v):
    return float(np.float32(v))


@pytest.mark.parametrize("beta,alpha,gamma", PARAMS)
def test_balanced_l1_oracle_against_float64_autograd(beta, alpha, gamma):
    rng = np.random.default_rng(3)
    pred = rng.normal(0, 1.0, 4000).astype(np.float32)
    target = rng.normal(0, 0.5, 4000).astype(np.float32)
    p = torch.from_numpy(pred).double().requires_grad_(True)
    loss = _mmdet_balanced_l1(p, torch.from_numpy(target).double(), _f(beta), _f(alpha), _f(gamma))
    loss.sum().backward()
    l64, g64 = R.balanced_l1(pred, target, beta, alpha, gamma)
    assert np.allclose(l64, loss.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert np.allclose(g64, p.grad.numpy(), rtol=1e-12, atol=1e-14)
    both = np.abs(pred - target) < np.float32(beta)
    assert both.any() and (~both).any()
    # the float32 restatement: a few units of 2^-24 of the terms it adds (the loss is a difference of two terms)
    l32, g32, outer = R.balanced_l1_32(pred, target, beta, alpha, gamma)
    a = np.abs(pred.astype(np.float64) - target)
    terms = np.where(outer, _f(gamma) * a + abs(float(R.balanced_consts(beta, alpha, gamma)[2])), 2 * _f(alpha) * a + l64)
    assert (np.abs(l32 - l64) <= 8 * 2.0 ** -24 * terms + 1e-45).all()
    dmax = _f(gamma) + _f(alpha) * abs(1 - _f(beta)) / _f(beta)          # the largest |dl| of the inner branch
    assert (np.abs(g32 - g64) <= 8 * 2.0 ** -24 * dmax).all()
    assert np.array_equal(outer, ~both)
    assert np.array_equal(g32[outer], (np.sign(pred - target) * np.float32(gamma))[outer])


@pytest.mark.parametrize("beta,alpha,gamma", PARAMS)
def test_continuous_at_the_knee_and_exact_at_zero(beta, alpha, gamma):
    be = np.float32(beta)
    below = np.nextafter(be, np.float32(0))
    t = np.zeros(3, np.float32)
    l64, g64 = R.balanced_l1(np.array([below, be, -be], np.float32), t, beta, alpha, gamma)
    assert abs(l64[0] - l64[1]) <= 4 * 2.0 ** -24 * _f(gamma) * _f(beta) and l64[1] == l64[2]
    # the gradient steps at the knee by alpha (1 - beta) / (beta (b + 1)) unless beta is 1: mmdetection's function does
    step = _f(alpha) * (1 - _f(beta)) / (_f(beta) * np.exp(_f(gamma) / _f(alpha)))
    assert abs(g64[0] - g64[1] - step) <= 4 * 2.0 ** -24 * _f(gamma) and g64[1] == _f(gamma) and g64[2] == -_f(gamma)
    l32, g32, outer = R.balanced_l1_32(np.array([below, be, -be], np.float32), t, beta, alpha, gamma)
    assert list(outer) == [False, True, True]                       # a == beta takes the outer branch
    assert abs(float(l32[0]) - float(l32[1])) <= 8 * 2.0 ** -24 * _f(gamma) * _f(beta)
    z = np.array([0.25, -1.5, 0.0], np.float32)
    l32, g32, _ = R.balanced_l1_32(z, z.copy(), beta, alpha, gamma)
    assert (l32 == 0).all() and (g32 == 0).all()
    l64, g64 = R.balanced_l1(z, z.copy(), beta, alpha, gamma)
    assert (l64 == 0).all() and (g64 == 0).all()


def test_constants_are_rounded_once_from_double():
    b, a_over_b, c, k = R.balanced_consts(1.0, 0.5, 1.5)
    e3 = np.exp(3.0) - 1.0
    assert b == np.float32(e3) and a_over_b == np.float32(0.5 / e3) and c == np.float32(1.5 / e3 - 0.5) and k == 0
    # at beta = 1 the gradient is sign(d) (alpha t) bit for bit: the knee term is +0
    pred = np.linspace(-0.99, 0.99, 199).astype(np.float32)
    _, g32, outer = R.balanced_l1_32(pred, np.zeros_like(pred), 1.0, 0.5, 1.5)
    t = np.log1p(((b * np.abs(pred)).astype(np.float32) / np.float32(1)).astype(np.float32)).astype(np.float32)
    assert not outer.any() and np.array_equal(g32.view(np.uint32), (np.sign(pred) * (np.float32(0.5) * t)).view(np.uint32))


def test_keyword_refusals_need_no_gpu():
    import torch_detection_amd as T
    z = torch.zeros
    args = (z(2, 3), z(2, 12), z(2, dtype=torch.int64), z(2), z(2, 4), z(2, 4))
    with pytest.raises(ValueError, match="reg_loss"):
        T.bbox_head_loss(*args, reg_loss="l2")
    with pytest.raises(ValueError, match="reg_alpha"):
        T.bbox_head_loss(*args, reg_loss="balanced_l1", reg_alpha=0.0)
    with pytest.raises(ValueError, match="reg_gamma"):
        T.bbox_head_loss(*args, reg_loss="balanced_l1", reg_gamma=float("inf"))
    with pytest.raises(ValueError, match="at most 80"):
        T.bbox_head_loss(*args, reg_loss="balanced_l1", reg_alpha=0.01, reg_gamma=1.5)
    with pytest.raises(ValueError, match="CUDA"):
        T.bbox_head_loss(*args, reg_loss="balanced_l1")              # everything else was fine: the device comes last


# ---- IoU-balanced negative sampling -------------------------------------------------------------------------------------------
def _neg(overlaps, keys, n, assigned=None, **kw):
    o = np.asarray(overlaps, np.float32)
    a = np.zeros(o.shape, np.int32) if assigned is None else np.asarray(assigned, np.int32)
    k = np.asarray(keys, np.int64)
    got = R.iou_balanced_negatives(a, o, k, n, **kw)
    assert np.array_equal(got, R.lineage_negatives(a, o, k, n, **kw))
    return got.tolist()


def test_sampler_hand_worked_cases():
    # fewer negatives than may be kept: all of them
    assert _neg([0.1, 0.2, 0.9, 0.4, 0.3], [5, 4, 3, 2, 1], 5, assigned=[0, 0, 1, -1, 0]) == [0, 1, 4]
    # m = 0.9 comes from a POSITIVE; bins of width 0.3: an overfull one (4 -> 2), an underfull one (1) that feeds the
    # extras, an overfull one (3 -> 2); one extra from the rest by key
    o = [0.05, 0.10, 0.15, 0.20, 0.35, 0.65, 0.70, 0.75, 0.9]
    assert _neg(o, [5, 1, 7, 3, 9, 2, 8, 4, 0], 6, assigned=[0] * 8 + [1]) == [0, 1, 3, 4, 5, 7]
    # a candidate at o == m lies in no bin and is reachable only as an extra
    o = [0.125, 0.25, 0.375, 0.5, 0.625, 0.75]
    assert _neg(o, [0, 5, 1, 7, 2, 3], 5) == [0, 1, 2, 4, 5]
    assert _neg(o, [0, 5, 1, 7, 2, 3], 4) == [0, 2, 4, 5]
    assert _neg(o, [0, 5, 1, 7, 2, 9], 4) == [0, 1, 2, 4]            # ... and not when its key is the largest
    # all keys equal: the index decides
    assert _neg(o, [7] * 6, 5) == [0, 1, 2, 3, 4]
    # num_bins = 1: the n_S smallest of S
    assert _neg(o, [0, 5, 1, 7, 2, 3], 3, num_bins=1) == [0, 2, 4]
    # empty S (every overlap below the floor): everything comes from F
    assert _neg([0.1, 0.2, 0.3, 0.4], [3, 1, 2, 0], 2, floor_thr=0.5, floor_fraction=0.25) == [1, 3]
    # floor_thr == 0: F = {o == 0}, S = {o > 0}; n_S = int(4 * 0.75) = 3 = |S|: all of S, one of F by key
    assert _neg([0, 0, 0.25, 0.5, 0, 0.75], [9, 2, 0, 0, 1, 0], 4, floor_thr=0.0, floor_fraction=0.25) == [2, 3, 4, 5]
    # F too small: S gives n_S = 2, F its only member, the last one comes from the remaining negatives by key
    o = [0.1, 0.5, 0.625, 0.75, 0.875, 0.9375]
    assert _neg(o, [4, 3, 0, 5, 1, 2], 4, floor_thr=0.5, floor_fraction=0.5, num_bins=1) == [0, 2, 4, 5]


@pytest.mark.parametrize("floor_thr", [-1.0, 0.0, 0.1])
@pytest.mark.parametrize("floor_fraction", [0.0, 0.25])
@pytest.mark.parametrize("num_bins", [1, 3])
def test_sampler_oracle_equals_the_set_restatement(floor_thr, floor_fraction, num_bins):
    rng = np.random.default_rng(int(100 * (floor_thr + 2)) + int(8 * floor_fraction) + num_bins)
    for trial in range(12):
        N = int(rng.integers(5, 400))
        o = rng.choice([0.0, 0.0, 0.03, 0.07, 0.2, 0.31, 0.45], N).astype(np.float32) + \
            (rng.random(N) < 0.5) * rng.random(N).astype(np.float32) * np.float32(0.04)
        a = rng.choice([-1, 0, 0, 0, 1, 2], N).astype(np.int32)
        o[a > 0] = rng.uniform(0.5, 0.95, int((a > 0).sum())).astype(np.float32)
        o[a < 0] = 0.48
        keys = rng.integers(0, 12 if trial % 2 else 1 << 31, N).astype(np.int64)        # odd trials: many equal keys
        for n in (0, 1, 7, 64, N):
            _neg(o, keys, n, assigned=a, floor_thr=floor_thr, floor_fraction=floor_fraction, num_bins=num_bins)


def test_sample_assigned_iou_balanced_keeps_the_positives_and_the_counts():
    import target_ref as TR
    rng = np.random.default_rng(5)
    a = rng.choice([-1, 0, 0, 0, 0, 1, 2], (3, 300)).astype(np.int32)
    o = rng.random((3, 300)).astype(np.float32) * np.float32(0.5)
    a[1] = np.where(a[1] == 0, -1, a[1])                                  # an image without negatives
    for keys in (None, rng.integers(0, 1 << 31, (3, 300)).astype(np.int32)):
        pm, nm, npos, nneg = R.sample_assigned_iou_balanced(a, o, 64, 0.25, neg_pos_ub=3, keys=keys, seed=9)
        pm0, nm0, npos0, nneg0 = TR.sample_assigned(a, 64, 0.25, neg_pos_ub=3, keys=keys, seed=9)
        assert np.array_equal(pm, pm0) and np.array_equal(npos, npos0) and np.array_equal(nneg, nneg0)
        assert np.array_equal(nm.sum(1), nneg) and not (nm & (a != 0)).any() and nneg[1] == 0
        assert not np.array_equal(nm, nm0)                                # another choice of the same number


def test_sampler_keyword_refusals_need_no_gpu():
    import torch_detection_amd as T
    a, o = torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8)
    with pytest.raises(ValueError, match="num_bins"):
        T.sample_assigned_iou_balanced(a, o, 4, 0.25, num_bins=9)
    with pytest.raises(ValueError, match="num_bins"):
        T.sample_assigned_iou_balanced(a, o, 4, 0.25, num_bins=0)
    with pytest.raises(ValueError, match="floor_fraction"):
        T.sample_assigned_iou_balanced(a, o, 4, 0.25, floor_fraction=1.5)
    with pytest.raises(ValueError, match="floor_thr"):
        T.sample_assigned_iou_balanced(a, o, 4, 0.25, floor_thr=1.0)
    with pytest.raises(ValueError, match="max_overlaps"):
        T.sample_assigned_iou_balanced(a, o[:, :4], 4, 0.25)
    with pytest.raises(ValueError, match="CUDA"):
        T.sample_assigned_iou_balanced(a, o, 4, 0.25)
    z = torch.zeros
    with pytest.raises(ValueError, match="neg_sampler"):
        T.sample_rois(z(1, 4, 5), z(1, dtype=torch.int32), z(1, 2, 4), z(1, 2, dtype=torch.int64), z(1, dtype=torch.int32),
                      neg_sampler="ohem")


def test_new_struct_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of tdn_balanced_config as gcc lays it out == the ctypes mirror in _lib.py."""
    import ctypes
    import os
    import subprocess
    from torch_detection_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cls, cname = _lib.BalancedConfig, "tdn_balanced_config"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {',
             'printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    rows = [ln.split() for ln in subprocess.check_output([str(exe)]).decode().split("\n") if ln]
    assert len(rows) == len(cls._fields_) + 1
    for fname, val in rows:
        got = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert got == int(val), (fname, got, val)
