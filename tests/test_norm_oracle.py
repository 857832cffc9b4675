"""The float64 oracle of the normalisation kernels (tests/norm_ref.py) against torch's own GroupNorm / BatchNorm with
autograd in float64, and the host-side answers of tdn_gn_workspace.  No GPU: the library loads without one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_ref as R
import test_gpu_gn as GN

RTOL = 1e-12


def _rand(shape, seed, lo=-1.0, hi=1.0):
    return GN._det(shape, seed, lo, hi)


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    den = float(np.abs(b).max())
    assert float(np.abs(a - b).max()) <= RTOL * (den if den > 0 else 1.0), what


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _operands(N, C, H, W):
    n = np.arange(N, dtype=np.float64).reshape(-1, 1, 1, 1)
    z = _rand((N, C, H, W), 1, -2, 2) * 2.0 ** (n % 3) + 0.3 + n
    return (z, _rand((C,), 2, 0.5, 1.5), _rand((C,), 3, -0.5, 0.5), _rand((N, C, H, W), 4),
            _rand((N, C, H // 2, W // 2), 6), _rand((N, C, H, W), 5))


def _torch_epilogue(pre, res, coarse, mode, relu):
    if mode == "same":
        pre = pre + _t(res)
    elif mode == "up2x":
        pre = pre + F.interpolate(_t(coarse), scale_factor=2, mode="nearest")
    return {0: pre, 1: F.relu(pre), 2: F.relu6(pre)}[relu]


MODES = [(None, 0), ("same", 1), ("up2x", 0), ("up2x", 2)]


@pytest.mark.parametrize("mode,relu", MODES)
@pytest.mark.parametrize("case", [(2, 8, 4, 6, 8), (3, 12, 2, 4, 1), (1, 16, 6, 2, 4)])   # cpg = 1; G = 1; cpg = 4
def test_gn_oracle_matches_torch_float64(case, mode, relu):
    N, C, H, W, G = case
    z, gamma, beta, res, coarse, cot = _operands(N, C, H, W)
    eps = 1e-5
    zt, gt, bt = (_t(a).requires_grad_(True) for a in (z, gamma, beta))
    pre = F.group_norm(zt, G, gt, bt, eps)
    ref = _torch_epilogue(pre, res, coarse, mode, relu)
    y, mean, rstd = R.gn_fwd(z, gamma, beta, G, eps, {None: None, "same": res, "up2x": coarse}[mode], mode == "up2x",
                             relu)
    _close(y, ref.detach().numpy(), "y")
    zg = zt.detach().view(N, G, -1)
    _close(mean, zg.mean(-1).numpy(), "mean")
    _close(rstd, (1.0 / torch.sqrt(zg.var(-1, unbiased=False) + eps)).numpy(), "rstd")
    g = cot * ((y > 0) & ((y < 6) | (relu != 2)) if relu else 1.0)     # the mask the consumer applies
    pre.backward(_t(g))
    dz, dgamma, dbeta = R.gn_bwd(g, z, gamma, G, eps)
    _close(dz, zt.grad.numpy(), "dz")
    _close(dgamma, gt.grad.numpy(), "dgamma")
    _close(dbeta, bt.grad.numpy(), "dbeta")


@pytest.mark.parametrize("mode,relu", MODES)
@pytest.mark.parametrize("case", [(2, 8, 4, 6), (3, 12, 2, 4), (1, 16, 6, 2)])
def test_bn_oracle_matches_torch_float64(case, mode, relu):
    N, C, H, W = case
    z, gamma, beta, res, coarse, cot = _operands(N, C, H, W)
    eps = 1e-5
    zt, gt, bt = (_t(a).requires_grad_(True) for a in (z, gamma, beta))
    pre = F.batch_norm(zt, None, None, gt, bt, True, 0.1, eps)
    ref = _torch_epilogue(pre, res, coarse, mode, relu)
    y, mean, rstd, rm, rv = R.bn_train_fwd(z, gamma, beta, eps, {None: None, "same": res, "up2x": coarse}[mode],
                                           mode == "up2x", relu)
    assert rm is None and rv is None
    _close(y, ref.detach().numpy(), "y")
    _close(mean, zt.detach().mean((0, 2, 3)).numpy(), "mean")
    _close(rstd, (1.0 / torch.sqrt(zt.detach().var((0, 2, 3), unbiased=False) + eps)).numpy(), "rstd")
    g = cot * ((y > 0) & ((y < 6) | (relu != 2)) if relu else 1.0)
    pre.backward(_t(g))
    dz, dgamma, dbeta = R.bn_train_bwd(g, z, gamma, eps)
    _close(dz, zt.grad.numpy(), "dz")
    _close(dgamma, gt.grad.numpy(), "dgamma")
    _close(dbeta, bt.grad.numpy(), "dbeta")


@pytest.mark.parametrize("momentum", [0.1, 0.25, 1.0])
def test_running_statistics_match_torch_float64(momentum):
    N, C, H, W = 3, 12, 2, 4
    z, gamma, beta, _, _, _ = _operands(N, C, H, W)
    rm0, rv0 = _rand((C,), 7, -0.2, 0.2), _rand((C,), 8, 0.5, 1.5)
    rmt, rvt = _t(rm0).clone(), _t(rv0).clone()
    F.batch_norm(_t(z), rmt, rvt, _t(gamma), _t(beta), True, momentum, 1e-5)
    _, _, _, rm, rv = R.bn_train_fwd(z, gamma, beta, 1e-5, running_mean=rm0, running_var=rv0, momentum=momentum)
    _close(rm, rmt.numpy(), "running_mean")
    _close(rv, rvt.numpy(), "running_var")


def test_running_variance_of_one_value_is_the_biased_one():
    """N*H*W == 1: the unbiased variance does not exist (torch refuses the shape); the kernel documents the biased one,
    which is zero."""
    z = _rand((1, 8, 1, 1), 1, -2, 2)
    rm0, rv0 = _rand((8,), 7, -0.2, 0.2), _rand((8,), 8, 0.5, 1.5)
    y, mean, rstd, rm, rv = R.bn_train_fwd(z, np.ones(8), np.zeros(8), 1e-5, running_mean=rm0, running_var=rv0,
                                           momentum=0.25)
    _close(mean, z.reshape(8), "mean")
    _close(rstd, np.full(8, 1e-5 ** -0.5), "rstd")
    _close(y, np.zeros_like(z), "y")
    _close(rm, 0.75 * rm0 + 0.25 * z.reshape(8), "running_mean")
    _close(rv, 0.75 * rv0, "running_var")


# ---- tdn_gn_workspace: refusals and sizes ---------------------------------------------------------------------
def ws_bytes(N, H, W, C, G):
    """part [N][chunks][2][C] + 3 N C coefficient floats, + 256: the chunking of make_geom (csrc/gn.hip) restated"""
    ceil_div = lambda a, b: -(-a // b)   # noqa: E731
    HW = H * W
    ppp = 256 // (C // 8)                                   # pixels per pass of a 256-thread block
    chunks = max(1, min(ceil_div(1024, N), ceil_div(HW, ppp * 4)))
    chunk_px = ceil_div(HW, chunks)
    chunks = ceil_div(HW, chunk_px)
    return (N * chunks * 2 * C + N * C * 3) * 4 + 256


REFUSED = [  # N, H, W, C, G, what tdn_last_error must name
    (1, 4, 4, 32, 32, b"C=32 must be a power of two in 64..2048"),
    (1, 4, 4, 96, 32, b"C=96 must be a power of two in 64..2048"),
    (1, 4, 4, 4096, 32, b"C=4096 must be a power of two in 64..2048"),
    (1, 4, 4, 64, 48, b"48 groups do not divide 64 channels"),
    (1, 4, 4, 64, 0, b"0 groups do not divide 64 channels"),
    (1, 4, 4, 2048, 4, b"512 channels per group not supported"),
    (0, 4, 4, 64, 32, b"bad shape N=0"),
    (1, 0, 4, 64, 32, b"bad shape N=1 H=0"),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: "N%d-H%d-W%d-C%d-G%d" % c[:5])
def test_gn_workspace_refuses(case):
    from torch_detection_amd import _lib
    lib = _lib.load()
    N, H, W, C, G, why = case
    assert lib.tdn_gn_workspace(N, H, W, C, G) == -1
    assert why in lib.tdn_last_error(), lib.tdn_last_error()


def _geometries():
    gn = [c[:5] for c in GN.GEOM_CASES + [GN.BIG_CASE]] + [c + (32,) for c in GN.CASES + GN.COND_SHAPES]
    gn += [s + (s[1] // 2,) for s in GN.COND_SHAPES] + [GN.OPT_SHAPE + (32,)]
    bn = [c[:4] for c in GN.BN_GEOM_CASES + [GN.BN_BIG_CASE]] + GN.BN_CASES + GN.COND_SHAPES + [GN.OPT_SHAPE]
    return sorted(set(gn + [c + (c[1],) for c in bn]))


@pytest.mark.parametrize("case", _geometries(), ids=lambda c: "-".join(map(str, c)))
def test_gn_workspace_size(case):
    """Every geometry the GPU tests run (BatchNorm asks with G = C): the size is the documented layout."""
    from torch_detection_amd import _lib
    N, C, H, W, G = case
    assert _lib.load().tdn_gn_workspace(N, H, W, C, G) == ws_bytes(N, H, W, C, G)


def test_gn_workspace_chunking_branches():
    """The restatement above takes each of its branches at some tested geometry."""
    chunks = lambda N, C, H, W, G: (ws_bytes(N, H, W, C, G) - 256 - N * C * 12) // (N * 2 * C * 4)   # noqa: E731
    assert chunks(1024, 64, 2, 2, 32) == 1 and chunks(2, 64, 1, 1, 32) == 1      # N >= 1024; HW below one pass
    assert chunks(1, 64, 37, 41, 32) == 12                                       # ceil(1517 / 128); ragged: 12 * 127
    assert chunks(1, 64, 514, 512, 32) == 1024                                   # capped by 1024 / N
    assert chunks(2, 2048, 3, 2, 8) == 2                                         # one pixel per pass: ceil(6 / 4)
