"""NumPy restatement of GroupNorm and training-mode BatchNorm2d in float64: the CPU oracle of csrc/gn.hip.

Plain closed forms on NCHW arrays, no autograd.  The variance is the biased, two-pass one, ``mean((z - mu)**2)``, so
the oracle itself has no cancellation whatever the ratio |mean| / std of the input.  ``relu`` is 0 (none), 1 (ReLU) or
2 (ReLU6); an ``up2x`` addend is the coarser level (H/2 x W/2), added after nearest-neighbour 2x upsampling.
Inputs may be any real arrays; the GPU tests pass the STORED values (a bf16 / fp16 tensor converted exactly).
"""
import numpy as np

F64 = np.float64


def _epilogue(pre, addend, up2x, relu):
    if addend is not None:
        a = np.asarray(addend, F64)
        if up2x:
            a = a.repeat(2, axis=2).repeat(2, axis=3)
        pre = pre + a
    if relu:
        pre = np.maximum(pre, 0.0)
        if relu == 2:
            pre = np.minimum(pre, 6.0)
    return pre


def _vec(v):
    return np.asarray(v, F64)[None, :, None, None]


def gn_stats(z, G, eps):
    """(mean, rstd, var) per (sample, group), each (N, G)."""
    z = np.asarray(z, F64)
    N, C = z.shape[:2]
    zg = z.reshape(N, G, -1)
    mu = zg.mean(-1)
    var = ((zg - mu[..., None]) ** 2).mean(-1)
    return mu, 1.0 / np.sqrt(var + F64(eps)), var


def _gn_normalise(z, G, eps):
    z = np.asarray(z, F64)
    N = z.shape[0]
    mu, rstd, var = gn_stats(z, G, eps)
    xhat = ((z.reshape(N, G, -1) - mu[..., None]) * rstd[..., None]).reshape(z.shape)
    return xhat, mu, rstd


def gn_xhat(z, G, eps):
    return _gn_normalise(z, G, eps)[0]


def gn_fwd(z, gamma, beta, G, eps, addend=None, up2x=False, relu=0):
    """y (N, C, H, W), mean (N, G), rstd (N, G)."""
    xhat, mu, rstd = _gn_normalise(z, G, eps)
    return _epilogue(xhat * _vec(gamma) + _vec(beta), addend, up2x, relu), mu, rstd


def gn_bwd(g, z, gamma, G, eps):
    """(dz, dgamma, dbeta) from g = dL/d(normalised, affine output), i.e. with any ReLU mask already applied."""
    g = np.asarray(g, F64)
    N = g.shape[0]
    xh, _, rstd = _gn_normalise(z, G, eps)
    dgamma = (g * xh).sum((0, 2, 3))
    dbeta = g.sum((0, 2, 3))
    dx = (g * _vec(gamma)).reshape(N, G, -1)
    xg = xh.reshape(N, G, -1)
    m1 = dx.mean(-1, keepdims=True)
    m2 = (dx * xg).mean(-1, keepdims=True)
    dz = (rstd[..., None] * (dx - m1 - xg * m2)).reshape(g.shape)
    return dz, dgamma, dbeta


def bn_stats(z, eps):
    """(mean, rstd, biased var) per channel over (N, H, W), each (C,)."""
    z = np.asarray(z, F64)
    mu = z.mean((0, 2, 3))
    var = ((z - _vec(mu)) ** 2).mean((0, 2, 3))
    return mu, 1.0 / np.sqrt(var + F64(eps)), var


def bn_train_fwd(z, gamma, beta, eps, addend=None, up2x=False, relu=0, running_mean=None, running_var=None,
                 momentum=0.1):
    """y, mean (C,), rstd (C,), updated running_mean, running_var (None when none were given).  The running variance
    takes the unbiased batch variance — the biased one when N*H*W == 1, where the unbiased one does not exist."""
    z = np.asarray(z, F64)
    mu, rstd, var = bn_stats(z, eps)
    y = _epilogue((z - _vec(mu)) * _vec(rstd) * _vec(gamma) + _vec(beta), addend, up2x, relu)
    rm = rv = None
    if running_mean is not None:
        cnt = z.shape[0] * z.shape[2] * z.shape[3]
        unb = var * cnt / (cnt - 1) if cnt > 1 else var
        m = F64(momentum)
        rm = (1 - m) * np.asarray(running_mean, F64) + m * mu
        rv = (1 - m) * np.asarray(running_var, F64) + m * unb
    return y, mu, rstd, rm, rv


def bn_train_bwd(g, z, gamma, eps):
    g = np.asarray(g, F64)
    z = np.asarray(z, F64)
    mu, rstd, _ = bn_stats(z, eps)
    xh = (z - _vec(mu)) * _vec(rstd)
    dgamma = (g * xh).sum((0, 2, 3))
    dbeta = g.sum((0, 2, 3))
    dx = g * _vec(gamma)
    m1 = dx.mean((0, 2, 3), keepdims=True)
    m2 = (dx * xh).mean((0, 2, 3), keepdims=True)
    dz = _vec(rstd) * (dx - m1 - xh * m2)
    return dz, dgamma, dbeta
