"""NumPy restatement, in float64, of GroupNorm (+ ReLU) with shared affine parameters over a pyramid: the CPU oracle of
csrc/pyramid_gn.hip.  Per level it is tests/norm_ref.py; the statistics are per (level, image, group),
``gamma`` / ``beta`` are shared, and the affine gradients are the sums over the levels.  An empty level (H or W zero)
gives empty maps and contributes nothing.  Arrays are NCHW."""
import numpy as np

import norm_ref as N

F64 = np.float64


def fwd(zs, gamma, beta, G, eps, relu):
    """-> (ys, means, rstds): per level y (B, C, H, W), mean and rstd (B, G) (zeros for an empty level)."""
    ys, means, rstds = [], [], []
    for z in zs:
        z = np.asarray(z, F64)
        if z.size == 0:
            ys.append(z.copy())
            means.append(np.zeros((z.shape[0], G)))
            rstds.append(np.zeros((z.shape[0], G)))
            continue
        y, mu, rstd = N.gn_fwd(z, gamma, beta, G, eps, relu=1 if relu else 0)
        ys.append(y)
        means.append(mu)
        rstds.append(rstd)
    return ys, means, rstds


def masked(gs, zs, gamma, beta, G, eps, relu):
    """The cotangents as the backward counts them: exactly 0 where the reference output is not positive (``relu``)."""
    if not relu:
        return [np.asarray(g, F64) for g in gs]
    ys, _, _ = fwd(zs, gamma, beta, G, eps, True)
    return [np.asarray(g, F64) * (y > 0) for g, y in zip(gs, ys)]


def bwd(gs, zs, gamma, beta, G, eps, relu, mask_src=None):
    """-> (dzs, dgamma, dbeta) from the UNMASKED cotangents.  ``mask_src``: the maps whose sign masks (default: the
    reference output; the GPU tests pass the device's stored y, whose sign may differ where y rounds to zero)."""
    C = np.asarray(gamma).shape[0]
    if relu and mask_src is not None:
        gm = [np.asarray(g, F64) * (np.asarray(y, F64) > 0) for g, y in zip(gs, mask_src)]
    else:
        gm = masked(gs, zs, gamma, beta, G, eps, relu)
    dzs, dgamma, dbeta = [], np.zeros(C), np.zeros(C)
    for g, z in zip(gm, zs):
        z = np.asarray(z, F64)
        if z.size == 0:
            dzs.append(z.copy())
            continue
        dz, dg, db = N.gn_bwd(g, z, gamma, G, eps)
        dzs.append(dz)
        dgamma += dg
        dbeta += db
    return dzs, dgamma, dbeta
