"""fp64 oracle of the dense head predictors (csrc/dense_head.hip) and their a-priori rounding bounds
(test infrastructure; pure CPU, torch only).

The two 1x1 predictors of all pyramid levels are ONE linear layer on the level-concatenated rows with the stacked weight
(the A cls rows, then the 4A reg rows), so the oracle is ``linear_ref.fwd / dgrad / wgrad`` and the allowance is
``linear_ref``'s ``*_bound`` (``bound_util`` on 1x1 views) unchanged: no tolerance is invented here.

Conventions.  A pyramid is a list of NHWC tensors: hidden maps ``hs[l]`` (B, H_l, W_l, C), outputs / cotangents
``cls[l]`` (B, H_l, W_l, A) and ``reg[l]`` (B, H_l, W_l, 4A) — fp32 containers of 16-bit values; ``wc`` (A, C) and ``wr``
(4A, C) already rounded to the compute type (``round16``), biases fp32.
"""
import torch

import linear_ref as LR

round16 = LR.round16
within = LR.within


def rows(ts):
    """list of (B, H_l, W_l, ch) -> the level-concatenated (sum of B*H_l*W_l, ch) matrix"""
    return torch.cat([t.reshape(-1, t.shape[-1]) for t in ts])


def split(mat, like, ch=None):
    """inverse of ``rows``: the (M, ch) matrix cut back into levels shaped like ``like``'s (ch channels)"""
    out, m = [], 0
    for t in like:
        n = t.shape[0] * t.shape[1] * t.shape[2]
        out.append(mat[m:m + n].reshape(t.shape[0], t.shape[1], t.shape[2], mat.shape[1] if ch is None else ch))
        m += n
    return out


def stack(wc, wr):
    return torch.cat([wc.reshape(wc.shape[0], -1), wr.reshape(wr.shape[0], -1)])


def stack_g(g_cls, g_reg):
    return torch.cat([rows(g_cls), rows(g_reg)], 1)


def fwd(hs, wc, bc, wr, br):
    """-> (cls, reg) lists, fp64 NHWC"""
    y = LR.fwd(rows(hs), stack(wc, wr), torch.cat([bc, br]))
    A = wc.shape[0]
    return split(y[:, :A].contiguous(), hs), split(y[:, A:].contiguous(), hs)


def dgrad(g_cls, g_reg, wc, wr, hs):
    """-> dh list, fp64 NHWC, zero where hs <= 0"""
    return split(LR.dgrad(stack_g(g_cls, g_reg), stack(wc, wr), None, rows(hs)), hs)


def wgrad(hs, g_cls, g_reg):
    """-> (dwc (A, C), dbc, dwr (4A, C), dbr), fp64"""
    dw, db = LR.wgrad(rows(hs), stack_g(g_cls, g_reg))
    A = g_cls[0].shape[-1]
    return dw[:A], db[:A], dw[A:], db[A:]


def fwd_bound(hs, wc, bc, wr, br, cheap=False):
    """Bound of the stacked output (M, 5A, 1, 1): compare ``stack_g(cls, reg)`` with it."""
    return LR.fwd_bound(rows(hs), stack(wc, wr), torch.cat([bc, br]), cheap=cheap)


def dgrad_bound(g_cls, g_reg, wc, wr, hs, cheap=False):
    """Bound of ``rows(dh)`` (M, C, 1, 1)."""
    return LR.dgrad_bound(stack_g(g_cls, g_reg), stack(wc, wr), None, rows(hs), cheap=cheap)


def wgrad_bound(hs, g_cls, g_reg, cheap=False):
    """Bound of the stacked weight gradient (5A, C, 1, 1): compare ``stack(dwc, dwr)`` with it."""
    return LR.wgrad_bound(rows(hs), stack_g(g_cls, g_reg), cheap=cheap)


def dbias_bound(g_cls, g_reg):
    """Bound of the stacked bias gradient (5A, 1, 1, 1)."""
    return LR.dbias_bound(stack_g(g_cls, g_reg))
