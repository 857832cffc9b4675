"""fp64 oracle of the fully connected layers (csrc/linear.hip) and their a-priori rounding bounds
(test infrastructure; pure CPU, torch only).

Conventions.  ``x`` is the (M, K) operand IN MEMORY ORDER (what the kernel reads): for a channels_last (R, S, S, C) RoI
buffer that is the packed column order p * C + c.  ``w`` is the (O, K) weight in the parameter's LOGICAL column order
c * hw + p, already rounded to the 16-bit compute type (``round16``).  ``C=None`` (or K) means the two orders coincide.
The permutation is written as ``w.view(O, C, hw).permute(0, 2, 1)``.

A linear layer is a 1x1 conv on an (M, K, 1, 1) tensor, so the allowance is ``bound_util``'s: ``fwd_bound``,
``dgrad_bound`` and ``wgrad_bound`` on 4-D views, checked with ``assert_within``; every element takes part.
"""
import torch

import bound_util as B


def round16(t, dtype):
    """fp32 container of ``t`` rounded to ``dtype``."""
    return t.detach().float().cpu().to(dtype).float()


def pack_w(w, C=None):
    """(O, K) logical -> (O, K) in the memory order of the activations."""
    O, K = w.shape
    if C is None or C == K:
        return w
    hw = K // C
    return w.view(O, C, hw).permute(0, 2, 1).reshape(O, K)


def unpack_w(wp, C=None):
    """inverse of ``pack_w``: (O, K) in memory order -> logical."""
    O, K = wp.shape
    if C is None or C == K:
        return wp
    hw = K // C
    return wp.view(O, hw, C).permute(0, 2, 1).reshape(O, K)


def fwd(x, w, b=None, relu=False, C=None):
    y = x.double() @ pack_w(w, C).double().T
    if b is not None:
        y = y + b.double()
    return y.clamp(min=0) if relu else y


def dgrad(g, w, C=None, mask_src=None):
    dx = g.double() @ pack_w(w, C).double()
    if mask_src is not None:
        dx = dx * (mask_src > 0).double()
    return dx


def wgrad(x, g, C=None):
    """-> (dw in LOGICAL order, dbias)."""
    return unpack_w(g.double().T @ x.double(), C), g.double().sum(0)


def _x4(t):
    return t.detach().float().cpu().reshape(t.shape[0], t.shape[1], 1, 1)


def fwd_bound(x, w, b=None, relu=False, C=None, cheap=False):
    """Bound of y (M, O, 1, 1)."""
    return B.fwd_bound(_x4(x), _x4(pack_w(w, C)), shift=b, relu=relu, cheap=cheap)


def dgrad_bound(g, w, C=None, mask_src=None, cheap=False):
    """Bound of dx (M, K, 1, 1), memory order."""
    return B.dgrad_bound(_x4(g), _x4(pack_w(w, C)), (1, 1), mask_src=None if mask_src is None else _x4(mask_src),
                         cheap=cheap)


def wgrad_bound(x, g, cheap=False, mult=1.0):
    """Bound of dw (O, K, 1, 1) in MEMORY order: compare ``pack_w(dw_gpu, C)`` with it."""
    return B.wgrad_bound(_x4(x), _x4(g), (g.shape[1], x.shape[1], 1, 1), cheap=cheap, mult=mult)


def dbias_bound(g, mult=1.0):
    """Bound of dbias (O, 1, 1, 1): the weight gradient against a column of ones."""
    return B.wgrad_bound(torch.ones(g.shape[0], 1, 1, 1), _x4(g), (g.shape[1], 1, 1, 1), mult=mult)


def within(got, bound, out_dtype, what):
    """``assert_within`` on a 2-D (or 1-D) result; returns the record."""
    return B.assert_within(got.detach().float().cpu().reshape(bound.v.shape), bound, out_dtype, what)
