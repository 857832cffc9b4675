"""fp64 oracle of the shared-weight 3x3 conv over a pyramid (csrc/pyramid_conv.hip) and its a-priori
rounding bounds (test infrastructure; pure CPU, torch only).

Every level is an ordinary 3x3, stride-1, pad-1 convolution with the same weight, so the oracle is ``F.conv2d`` /
``F.conv_transpose2d`` / ``conv2d_weight`` in fp64 level by level, and the allowance is ``bound_util``'s unchanged:
``fwd_bound(pad=1, shift=bias, relu=...)`` and ``dgrad_bound(pad=1, mask_src=..., addend=..., mode='same')`` per level,
and for the shared weight gradient the per-level ``wgrad_bound`` combined into the bound of the level sum — v = sum of
v_l, S = sum of S_l, T = the total pixel count, the length of the longest chain of rounded additions any summation order
of all pixels can have.  The bias gradient is ``linear_ref.dbias_bound`` on the level-concatenated rows.  No tolerance is
invented here and no element is excluded.

Conventions.  A pyramid is a list of NHWC tensors: inputs ``xs[l]`` (B, H_l, W_l, Cin), outputs / cotangents ``ys[l]``
(B, H_l, W_l, Cout) — fp32 containers of 16-bit values; ``w`` (Cout, Cin, 3, 3) already rounded to the compute type
(``round16``), ``bias`` fp32.
"""
import torch
import torch.nn.functional as F

import bound_util as B
import linear_ref as LR

round16 = LR.round16


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def rows(ts):
    """list of (B, H_l, W_l, ch) -> the level-concatenated (sum of B*H_l*W_l, ch) matrix"""
    return torch.cat([t.reshape(-1, t.shape[-1]) for t in ts])


def fwd(xs, w, bias=None, relu=False):
    """-> ys list, fp64 NHWC"""
    out = []
    for x in xs:
        y = F.conv2d(nchw(x).double(), w.double(), None if bias is None else bias.double(), 1, 1)
        out.append(nhwc(y.clamp(min=0) if relu else y).contiguous())
    return out


def dgrad(gs, w, mask_src=None, addend=None):
    """-> dxs list, fp64 NHWC: conv3x3^T(g, w) (+ addend), zero where mask_src <= 0"""
    out = []
    for l, g in enumerate(gs):
        d = F.conv_transpose2d(nchw(g).double(), w.double(), None, 1, 1)
        if addend is not None and addend[l] is not None:
            d = d + nchw(addend[l]).double()
        if mask_src is not None and mask_src[l] is not None:
            d = d * (nchw(mask_src[l]) > 0).double()
        out.append(nhwc(d).contiguous())
    return out


def wgrad(xs, gs):
    """-> (dw (Cout, Cin, 3, 3), dbias (Cout,)), fp64, summed over the levels"""
    Cout, Cin = gs[0].shape[-1], xs[0].shape[-1]
    dw = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    db = torch.zeros(Cout, dtype=torch.float64)
    for x, g in zip(xs, gs):
        if x.numel():
            dw += torch.nn.grad.conv2d_weight(nchw(x).double(), (Cout, Cin, 3, 3), nchw(g).double(), 1, 1)
        db += g.double().sum((0, 1, 2))
    return dw, db


def fwd_bounds(xs, w, bias=None, relu=False):
    """One Bound per level (v is NCHW): compare the level's logical (B, Cout, H, W) output with it."""
    return [B.fwd_bound(nchw(x), w, pad=1, shift=bias, relu=relu) for x in xs]


def dgrad_bounds(gs, w, mask_src=None, addend=None):
    """One Bound per level (v is NCHW)."""
    out = []
    for l, g in enumerate(gs):
        a = None if addend is None or addend[l] is None else nchw(addend[l])
        m = None if mask_src is None or mask_src[l] is None else nchw(mask_src[l])
        out.append(B.dgrad_bound(nchw(g), w, (g.shape[1], g.shape[2]), pad=1, addend=a,
                                 mode="same" if a is not None else None, mask_src=m))
    return out


def wgrad_bound(xs, gs):
    """Bound of the shared weight gradient (Cout, Cin, 3, 3): the per-level bounds combined into the bound of the level
    sum, v = sum v_l, S = sum S_l, T = total pixel count."""
    Cout, Cin = gs[0].shape[-1], xs[0].shape[-1]
    v = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64)
    S = torch.zeros_like(v)
    T = 0
    for x, g in zip(xs, gs):
        if not x.numel():
            continue
        b = B.wgrad_bound(nchw(x), nchw(g), (Cout, Cin, 3, 3), pad=1)
        v, S, T = v + b.v, S + b.S, T + b.T
    return B.Bound(v, S, T, None, "S: exact, summed over the levels; v: fp64", activation=False)


def dbias_bound(gs):
    """Bound of the bias gradient (Cout, 1, 1, 1)."""
    return LR.dbias_bound(rows(gs))


def within(got, bound, out_dtype, what):
    """``assert_within`` on a result of the bound's shape (any float tensor, any strides); returns the record."""
    return B.assert_within(got.detach().float().cpu().reshape(bound.v.shape), bound, out_dtype, what)
