"""A-priori, per-element rounding bound for one fused conv-family launch, and the checker that applies it
(test infrastructure; pure CPU, torch only).

The operands of a launch are exactly representable 16-bit values (plus fp32 scale / shift vectors).  Let ``v`` be the
exact real-valued result of the launch — conv, then the optional scale, shift or bias, then the optional addend, then
the optional ReLU or mask — evaluated here in fp64.  Any evaluation that forms the same products and adds them in
SOME order with one rounding of relative size ``u`` per operation satisfies, before its final store,

    |v_gpu - v| <= E = (T * u) * S

  S  the same expression on absolute values: conv(|x|, |w|) * |scale| + |shift| + |addend terms| (a mask or ReLU can
     only shrink it, so it is left out);
  T  the number of rounded operations on the longest path: the K-term count (Cin_per_group * kh * kw forward,
     Cout_per_group * kh * kw for the input gradient — the full tap count even at stride 2 —, N * Ho * Wo for a weight
     gradient) plus the epilogue operations of EPI_OPS;
  u  = 2^-23.  The 16-bit products are exact in fp32 (8 x 8 or 11 x 11 significand bits).  What is NOT documented
     anywhere in this repository or its guides is the internal rounding of the bf16 / fp16 MFMA accumulate: only the
     f32-input MFMA is described (a round-to-nearest fmaf chain, u = 2^-24).  2^-23 is the unit roundoff of a
     TRUNCATING fp32 accumulate, which covers both.  It is a derived constant, not a tuned one.

The stored value then obeys

    fp32 output:    |got - v| <= E + 2^-24 * |v|
    16-bit output:  |got - v| <= E + half_ulp16(|v| + E)

with the exact half-ulp of the storage type (bf16: 8 significand bits; fp16: 11 and a subnormal floor).  The comparison
is against the UNROUNDED v, so a legitimate flip to the neighbouring 16-bit value is inside the bound by construction.
No element is excluded: the checker has no outlier fraction.

Cheaper variants, all provable and all stated in the record a check returns:
  * S may be replaced by the Cauchy-Schwarz bound sqrt(box_k(sum_c x^2)) * sqrt(sum w^2 per output channel) >= S
    (``cheap=True``): no second convolution.
  * v may come from an fp32 CPU convolution (``conv32=``): its own error K * 2^-24 * S_conv * |scale| is then added to
    the allowance as ``R`` (the epilogue on top of that convolution is still evaluated in fp64).
  * an operand that is itself one CPU launch deep (the downsample residual the HIP path does not save) differs from
    the GPU's by at most its own E (+ R) and two roundings to 16 bits: ``operand_slack`` returns that term.

A worst-case bound has slack: rounding errors add like sqrt(K), the bound like K, so at K = 2304 an element may be off
by several bf16 ulps before it is seen.  What the bound cannot miss is what a norm hides: ONE element that is wrong by
a visible fraction of its own magnitude.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -23        # per-operation unit roundoff granted to the GPU (see module docstring)
U32 = 2.0 ** -24      # round-to-nearest fp32: the CPU reference's own operations, and the final fp32 store
EPI_OPS = {"scale": 1, "shift": 1, "same": 1, "sumpool": 4, "up2x": 1, None: 0}


def half_ulp16(a, dtype):
    """Half the spacing of ``dtype`` (torch.bfloat16 / torch.float16) at magnitude |a|: the largest error of a
    round-to-nearest store of a value of that magnitude.  fp64 tensor in, fp64 tensor out."""
    p, emin = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    a = a.double().abs()
    _, ex = torch.frexp(a)                                   # a = m * 2^ex, 0.5 <= m < 1
    e = torch.where(a > 0, ex - 1, torch.full_like(ex, emin)).clamp_(min=emin)
    return torch.ldexp(torch.ones_like(a), e - p)


class Bound(object):
    """v: the exact value (fp64, or fp32-derived with R > 0); E = T * U * S; R: the reference's own error bound."""

    def __init__(self, v, S, T, R=None, note="", activation=True):
        self.v, self.S, self.T = v, S, T
        self.E = S * (T * U)
        self.R = R
        self.note = note
        self.activation = activation      # NCHW activation (border classification applies); False: OIHW weights

    def slack(self):
        return self.E if self.R is None else self.E + self.R


def _vec(t, ndim=4):
    return None if t is None else t.detach().double().cpu().view(1, -1, *([1] * (ndim - 2)))


def _ksum_w(w):
    return w.double().pow(2).sum((1, 2, 3)).sqrt()


def fwd_bound(x, w, stride=1, pad=0, scale=None, shift=None, addend=None, mode=None, relu=False, dilation=1, groups=1,
              cheap=False, conv32=None):
    """Forward launch.  x: NCHW, w: OIHW (fp32 containers of 16-bit values), scale / shift: fp32 vectors or None,
    addend with mode 'same' or 'up2x'.  ``cheap``: Cauchy-Schwarz S; ``conv32``: an fp32 F.conv2d(x, w) to take v from
    (True: compute it here)."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    T = K + (scale is not None) * EPI_OPS["scale"] + (shift is not None) * EPI_OPS["shift"] + \
        (EPI_OPS[mode] if addend is not None else 0)
    if conv32 is True:
        conv32 = F.conv2d(x, w, None, stride, pad, dilation, groups)
    if conv32 is not None:
        c = conv32.double()
    else:
        c = F.conv2d(x.double(), w.double(), None, stride, pad, dilation, groups)
    if cheap:
        assert groups == 1
        ones = torch.ones(1, 1, w.shape[2], w.shape[3], dtype=torch.float64)
        box = F.conv2d(x.double().pow(2).sum(1, keepdim=True), ones, None, stride, pad, dilation)
        Sc = box.clamp_(min=0).sqrt_() * _ksum_w(w).view(1, -1, 1, 1)
    else:
        Sc = F.conv2d(x.double().abs(), w.double().abs(), None, stride, pad, dilation, groups)
    sc, sh = _vec(scale), _vec(shift)
    if sc is not None:
        c = c * sc
        Sc = Sc * sc.abs()
    R = Sc * (K * U32) if conv32 is not None else None
    S = Sc
    if sh is not None:
        c = c + sh
        S = S + sh.abs()
    if addend is not None:
        a = addend.double()
        if mode == "up2x":
            a = F.interpolate(a, scale_factor=2, mode="nearest")
        else:
            assert mode == "same", mode
        c = c + a
        S = S + a.abs()
    if relu:
        c = c.clamp_(min=0)
    return Bound(c, S, T, R, "S: %s; v: %s" % ("Cauchy-Schwarz" if cheap else "exact",
                                               "fp32 conv + K*2^-24*S" if conv32 is not None else "fp64"))


def dgrad_bound(g, w_eff, in_hw, stride=1, pad=0, addend=None, mode=None, mask_src=None, dilation=1, groups=1,
                cheap=False, conv32=None):
    """Input-gradient launch.  g: NCHW cotangent, w_eff: OIHW weights of the forward conv as the launch reads them
    (scale folded, rounded to 16 bits); addend with mode 'same' or 'sumpool' (2x2 sum of a finer tensor);
    mask_src: the result is zeroed where mask_src <= 0.  ``conv32``: an fp32 conv_transpose2d result, or True."""
    H, W = in_hw
    k = w_eff.shape[2]
    op = (H - ((g.shape[2] - 1) * stride - 2 * pad + dilation * (k - 1) + 1),
          W - ((g.shape[3] - 1) * stride - 2 * pad + dilation * (k - 1) + 1))
    K = (w_eff.shape[0] // groups) * k * w_eff.shape[3]
    T = K + (EPI_OPS[mode] if addend is not None else 0)
    if conv32 is True:
        conv32 = F.conv_transpose2d(g, w_eff, None, stride, pad, op, groups, dilation)
    if conv32 is not None:
        c = conv32.double()
    else:
        c = F.conv_transpose2d(g.double(), w_eff.double(), None, stride, pad, op, groups, dilation)
    if cheap:
        assert groups == 1
        ones = torch.ones(1, 1, k, w_eff.shape[3], dtype=torch.float64)
        box = F.conv_transpose2d(g.double().pow(2).sum(1, keepdim=True), ones, None, stride, pad, op, 1, dilation)
        Sc = box.clamp_(min=0).sqrt_() * w_eff.double().pow(2).sum((0, 2, 3)).sqrt().view(1, -1, 1, 1)
    else:
        Sc = F.conv_transpose2d(g.double().abs(), w_eff.double().abs(), None, stride, pad, op, groups, dilation)
    R = Sc * (K * U32) if conv32 is not None else None
    S = Sc
    if addend is not None:
        a = addend.double()
        if mode == "sumpool":
            S = S + F.avg_pool2d(a.abs(), 2) * 4.0
            a = F.avg_pool2d(a, 2) * 4.0        # four exactly representable terms: exact in fp64
        else:
            assert mode == "same", mode
            S = S + a.abs()
        c = c + a
    if mask_src is not None:
        c = c * (mask_src > 0).double()
    return Bound(c, S, T, R, "S: %s; v: %s" % ("Cauchy-Schwarz" if cheap else "exact",
                                               "fp32 conv + K*2^-24*S" if conv32 is not None else "fp64"))


def wgrad_bound(x, g, wshape, stride=1, pad=0, scale=None, dilation=1, groups=1, cheap=False, mult=1.0,
                G32=None):
    """Weight gradient dw (OIHW, fp32 output): K = N * Ho * Wo terms per element, times |scale| for a BN-folded member
    (one more operation); ``mult``: an exact factor (the doubled result of an accumulate call).  ``cheap``: v from the
    fp32 conv2d_weight (``G32`` if the caller has it; its error K * 2^-24 * S added as R) and S <= ||x_c|| * ||g_o|| (Cauchy-Schwarz over pixels)."""
    K = g.shape[0] * g.shape[2] * g.shape[3]
    T = K + (scale is not None) * EPI_OPS["scale"]
    cw = torch.nn.grad.conv2d_weight
    if cheap:
        assert groups == 1
        c = (cw(x, wshape, g, stride, pad, dilation, groups) if G32 is None else G32).double()
        Sc = g.double().pow(2).sum((0, 2, 3)).sqrt().view(-1, 1, 1, 1) * \
            x.double().pow(2).sum((0, 2, 3)).sqrt().view(1, -1, 1, 1) * torch.ones(wshape, dtype=torch.float64)
    else:
        c = cw(x.double(), wshape, g.double(), stride, pad, dilation, groups)
        Sc = cw(x.double().abs(), wshape, g.double().abs(), stride, pad, dilation, groups)
    if scale is not None:
        sc = scale.detach().double().cpu().view(-1, 1, 1, 1)
        c, Sc = c * sc, Sc * sc.abs()
    R = Sc * (K * U32 * mult) if cheap else None
    note = "S: %s; v: %s" % ("Cauchy-Schwarz" if cheap else "exact",
                             "fp32 conv2d_weight + K*2^-24*S" if cheap else "fp64")
    return Bound(c * mult, Sc * mult, T, R, note, activation=False)


def operand_slack(b, dtype):
    """How far the GPU's own 16-bit value of an operand may lie from the CPU's 16-bit value of it, when both are one
    launch deep on identical inputs and ``b`` is that launch's Bound: each is within E (+ R for an fp32 reference) of
    v before its store, and each store moves it by at most half an ulp16 — E + R + one ulp16 in all.  The CPU's value
    is rounded from fp64 through fp32 to 16 bits: the extra rounding adds 2^-24 |v|."""
    s = b.slack() + b.v.abs() * U32
    return s + 2.0 * half_ulp16(b.v.abs() + s, dtype)


def where_of(index, shape):
    """Border classification of an (n, c, h, w) element of an NCHW activation."""
    n, _, h, w = index
    N, _, H, W = shape
    tags = []
    if h == 0 or w == 0 or h == H - 1 or w == W - 1:
        tags.append("image border")
    if (h == 0 and w == 0 and n > 0) or (h == H - 1 and w == W - 1 and n < N - 1):
        tags.append("image boundary in M")
    if h == H - 1:
        tags.append("last row")
    if w == W - 1:
        tags.append("last column")
    return ", ".join(tags) if tags else "interior"


def check(got, b, out_dtype, extra=None, what=""):
    """Compares ``got`` (any float tensor shaped like b.v; NCHW for activations, OIHW for weights) with the bound.
    Returns {"ratio": worst |got - v| / allowance, "index": its (n, c, h, w), "where": border classification,
    "err", "allowance", "got", "v", "T", "note"}.  Every element takes part."""
    v = b.v
    assert tuple(got.shape) == tuple(v.shape), (tuple(got.shape), tuple(v.shape))
    tot = b.slack()
    if extra is not None:
        tot = tot + extra
    if out_dtype == torch.float32:
        allow = tot + v.abs() * U32
    else:
        allow = tot + half_ulp16(v.abs() + tot, out_dtype)
    err = (got.detach().double().cpu() - v).abs_()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = torch.where(allow > 0, err / allow, torch.where(err > 0, torch.full_like(err, float("inf")),
                                                            torch.zeros_like(err)))
    flat = int(ratio.argmax())
    idx = []
    for d in reversed(v.shape):
        idx.append(flat % d)
        flat //= d
    idx = tuple(reversed(idx))
    note = b.note + ("; operand slack added" if extra is not None else "")
    where = where_of(idx, v.shape) if b.activation and v.dim() == 4 else "weights"
    return {"ratio": float(ratio[idx]), "index": list(idx), "where": where, "err": float(err[idx]),
            "allowance": float(allow[idx]), "got": float(got[idx]), "v": float(v[idx]), "T": int(b.T), "note": note,
            "what": what}


def message(r):
    return ("%s: element (n, c, h, w) = %s [%s] is off by %.6g, %.3f x its allowance %.6g (got %.9g, exact %.9g; "
            "T = %d; %s)" % (r["what"], tuple(r["index"]), r["where"], r["err"], r["ratio"], r["allowance"], r["got"],
                             r["v"], r["T"], r["note"]))


def assert_within(got, b, out_dtype, what="", extra=None):
    """check() and assert worst ratio <= 1; the failure message names the element.  Returns the record."""
    r = check(got, b, out_dtype, extra, what)
    assert r["ratio"] <= 1.0, message(r)
    return r
