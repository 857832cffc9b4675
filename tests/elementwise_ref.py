"""Oracle of the element-wise, pool, layout and pack kernels of csrc/elementwise.hip (test infrastructure; pure CPU,
torch only).

Every function takes the logical inputs of its ``ops`` wrapper — fp32 containers of 16-bit values, NCHW activations,
OIHW weights — and returns ``Ref(v, bits)`` (or a tuple of them):

  v     the answer in float64;
  bits  where the kernel is a FIXED chain of IEEE fp32 operations: that chain emulated in fp32 and rounded once to the
        element type ``dtype`` (torch.bfloat16 / torch.float16), as an fp32 container.  These are the expected bits:
        compare with ``assert_bits``.  Where the compiler may contract a multiply-add (channel_affine_fwd, the channel
        sums of channel_affine_bwd) there is no single chain: the function returns a ``bound_util.Bound`` instead and
        the comparison is ``bound_util.assert_within``.

Activations come back in the layout of the input (NCHW); the layout converters, ``stage_image`` and the packers come
back in the layout the kernel writes.  Rounding fp32 to the element type is torch's CPU ``.to(dtype)``: round to
nearest, ties to even, fp16 overflow to inf, gradual underflow.
"""
import collections

import torch

import bound_util as B

Ref = collections.namedtuple("Ref", "v bits")
# the pool adjoint also hands out its fp32 accumulator BEFORE the rounding to the element type: bits == r16(acc32)
PoolGrad = collections.namedtuple("PoolGrad", "v bits acc32")

TOP6 = {torch.bfloat16: 5.96875, torch.float16: 5.99609375}      # the largest element value under 6


def r16(t, dtype):
    """fp32 container of ``t`` rounded to ``dtype`` (round to nearest even)."""
    return t.detach().float().cpu().to(dtype).float()


def trunc16(t, dtype):
    """fp32 container of ``t`` rounded TOWARDS ZERO to ``dtype`` — what a truncating conversion would give (the teeth
    tests use it; finite values inside the type's normal range only)."""
    drop = {torch.bfloat16: 16, torch.float16: 13}[dtype]
    i = t.detach().float().cpu().contiguous().view(torch.int32)
    return ((i >> drop) << drop).view(torch.float32)


# ---- comparison ---------------------------------------------------------------------------------------------------
def _pattern(t):
    t = t.detach().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.float()                      # exact, keeps the sign of zero
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32), torch.isnan(t)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64), torch.isnan(t)
    return t.contiguous().long(), torch.zeros(t.shape, dtype=torch.bool)


def assert_bits(got, want, what="", nchw=False):
    """Bit-pattern comparison of two tensors of one shape (16-bit values may sit in fp32 containers on either side).
    NaN matches any NaN; -0.0 is not +0.0.  The failure names the first differing index in the tensors' own layout —
    as "(n, c, h, w)" when the caller says they are NCHW activations (``assert_nchw``) — and both values."""
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape),
                                                                                 tuple(want.shape))
    want = want.detach().cpu()
    got = got.detach().cpu()
    if want.dtype.is_floating_point != got.dtype.is_floating_point:
        raise AssertionError("%s: %s against %s" % (what, got.dtype, want.dtype))
    if want.dtype == torch.float64 or got.dtype == torch.float64:
        got, want = got.double(), want.double()
    pg, ng = _pattern(got)
    pw, nw = _pattern(want)
    bad = ((pg != pw) & ~(ng & nw)) | (ng != nw)
    nbad = int(bad.sum())
    if nbad:
        flat = int(torch.nonzero(bad.flatten())[0])
        idx = []
        for d in reversed(want.shape):
            idx.append(flat % d)
            flat //= d
        idx = tuple(reversed(idx))
        g, w = got[idx], want[idx]
        raise AssertionError("%s: %d of %d elements differ; first at %s = %s: got %r (0x%x), expected %r (0x%x)" %
                             (what, nbad, bad.numel(), "(n, c, h, w)" if nchw and want.dim() == 4 else "index", idx,
                              float(g), int(pg[idx]) & 0xffffffffffffffff, float(w), int(pw[idx]) & 0xffffffffffffffff))


def assert_nchw(got, want, what=""):
    """``assert_bits`` of two NCHW activations."""
    assert_bits(got, want, what, nchw=True)


# ---- max pool 3x3, stride 2, pad 1 --------------------------------------------------------------------------------
def pool_out(h):
    return (h - 1) // 2 + 1


def maxpool3x3s2_fwd(x, last_max=False):
    """-> (Ref of the values, window codes kh * 3 + kw as uint8).  The first maximum in (kh, kw) scan order wins; a
    NaN wins over anything and a later NaN replaces an earlier one; an all -inf window gives -inf at its first
    in-bounds position.  The values are selections, so ``bits`` is ``v`` in fp32.  ``last_max``: the WRONG rule (the
    last maximum wins), for the teeth tests."""
    x = x.detach().cpu()
    if x.dtype != torch.float64:
        x = x.float()                       # selections only: any type that holds the inputs gives the same answer
    N, C, H, W = x.shape
    Ho, Wo = pool_out(H), pool_out(W)
    xp = torch.zeros(N, C, H + 2, W + 2, dtype=x.dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    inb = torch.zeros(1, 1, H + 2, W + 2, dtype=torch.bool)
    inb[:, :, 1:H + 1, 1:W + 1] = True
    best = torch.full((N, C, Ho, Wo), float("-inf"), dtype=x.dtype)
    code = torch.full((N, C, Ho, Wo), -1, dtype=torch.int64)
    for kh in range(3):
        for kw in range(3):
            f = xp[:, :, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
            ok = inb[:, :, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
            take = ok & ((code < 0) | ((f >= best) if last_max else (f > best)) | torch.isnan(f))
            best = torch.where(take, f, best)
            code = torch.where(take, torch.full_like(code, kh * 3 + kw), code)
    return Ref(best.double(), best.float()), code.to(torch.uint8)


def maxpool3x3s2_bwd(dy, idx, in_hw, dtype, mask_src=None, pooled=None, descending=False, f64=True):
    """Adjoint of the pool: each input pixel sums the dy of the windows whose code points at it — in fp32, in
    ascending (ho, wo) order, starting from 0.f — then the ReLU mask (``mask_src`` > 0 at the pixel, or ``pooled`` > 0
    at the window), then one rounding.  ``descending``: the WRONG order, for the teeth tests.  ``f64=False`` skips the
    float64 answer (the large second-trip case)."""
    H, W = in_hw
    dy = dy.detach().cpu().float()
    idx = idx.detach().cpu().long()
    N, C, Ho, Wo = dy.shape
    live = torch.ones_like(idx, dtype=torch.bool) if pooled is None else pooled.detach().cpu() > 0
    acc = torch.zeros(N, C, H + 2, W + 2, dtype=torch.float32)
    a64 = torch.zeros(N, C, H + 2, W + 2, dtype=torch.float64) if f64 else None
    # a pixel's windows in ascending (ho, wo) are its positions in DESCENDING (kh, kw): ho = (h + 1 - kh) / 2
    order = [(kh, kw) for kh in (2, 1, 0) for kw in (2, 1, 0)]
    for kh, kw in (order[::-1] if descending else order):
        sel = (idx == kh * 3 + kw) & live
        hs, ws = slice(kh, kh + 2 * Ho - 1, 2), slice(kw, kw + 2 * Wo - 1, 2)
        acc[:, :, hs, ws] = torch.where(sel, acc[:, :, hs, ws] + dy, acc[:, :, hs, ws])
        if f64:
            a64[:, :, hs, ws] += torch.where(sel, dy.double(), torch.zeros((), dtype=torch.float64))
    acc = acc[:, :, 1:H + 1, 1:W + 1]
    if f64:
        a64 = a64[:, :, 1:H + 1, 1:W + 1]
    if mask_src is not None:
        m = mask_src.detach().cpu() > 0
        acc = torch.where(m, acc, torch.zeros((), dtype=torch.float32))
        if f64:
            a64 = torch.where(m, a64, torch.zeros((), dtype=torch.float64))
    return PoolGrad(a64, r16(acc, dtype), acc.contiguous())


# ---- stride-2 subsample, add, clamp, mask -------------------------------------------------------------------------
def subsample2_fwd(x):
    y = x.detach().cpu()[:, :, ::2, ::2].contiguous()
    return Ref(y.double(), y.float())


def subsample2_bwd(dy, in_hw, dtype, dx_in=None):
    """fl32(dx_in + dy) at the even / even positions (0.f + dy without dx_in), dx_in or 0 elsewhere; one rounding."""
    H, W = in_hw
    dy = dy.detach().cpu().float()
    N, C = dy.shape[:2]
    acc = torch.zeros(N, C, H, W, dtype=torch.float32) if dx_in is None else dx_in.detach().cpu().float().clone()
    a64 = acc.double()
    acc[:, :, ::2, ::2] = acc[:, :, ::2, ::2] + dy
    a64[:, :, ::2, ::2] += dy.double()
    return PoolGrad(a64, r16(acc, dtype), acc.contiguous())


def add_relu_mask(a, dtype, b=None, mask_src=None):
    """fl32(a + b), zeroed where mask_src <= 0, rounded once."""
    v = a.detach().cpu().float()
    v64 = v.double()
    if b is not None:
        v = v + b.detach().cpu().float()
        v64 = v64 + b.detach().cpu().double()
    if mask_src is not None:
        m = mask_src.detach().cpu() > 0
        v = torch.where(m, v, torch.zeros((), dtype=torch.float32))
        v64 = torch.where(m, v64, torch.zeros((), dtype=torch.float64))
    return Ref(v64, r16(v, dtype))


def clamp_max_(y, hi):
    """min(y, hi): a selection (finite inputs)."""
    y = y.detach().cpu().float()
    v = torch.where(y < hi, y, torch.full_like(y, hi))
    return Ref(v.double(), v)


def act_mask(g, y, hi=float("inf")):
    """g where 0 < y < hi, else +0: a selection."""
    g, y = g.detach().cpu().float(), y.detach().cpu().float()
    v = torch.where((y > 0) & (y < hi), g, torch.zeros((), dtype=torch.float32))
    return Ref(v.double(), v)


# ---- per-channel affine -------------------------------------------------------------------------------------------
def _c(t):
    return t.detach().cpu().double().view(1, -1, 1, 1)


def channel_affine_fwd(x, scale, shift, act, dtype):
    """act(x * scale[c] + shift[c]) -> (Bound, float64 pre-activation).  S = |x * scale| + |shift|, T = 2 (a multiply
    and an add, or one fma).  act 2 is the library's ReLU6 for a value about to be stored in ``dtype``: 6 from 6 up,
    and below 6 never more than the largest element value under 6 (``TOP6``), so that the backward mask 0 < y < 6 read
    from the stored output is the mask of the exact value."""
    xd = x.detach().cpu().double()
    pre = xd * _c(scale) + _c(shift)
    S = (xd * _c(scale)).abs() + _c(shift).abs()
    v = pre
    if act >= 1:
        v = v.clamp(min=0)
    if act == 2:
        v = torch.where(v >= 6, torch.full_like(v, 6.0), v.clamp(max=TOP6[dtype]))
    return B.Bound(v, S, 2, note="channel affine, act %d" % act), pre


def knee_resolved(got, b, pre, dtype):
    """The ReLU6 knee is a jump of one element ulp at 6: an element whose exact pre-activation lies within the Bound's
    E of 6 may legitimately be stored on either side.  Returns ``got`` (fp32, NCHW) with those elements replaced by
    the Bound's value WHERE they hold one of the two admissible values, and how many elements were undecided."""
    got = got.detach().cpu().double()
    und = (pre - 6).abs() <= b.E
    ok = und & ((got == 6.0) | (got == TOP6[dtype]))
    return torch.where(ok, b.v, got), int(und.sum())


def channel_affine_bwd(g, x, scale, mean, invstd, dtype):
    """-> (Ref dx, Bound dbeta, Bound dgamma, float64 per-channel sum of g * (x - mean)).
    dx = fl16(fl32(g * scale)): one fp32 multiply, one rounding to the element type.
    dbeta[c] = sum_p g, dgamma[c] = invstd[c] * sum_p g * (x - mean[c]) in float64; S per channel on absolute values,
    T = npix + 2 (the subtraction, the multiply-add chain over the pixels, the final multiply)."""
    gd, xd = g.detach().cpu().double(), x.detach().cpu().double()
    npix = gd.shape[0] * gd.shape[2] * gd.shape[3]
    dx32 = g.detach().cpu().float() * scale.detach().cpu().float().view(1, -1, 1, 1)
    dx = Ref(gd * _c(scale), r16(dx32, dtype))
    s1 = (gd * (xd - _c(mean))).sum((0, 2, 3))
    inv = invstd.detach().cpu().double()
    db = B.Bound(gd.sum((0, 2, 3)), gd.abs().sum((0, 2, 3)), npix + 2, note="dbeta", activation=False)
    dg = B.Bound(s1 * inv, (gd.abs() * (xd.abs() + _c(mean).abs())).sum((0, 2, 3)) * inv.abs(), npix + 2,
                 note="dgamma", activation=False)
    return dx, db, dg, s1


# ---- layouts ------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, dtype):
    """NCHW (fp32, or 16-bit: then a pure move) -> NHWC in ``dtype``."""
    y = x.detach().cpu().permute(0, 2, 3, 1).contiguous()
    return Ref(y.double(), r16(y, dtype))


def nhwc_to_nchw_f32(x):
    """NHWC 16-bit -> NCHW fp32: exact."""
    y = x.detach().cpu().float().permute(0, 3, 1, 2).contiguous()
    return Ref(y.double(), y)


def stage_image(img, dtype):
    """NCHW fp32 (N, 3, H, W) -> zero-padded NHWC4 (N, H + 6, W + 8, 4): the image at rows 3.., columns 3.., channel 3
    and the halo +0."""
    img = img.detach().cpu().float()
    N, _, H, W = img.shape
    v = torch.zeros(N, H + 6, W + 8, 4, dtype=torch.float64)
    v[:, 3:3 + H, 3:3 + W, :3] = img.permute(0, 2, 3, 1).double()
    return Ref(v, r16(v.float(), dtype))        # .float() of the fp64 copy of fp32 values is exact


def _dgrad_chain(w, scale, dtype):
    """fl16(fl32(fl16(w) * scale[co])), OIHW, and the same product in float64."""
    w16 = r16(w, dtype)
    if scale is None:
        return w16.double(), w16
    s = scale.detach().cpu().float().view(-1, 1, 1, 1)
    return w16.double() * s.double(), r16(w16 * s, dtype)


def pack_conv_weight(w, dtype, scale=None):
    """OIHW fp32 -> (w_fwd [O][kh][kw][I], w_dgrad [I][kh][kw][O] = fl16(fl32(fl16(w) * scale[o])))."""
    w = w.detach().cpu().float()
    d64, d16 = _dgrad_chain(w, scale, dtype)
    return (Ref(w.double().permute(0, 2, 3, 1).contiguous(), r16(w, dtype).permute(0, 2, 3, 1).contiguous()),
            Ref(d64.permute(1, 2, 3, 0).contiguous(), d16.permute(1, 2, 3, 0).contiguous()))


def pack_gconv_weight(w, groups, dtype, scale=None):
    """Grouped weight [C][cpg][kh][kw] -> block-diagonal operands [C][kh][kw][64] (elementwise.hip):
        w_fwd[co][tap][j]   = w[co][j % cpg][tap]                 if input slot j (channel 64*(co/64) + j) is in co's group
        w_dgrad[ci][tap][j] = scale[co'] * w[co'][ci % cpg][tap]  with co' = 64*(ci/64) + j, if co' is in ci's group
    zeros (+0) elsewhere."""
    w = w.detach().cpu().float()
    C, cpg, kh, kw = w.shape
    assert cpg * groups == C and C % 64 == 0 and 64 % cpg == 0
    d64, d16 = _dgrad_chain(w, scale, dtype)
    c = torch.arange(C).view(C, 1)
    j = torch.arange(64).view(1, 64)
    same = ((j // cpg) == ((c % 64) // cpg)).view(C, 64, 1, 1)
    co = (c // 64) * 64 + j

    def blocks(src_fwd, src_dg, zero):
        f = torch.where(same, src_fwd[c.expand(C, 64), (j % cpg).expand(C, 64)], zero)
        d = torch.where(same, src_dg[co, (c % cpg).expand(C, 64)], zero)
        return f.permute(0, 2, 3, 1).contiguous(), d.permute(0, 2, 3, 1).contiguous()

    f64, g64 = blocks(w.double(), d64, torch.zeros((), dtype=torch.float64))
    f16, g16 = blocks(r16(w, dtype), d16, torch.zeros((), dtype=torch.float32))
    return Ref(f64, f16), Ref(g64, g16)


def pack_stem_weight(w, dtype):
    """[Cout][3][7][7] -> [co][kh][kw padded to 8][c padded to 4], zero (+0) padding."""
    w = w.detach().cpu().float()
    O = w.shape[0]
    v = torch.zeros(O, 7, 8, 4, dtype=torch.float64)
    v[:, :, :7, :3] = w.permute(0, 2, 3, 1).double()
    return Ref(v, r16(v.float(), dtype))
