"""CPU oracle of CARAFE upsampling (the kernels are csrc/carafe.hip).  NumPy / torch CPU only.

The spec.  x (N, C, H, W), kernel size k (odd), r = (k - 1) / 2, groups g, scale s, masks (N, g k^2, sH, sW).  For the output
pixel (ph, pw), h = ph // s, w = pw // s, and channel c of group gi = c // (C / g):

    out[n, c, ph, pw] = sum over taps t = i k + j, in that order, of masks[n, gi k^2 + t, ph, pw] * x[n, c, h - r + i, w - r + j]

a tap whose source pixel lies outside the map is skipped; with ``out_size`` = (Ho, Wo) only the top-left crop exists, and
``addend`` (of the crop's shape) is added to the finished sum.  ``forward`` evaluates that in float32, one IEEE operation at a
time — multiply, then add (NumPy float32 ufuncs; nothing is fused) — and rounds once to 16 bits: reproducible bit for bit.

The normaliser.  The encoder output ``logits`` is (N, g k^2 s^2, H, W); the logit of tap t of group gi at the output pixel
(s h + dy, s w + dx) is channel (gi k^2 + t) s^2 + dy s + dx — ``F.pixel_shuffle``'s rule — and the masks are the softmax of
those k^2 logits (``normalize``).

Gradients (``Grads``, float64), gout the cotangent of out (zero outside the crop):

    dx[n, c, h, w]          = sum over source pixels (h2, w2), |h - h2| <= r, |w - w2| <= r, inside the map, and their s^2
                              sub-pixels, of gout[n, c, s h2 + dy, s w2 + dx] * masks[n, gi k^2 + (h - h2 + r) k + (w - w2 + r), ...]
    dmasks[n, gi k^2 + t]   = sum over the C / g channels of the group of gout * x[tap t]      (0 for a tap outside the map)
    dlogit_t                = p_t (dmask_t - sum_u p_u dmask_u)

Bounds.  Every device result is a sum of n terms formed and added in float32.  With one rounding of relative size
u <= 2^-23 per operation (bound_util.U), any order of summation gives |got - v| <= T * 2^-23 * S before the final store,
S the same sum over absolute values and T the number of rounded operations on the longest path:

    forward          n = k^2 terms m * x (1 multiplication), + 1 for the addend                T = k^2 + 1 (+ 1)
    dx               n = k^2 s^2 terms gout * m (1)                                             T = k^2 s^2 + 1
    dmasks           n = C / g terms gout * x (1)                                               T = C / g + 1
    softmax          p_t = exp(l_t - max) / sum_u exp(l_u - max):  the sum's k^2 additions, the two exps (the device's exp
                     is within a few ulp of the exact one: EXP_OPS = 4 operations' worth each, as §4p counts it), the
                     division, and the rounding of l_t - max, which the exp turns into a relative error of u |l_t - max|:
                     D = ceil(max |l_t - max|) operations' worth                                 SOFTMAX = k^2 + 2 EXP_OPS + 1 + D
                     — added to T wherever the weights come from logits
    dlogits          p_t (dm_t - dot), dot = sum_u p_u dm_u: dm (C / g + 1), p (SOFTMAX), the dot's k^2 additions and its
                     multiplication, the subtraction and the final multiplication, with
                     S = p_t (S_dm_t + sum_u p_u S_dm_u)                                        T = C / g + k^2 + 4 + SOFTMAX

and the store adds half an ulp of the 16-bit type at |v| + E (2^-24 |v| for a float32 store).  The bound is derived, not
fitted: if a kernel misses it, the kernel or this derivation is wrong.
"""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
EXP_OPS = 4


def round16(a, dtype):
    """float array -> float32 array of the values after one round-to-nearest-even to ``dtype`` (torch.bfloat16/float16)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def bits16(a, dtype):
    """float32 array of 16-bit-representable values -> their int16 bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).view(torch.int16).numpy()


def _crop(H, W, s, out_size):
    Ho, Wo = (H * s, W * s) if out_size is None else out_size
    assert H * s - s < Ho <= H * s and W * s - s < Wo <= W * s, (out_size, H, W, s)
    return Ho, Wo


def _shift(x, di, dj):
    """x[..., h + di, w + dj] with zeros outside, and the (H, W) mask of positions whose source lies inside the map"""
    H, W = x.shape[-2:]
    out = np.zeros_like(x)
    valid = np.zeros((H, W), dtype=bool)
    h_lo, h_hi, w_lo, w_hi = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
    if h_lo < h_hi and w_lo < w_hi:
        out[..., h_lo:h_hi, w_lo:w_hi] = x[..., h_lo + di:h_hi + di, w_lo + dj:w_hi + dj]
        valid[h_lo:h_hi, w_lo:w_hi] = True
    return out, valid


def _up(a, s):
    return a.repeat(s, axis=-2).repeat(s, axis=-1)


def normalize(logits, k, g, s, dt=np.float64):
    """``CARAFEPack.kernel_normalizer``: (N, g k^2 s^2, H, W) logits -> (N, g k^2, sH, sW) masks in ``dt``: the softmax over
    the k^2 taps, the maximum subtracted first, the sum in tap order."""
    l = np.asarray(logits).astype(dt)
    N, ch, H, W = l.shape
    k2, s2 = k * k, s * s
    assert ch == g * k2 * s2, (ch, g, k, s)
    l = l.reshape(N, g, k2, s, s, H, W).transpose(0, 1, 2, 5, 3, 6, 4).reshape(N, g, k2, H * s, W * s)
    e = np.exp((l - l.max(axis=2, keepdims=True)).astype(dt)).astype(dt)
    tot = np.zeros_like(e[:, :, 0])
    for t in range(k2):
        tot = (tot + e[:, :, t]).astype(dt)
    return (e / tot[:, :, None]).astype(dt).reshape(N, g * k2, H * s, W * s)


def unshuffle(dm, k, g, s):
    """(N, g k^2, sH, sW) -> (N, g k^2 s^2, H, W): the logits' channel rule, inverted"""
    N, ch, sH, sW = dm.shape
    H, W = sH // s, sW // s
    return dm.reshape(N, ch, H, s, W, s).transpose(0, 1, 3, 5, 2, 4).reshape(N, ch * s * s, H, W)


def _reassemble(x, masks, k, g, s, dt):
    """sum over taps in order in ``dt`` (float32: every operation one correctly rounded IEEE operation); -> (N, C, sH, sW)
    and, with ``dt`` float64, the same over absolute values"""
    x = np.asarray(x).astype(dt)
    m = np.asarray(masks).astype(dt)
    N, C, H, W = x.shape
    r, k2, Cg = (k - 1) // 2, k * k, C // g
    assert m.shape == (N, g * k2, H * s, W * s), (m.shape, x.shape, k, g, s)
    acc = np.zeros((N, C, H * s, W * s), dtype=dt)
    S = np.zeros_like(acc) if dt is np.float64 else None
    for i in range(k):
        for j in range(k):
            xs, valid = _shift(x, i - r, j - r)
            xs, valid = _up(xs, s), _up(valid, s)
            mt = m.reshape(N, g, k2, H * s, W * s)[:, :, i * k + j].repeat(Cg, axis=1)
            with np.errstate(invalid="ignore"):          # inf * 0 of a skipped tap
                prod = (mt * xs).astype(dt)
            acc = np.where(valid, (acc + prod).astype(dt), acc)
            if S is not None:
                S = np.where(valid, S + np.abs(prod), S)
    return acc, S


def forward(x, masks, k, g, s, dtype, out_size=None, addend=None):
    """The spec in float32, one operation at a time, rounded once to ``dtype``: float32 array (N, C, Ho, Wo)."""
    Ho, Wo = _crop(x.shape[2], x.shape[3], s, out_size)
    acc, _ = _reassemble(x, masks, k, g, s, f32)
    acc = acc[:, :, :Ho, :Wo]
    if addend is not None:
        acc = (np.asarray(addend, dtype=f32) + acc).astype(f32)
    return round16(acc, dtype)


def softmax_ops(logits, k, g, s):
    """SOFTMAX of the module docstring for these logits"""
    l = np.asarray(logits, dtype=np.float64)
    N, ch, H, W = l.shape
    l = l.reshape(N, g, k * k, s * s, H, W)
    D = float((l.max(axis=2, keepdims=True) - l).max())
    return k * k + 2 * EXP_OPS + 1 + int(np.ceil(D))


class Forward64(object):
    """float64: ``v`` (N, C, Ho, Wo), ``S`` and ``T`` of the bound, from masks or from logits"""

    def __init__(self, x, k, g, s, masks=None, logits=None, out_size=None, addend=None):
        assert (masks is None) != (logits is None)
        Ho, Wo = _crop(x.shape[2], x.shape[3], s, out_size)
        self.T = k * k + 1
        if logits is not None:
            masks = normalize(logits, k, g, s)
            self.T += softmax_ops(logits, k, g, s)
        v, S = _reassemble(x, masks, k, g, s, np.float64)
        self.v, self.S = v[:, :, :Ho, :Wo], S[:, :, :Ho, :Wo]
        if addend is not None:
            a = np.asarray(addend, dtype=np.float64)
            self.v, self.S, self.T = self.v + a, self.S + np.abs(a), self.T + 1


class Grads(object):
    """float64 gradients ``dx`` (N, C, H, W), ``dmasks`` (N, g k^2, sH, sW) and, from logits, ``dlogits``
    (N, g k^2 s^2, H, W), each with ``S_*`` and ``T_*`` of the bound.  ``gout``: (N, C, Ho, Wo)."""

    def __init__(self, x, gout, k, g, s, masks=None, logits=None):
        assert (masks is None) != (logits is None)
        x = np.asarray(x, dtype=np.float64)
        N, C, H, W = x.shape
        r, k2, Cg, sH, sW = (k - 1) // 2, k * k, C // g, H * s, W * s
        Ho, Wo = _crop(H, W, s, tuple(gout.shape[2:]))
        gf = np.zeros((N, C, sH, sW))
        gf[:, :, :Ho, :Wo] = np.asarray(gout, dtype=np.float64)
        soft = softmax_ops(logits, k, g, s) if logits is not None else 0
        m = (normalize(logits, k, g, s) if logits is not None else np.asarray(masks, dtype=np.float64))
        m = m.reshape(N, g, k2, sH, sW)
        self.dx, self.S_dx = np.zeros_like(x), np.zeros_like(x)
        dm, S_dm = np.zeros((N, g, k2, sH, sW)), np.zeros((N, g, k2, sH, sW))
        pool = lambda a: a.reshape(N, C, H, s, W, s).sum((3, 5))
        for i in range(k):
            for j in range(k):
                t = i * k + j
                xs, valid = _shift(x, i - r, j - r)
                prod = gf * _up(xs, s)
                dm[:, :, t] = prod.reshape(N, g, Cg, sH, sW).sum(2)
                S_dm[:, :, t] = np.abs(prod).reshape(N, g, Cg, sH, sW).sum(2)
                # dx[h2 - r + i, w2 - r + j] += sum over the sub-pixels of (h2, w2) of gout * m_t
                c = gf * m[:, :, t].repeat(Cg, axis=1)
                for src, dst in ((pool(c), self.dx), (pool(np.abs(c)), self.S_dx)):
                    sh, _ = _shift(src, r - i, r - j)
                    dst += sh
        self.T_dx = k2 * s * s + 1 + soft
        self.dmasks, self.S_dmasks, self.T_dmasks = dm.reshape(N, g * k2, sH, sW), S_dm.reshape(N, g * k2, sH, sW), Cg + 1
        if logits is not None:
            dot, S_dot = (m * dm).sum(2, keepdims=True), (m * S_dm).sum(2, keepdims=True)
            self.dlogits = unshuffle((m * (dm - dot)).reshape(N, g * k2, sH, sW), k, g, s)
            self.S_dlogits = unshuffle((m * (S_dm + S_dot)).reshape(N, g * k2, sH, sW), k, g, s)
            self.T_dlogits = Cg + k2 + 4 + soft


def allowance(v, S, T, dtype):
    """The bound of the module docstring for an element of exact value ``v``: E = T * 2^-23 * S, plus the store's half ulp
    (``dtype`` torch.bfloat16 / torch.float16) or 2^-24 |v| (torch.float32).  float64 arrays."""
    E = np.asarray(T, dtype=np.float64) * 2.0 ** -23 * S
    if dtype == torch.float32:
        return E + np.abs(v) * 2.0 ** -24
    p, emin = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    a = np.abs(v) + E
    _, ex = np.frexp(a)
    ex = np.maximum(np.where(a > 0, ex - 1, emin), emin)
    return E + np.ldexp(1.0, ex - p)


# ---- the torch composition (pins the oracle in test_carafe_oracle.py; the float64 autograd reference) -----------------
def carafe_autograd(x, masks, k, g, s, out_size=None, addend=None):
    """torch (any float dtype, differentiable): the same function through ``F.unfold`` and a nearest resize."""
    N, C, H, W = x.shape
    k2, Cg = k * k, C // g
    cols = F.unfold(x, k, padding=(k - 1) // 2).reshape(N, g, Cg, k2, H, W)
    cols = cols.repeat_interleave(s, dim=4).repeat_interleave(s, dim=5)
    out = (cols * masks.reshape(N, g, 1, k2, H * s, W * s)).sum(3).reshape(N, C, H * s, W * s)
    if out_size is not None:
        out = out[:, :, :out_size[0], :out_size[1]]
    return out if addend is None else addend + out


def normalize_autograd(logits, k, s):
    """torch: ``F.pixel_shuffle`` then the softmax over the k^2 taps of every group — mmdetection's kernel_normalizer"""
    m = F.pixel_shuffle(logits, s)
    N, ch, sH, sW = m.shape
    return F.softmax(m.reshape(N, ch // (k * k), k * k, sH, sW), dim=2).reshape(N, ch, sH, sW)


def carafe_pack_autograd(x, wc, bc, we, be, k, g, s, out_size=None, addend=None):
    """torch: ``CARAFEPack.forward`` composed from torch ops"""
    logits = F.conv2d(F.conv2d(x, wc, bc), we, be, padding=1)
    return carafe_autograd(x, normalize_autograd(logits, k, s), k, g, s, out_size, addend)
