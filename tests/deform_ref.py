"""CPU oracle of deformable convolution (the kernels are csrc/deform.hip).  NumPy / torch CPU only.

The spec, per output pixel (ho, wo), tap k = 3 i + j, deformable group g, in float32, one IEEE operation at a time:

    py = float(ho * stride - pad + i * dil) + dy          px alike          (dil == pad)
    valid = py > -1 and py < H and px > -1 and px < W     (on the floats: NaN and +-inf are invalid)
    y0 = floor(py), ly = py - y0, hy = 1 - ly             x alike
    w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx
    val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4       corners (y0, x0), (y0, x1), (y1, x0), (y1, x1); a corner outside
                                                          the map is 0; an invalid sample is 0
    val = val * m                                          with a mask (m = 1 / (1 + exp(-logit)) for a logit)
    col = round_to_nearest_even_16(val)

``sample`` evaluates exactly that with NumPy float32 arrays (every NumPy float32 ufunc is one correctly rounded IEEE
operation, and nothing here is fused), so its result is reproducible bit for bit.  ``Positions`` holds the float32 sample
positions of the spec; the float64 functions start from THOSE positions (their rounding is part of the spec) and carry on
exactly.

Bounds.  A gradient element is a sum of n terms; the kernels form each term with a fixed number of float32 operations and
add the terms in float32.  With one rounding of relative size u <= 2^-23 per operation (bound_util.U), any order of
summation gives |got - v| <= T * 2^-23 * S before the final store, S the same sum over absolute values and T the number
of rounded operations on the longest path: the n additions plus the operations that form one term,

    dx       term  (dcol * m) * (wy * wx), wy, wx each 1 - l or l          5 operations             T = n + 5
    doffset  term  dcol * ((v3 - v1) * hx + (v4 - v2) * lx), hx = 1 - lx;  7, and the final * m     T = Cg + 8
    dmask    term  dcol * val, val = 7 operations, 2 for hy, hx            10                        T = Cg + 10
    logit    the device's exp is within a few ulp of the exact one: 8 more operations' worth for everything m enters,
             and dlogit = dmask * (t / ((1 + t) * (1 + t))), t = exp(-|logit|) — the form of s (1 - s) that does not
             cancel for a saturated sigmoid —: 6 more (the exp counted twice)

and the store adds half an ulp of the 16-bit type (bound_util.check: half_ulp16(|v| + E); 2^-24 |v| for a float32 store).
"""
import numpy as np
import torch

OPS_DX, OPS_DOFF, OPS_DMASK, OPS_LOGIT = 5, 8, 10, 8

f32 = np.float32


def out_size(H, stride, pad):
    """3x3, dilation == pad: (H + 2 pad - (2 pad + 1)) // stride + 1"""
    return (H - 1) // stride + 1


def round16(a, dtype):
    """float array -> float32 array of the values after one round-to-nearest-even to ``dtype`` (torch.bfloat16/float16)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).float().numpy()


def bits16(a, dtype):
    """float32 array of 16-bit-representable values -> their int16 bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).view(torch.int16).numpy()


class Positions(object):
    """The float32 sample positions and what the spec derives from them, arrays of shape (N, dg, 9, Ho, Wo):
    ``py, px, valid``, int ``y0, x0`` (0 where invalid) and float32 ``ly, lx, hy, hx`` (0 where invalid)."""

    def __init__(self, offset, H, W, stride, pad, dg):
        offset = np.asarray(offset, dtype=f32)
        N, ch, Ho, Wo = offset.shape
        assert ch == 18 * dg and Ho == out_size(H, stride, pad) and Wo == out_size(W, stride, pad), offset.shape
        off = offset.reshape(N, dg, 9, 2, Ho, Wo)
        k = np.arange(9)
        by = (np.arange(Ho)[None, :, None] * stride - pad + (k // 3)[:, None, None] * pad).astype(f32)   # (9, Ho, 1)
        bx = (np.arange(Wo)[None, None, :] * stride - pad + (k % 3)[:, None, None] * pad).astype(f32)    # (9, 1, Wo)
        with np.errstate(invalid="ignore", over="ignore"):
            self.py = (by + off[:, :, :, 0]).astype(f32)
            self.px = (bx + off[:, :, :, 1]).astype(f32)
            self.valid = (self.py > f32(-1)) & (self.py < f32(H)) & (self.px > f32(-1)) & (self.px < f32(W))
        py = np.where(self.valid, self.py, f32(0))
        px = np.where(self.valid, self.px, f32(0))
        fy, fx = np.floor(py), np.floor(px)
        self.y0, self.x0 = fy.astype(np.int64), fx.astype(np.int64)
        zero = lambda a: np.where(self.valid, a, f32(0)).astype(f32)
        self.ly, self.lx = zero(py - fy), zero(px - fx)
        self.hy, self.hx = zero(f32(1) - self.ly), zero(f32(1) - self.lx)
        self.N, self.dg, self.Ho, self.Wo, self.H, self.W = N, dg, Ho, Wo, H, W

    def corners(self):
        """[(y, x, inside)] * 4 in the spec's order; y, x clipped into the map, ``inside`` False for a corner outside it
        or an invalid sample"""
        out = []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            y, x = self.y0 + dy, self.x0 + dx
            inside = self.valid & (y >= 0) & (y < self.H) & (x >= 0) & (x < self.W)
            out.append((np.clip(y, 0, self.H - 1), np.clip(x, 0, self.W - 1), inside))
        return out

    def in_range_share(self):
        return float(self.valid.mean())


def mask_values(mask, dg, logit, dt):
    """(N, dg, 9, Ho, Wo) mask weights in ``dt`` (float32: the spec's operations; float64: exact), or None"""
    if mask is None:
        return None
    m = np.asarray(mask, dtype=f32)
    N, ch, Ho, Wo = m.shape
    assert ch == 9 * dg
    m = m.reshape(N, dg, 9, Ho, Wo).astype(dt)
    if logit:
        with np.errstate(over="ignore"):
            m = (dt(1) / (dt(1) + np.exp(-m))).astype(dt)
    return m


def _gather(x, P, dt):
    """v1..v4 of every channel: arrays (N, dg, Cg, 9, Ho, Wo) in ``dt``, zeros for corners outside"""
    N, C, H, W = x.shape
    Cg = C // P.dg
    xg = np.asarray(x, dtype=dt).reshape(N, P.dg, Cg, H, W)
    n = np.arange(N)[:, None, None, None, None, None]
    g = np.arange(P.dg)[None, :, None, None, None, None]
    c = np.arange(Cg)[None, None, :, None, None, None]
    vs = []
    for y, xx, inside in P.corners():
        v = xg[n, g, c, y[:, :, None], xx[:, :, None]]
        vs.append(np.where(inside[:, :, None], v, dt(0)).astype(dt))
    return vs


def _cols_layout(v):
    """(N, dg, Cg, 9, Ho, Wo) -> (N, Ho, Wo, 9, C)"""
    N, dg, Cg, K, Ho, Wo = v.shape
    return np.ascontiguousarray(v.transpose(0, 4, 5, 3, 1, 2).reshape(N, Ho, Wo, K, dg * Cg))


def _from_cols(d, dg):
    """(N, Ho, Wo, 9, C) -> (N, dg, Cg, 9, Ho, Wo)"""
    N, Ho, Wo, K, C = d.shape
    return d.reshape(N, Ho, Wo, K, dg, C // dg).transpose(0, 4, 5, 3, 1, 2)


def sample(x, offset, mask=None, stride=1, pad=1, dg=1, dtype=torch.bfloat16, mask_is_logit=False, positions=None):
    """cols (N, Ho, Wo, 9, C): float32 array holding the 16-bit values the spec gives.  ``x`` (N, C, H, W) float array of
    16-bit-representable values, ``offset`` (N, 18 dg, Ho, Wo), ``mask`` (N, 9 dg, Ho, Wo) or None."""
    N, C, H, W = x.shape
    P = positions or Positions(offset, H, W, stride, pad, dg)
    v1, v2, v3, v4 = _gather(x, P, f32)
    e = lambda a: a[:, :, None]
    w1, w2, w3, w4 = e(P.hy * P.hx), e(P.hy * P.lx), e(P.ly * P.hx), e(P.ly * P.lx)
    val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4
    assert val.dtype == f32
    if mask is not None:
        val = val * e(mask_values(mask, dg, mask_is_logit, f32))
    val = np.where(e(P.valid), val, f32(0)).astype(f32)
    return round16(_cols_layout(val), dtype)


def sample64(x, P, m64=None):
    """The exact (float64) sample values from the spec's positions, NOT rounded: (N, Ho, Wo, 9, C)"""
    v1, v2, v3, v4 = _gather(x, P, np.float64)
    e = lambda a: a.astype(np.float64)[:, :, None]
    val = e(P.hy64 * P.hx64) * v1 + e(P.hy64 * P.lx64) * v2 + e(P.ly64 * P.hx64) * v3 + e(P.ly64 * P.lx64) * v4
    if m64 is not None:
        val = val * m64[:, :, None]
    return _cols_layout(val)


def _exact_weights(P):
    """ly, lx from the float32 spec are exact differences; hy, hx in float64 are the exact 1 - l"""
    if not hasattr(P, "ly64"):
        P.ly64, P.lx64 = P.ly.astype(np.float64), P.lx.astype(np.float64)
        P.hy64 = np.where(P.valid, 1.0 - P.ly64, 0.0)
        P.hx64 = np.where(P.valid, 1.0 - P.lx64, 0.0)
    return P


def forward64(x, offset, weight, bias=None, mask=None, stride=1, pad=1, dg=1, mask_is_logit=False):
    """The whole forward in float64 from the spec's positions: y (N, Cout, Ho, Wo); no intermediate rounding."""
    N, C, H, W = x.shape
    P = _exact_weights(Positions(offset, H, W, stride, pad, dg))
    cols = sample64(x, P, mask_values(mask, dg, mask_is_logit, np.float64))
    return cols_gemm(cols, weight, bias)


def cols_gemm(cols, weight, bias=None):
    """(N, Ho, Wo, 9, C) x (Cout, C, 3, 3) -> (N, Cout, Ho, Wo), float64"""
    w = np.asarray(weight, dtype=np.float64)
    Cout, C = w.shape[:2]
    wk = w.reshape(Cout, C, 9).transpose(0, 2, 1)                       # [o][k][c]
    y = np.einsum("nhwkc,okc->nohw", np.asarray(cols, dtype=np.float64), wk, optimize=True)
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)[None, :, None, None]
    return y


class Grads(object):
    """Analytic float64 gradients of the sampling for a cotangent ``dcol`` (N, Ho, Wo, 9, C) of the cols, with the
    absolute-value sums S and operation counts T of the module docstring:

    ``dx, S_dx, T_dx`` (N, C, H, W); ``doffset, S_doffset`` (N, 18 dg, Ho, Wo); ``dmask, S_dmask`` (N, 9 dg, Ho, Wo) (of
    the logit with ``mask_is_logit``); ``T_doffset``, ``T_dmask`` ints."""

    def __init__(self, x, offset, dcol, mask=None, stride=1, pad=1, dg=1, mask_is_logit=False):
        N, C, H, W = x.shape
        Cg = C // dg
        P = _exact_weights(Positions(offset, H, W, stride, pad, dg))
        self.P = P
        m = mask_values(mask, dg, mask_is_logit, np.float64)
        mm = np.ones(P.valid.shape) if m is None else m
        mm = np.where(P.valid, mm, 0.0)                                       # an invalid sample has no gradient
        d = _from_cols(np.asarray(dcol, dtype=np.float64), dg)              # (N, dg, Cg, 9, Ho, Wo)
        v1, v2, v3, v4 = _gather(x, P, np.float64)
        e = lambda a: a[:, :, None]
        hy, hx, ly, lx = e(P.hy64), e(P.hx64), e(P.ly64), e(P.lx64)
        extra = OPS_LOGIT if (mask is not None and mask_is_logit) else 0
        # offsets
        gy = (v3 - v1) * hx + (v4 - v2) * lx
        gx = (v2 - v1) * hy + (v4 - v3) * ly
        ay = (np.abs(v3) + np.abs(v1)) * hx + (np.abs(v4) + np.abs(v2)) * lx
        ax = (np.abs(v2) + np.abs(v1)) * hy + (np.abs(v4) + np.abs(v3)) * ly
        ddy, ddx = mm * (d * gy).sum(2), mm * (d * gx).sum(2)               # (N, dg, 9, Ho, Wo)
        sdy, sdx = np.abs(mm) * (np.abs(d) * ay).sum(2), np.abs(mm) * (np.abs(d) * ax).sum(2)
        self.doffset = np.stack([ddy, ddx], 3).reshape(N, 18 * dg, P.Ho, P.Wo)
        self.S_doffset = np.stack([sdy, sdx], 3).reshape(N, 18 * dg, P.Ho, P.Wo)
        self.T_doffset = Cg + OPS_DOFF + extra
        # mask
        val = (hy * hx) * v1 + (hy * lx) * v2 + (ly * hx) * v3 + (ly * lx) * v4
        aval = (hy * hx) * np.abs(v1) + (hy * lx) * np.abs(v2) + (ly * hx) * np.abs(v3) + (ly * lx) * np.abs(v4)
        dm = np.where(P.valid, (d * val).sum(2), 0.0)
        sm = np.where(P.valid, (np.abs(d) * aval).sum(2), 0.0)
        self.T_dmask = Cg + OPS_DMASK
        if mask is not None and mask_is_logit:
            s = mask_values(mask, dg, True, np.float64)
            dm, sm = dm * s * (1.0 - s), sm * s * (1.0 - s)
            self.T_dmask += extra + 6
        self.dmask = dm.reshape(N, 9 * dg, P.Ho, P.Wo)
        self.S_dmask = sm.reshape(N, 9 * dg, P.Ho, P.Wo)
        # input: scatter every corner's contribution; count the terms of every element
        size = N * dg * Cg * H * W
        dx, S, cnt = np.zeros(size), np.zeros(size), np.zeros(N * dg * H * W)
        n = np.arange(N)[:, None, None, None, None, None]
        g = np.arange(dg)[None, :, None, None, None, None]
        c = np.arange(Cg)[None, None, :, None, None, None]
        dmm = d * e(mm)
        for (y, xx, inside), w in zip(P.corners(), (hy * hx, hy * lx, ly * hx, ly * lx)):
            t = dmm * np.where(e(inside), w, 0.0)
            flat = ((((n * dg + g) * Cg + c) * H + e(y)) * W + e(xx)).ravel()
            dx += np.bincount(flat, weights=t.ravel(), minlength=size)
            S += np.bincount(flat, weights=np.abs(t).ravel(), minlength=size)
            flat = (((n[:, :, 0] * dg + g[:, :, 0]) * H + y) * W + xx).ravel()
            cnt += np.bincount(flat, weights=inside.astype(np.float64).ravel(), minlength=cnt.size)
        dx, S, cnt = dx.reshape(N, dg, Cg, H, W), S.reshape(N, dg, Cg, H, W), cnt.reshape(N, dg, 1, H, W)
        self.dx, self.S_dx = dx.reshape(N, C, H, W), S.reshape(N, C, H, W)
        self.T_dx = np.broadcast_to(cnt, dx.shape).reshape(N, C, H, W) + OPS_DX + extra
        self.terms_dx = cnt.reshape(N, dg, H, W)


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


# ---- the grid_sample formulation (pins the oracle in test_deform_oracle.py; the float64 autograd reference) -----------
def deform_conv_autograd(x, offset, weight, bias=None, mask=None, stride=1, pad=1, dg=1):
    """torch (any float dtype, differentiable): the same function through ``F.grid_sample(align_corners=True,
    padding_mode='zeros')``, whose bilinear rule has the same zero corners.  The validity test is implied: a sample with
    py <= -1 or py >= H has only corners outside the map.  Returns y (N, Cout, Ho, Wo)."""
    import torch.nn.functional as F
    N, C, H, W = x.shape
    Ho, Wo = offset.shape[2:]
    Cg = C // dg
    off = offset.reshape(N, dg, 9, 2, Ho, Wo)
    k = torch.arange(9)
    by = (torch.arange(Ho).view(1, Ho, 1) * stride - pad + (k // 3).view(9, 1, 1) * pad).to(x.dtype)
    bx = (torch.arange(Wo).view(1, 1, Wo) * stride - pad + (k % 3).view(9, 1, 1) * pad).to(x.dtype)
    py, px = by + off[:, :, :, 0], bx + off[:, :, :, 1]                      # (N, dg, 9, Ho, Wo)
    gx = 2.0 * px / max(W - 1, 1) - 1.0
    gy = 2.0 * py / max(H - 1, 1) - 1.0
    grid = torch.stack([gx, gy], -1).reshape(N * dg, 9 * Ho, Wo, 2)
    s = F.grid_sample(x.reshape(N * dg, Cg, H, W), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    s = s.reshape(N, dg, Cg, 9, Ho, Wo)
    if mask is not None:
        s = s * mask.reshape(N, dg, 1, 9, Ho, Wo)
    cols = s.permute(0, 4, 5, 3, 1, 2).reshape(N, Ho, Wo, 9, C)
    wk = weight.reshape(weight.shape[0], C, 9).permute(0, 2, 1)
    y = torch.einsum("nhwkc,okc->nohw", cols, wk)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y
