"""fp64 oracle, a-priori bounds and fault models for ONE member of a weight-gradient group (test infrastructure; pure
CPU, torch only).  The GPU test (test_gpu_wgrad_plans.py) and the CPU sensitivity test (test_wgrad_oracle.py) call the
same ``check_member``.

A member is a conv / grouped conv / stem conv with 16-bit operands x (NCHW), g (NCHW cotangent), w (OIHW; grouped:
[C, C/groups, k, k]) and, with BN operands, fp32 vectors scale, mean, invstd.  Its launch produces

    G[co, k]   = sum_m g[m, co] * x[pix(m) + tap(k), ci(k)]        the unscaled gradient, K = N * Ho * Wo terms
    dw         = scale * G
    dbeta      = sum_m g[m, co]
    dgamma     = invstd * (sum_k w[co, k] * G[co, k] - mean * dbeta)

all evaluated here in fp64 from the 16-bit operand values (products of two 16-bit values and sums of a few thousand of
them are exact or within 2^-53 relative: the oracle's own error is 2^-29 of the allowances below and is ignored).

Allowances (u = bound_util.U = 2^-23 per rounded operation, see bound_util's docstring for why that unit):

  dw      bound_util.wgrad_bound, exact variant: (K [+ 1 for the scale]) * u * scale * sum_m |g| |x|, + the fp32 store.
  dbeta   K additions of exactly representable terms in some order: K * u * sum_m |g|, + the fp32 store.
  dgamma  the kernel forms every G[co, k] with K rounded additions (|G~ - G| <= K u Gabs, Gabs = sum_m |g| |x|, the
          gradient of |x|, |g|), multiplies each by the exact 16-bit w (1 rounding), adds the Ktot products in some
          order (per tile, per wave, per block: at most Ktot - 1 additions on a path; Ktot counts the columns the kernel
          really adds, the zero-padded ones included: 7 x 32 for the stem, k * k * 64 for a grouped member), subtracts
          mean * dbeta~ (1 product, 1 subtraction; dbeta~ carries its own K roundings, fewer than the G path's
          K + Ktot) and multiplies by invstd (1 rounding).  Longest path: K + 1 + (Ktot - 1) + 1 + 1 + 1 = K + Ktot + 3
          operations, each of which perturbs a partial result whose magnitude is bounded by the same expression on
          absolute values:
              (K + Ktot + 3) * u * |invstd| * (sum_k |w| Gabs + |mean| sum_m |g|),  + the fp32 store.
  beta=1  onto a known previous value p: the result is p + new with one more rounded operation:
              (T + 1) * u * (S + |p|).
Nothing in these is tuned.

Two input generators.  ``uniform``: golden_util.det_tensor in [-1, 1] (x, g) and [-0.2, 0.2] (w), checked with the
allowances above.  ``integers``: x, g, w from {-1, 0, 1}, scale all ones, mean from {-1, 0, 1}, invstd a power of two:
every product and every partial sum, in ANY summation order, is an integer of magnitude below 2^24 (K <= 16384 pixels,
K * Ktot <= 2^24 for the dot) — nothing rounds, and dw, dgamma, dbeta must EQUAL the oracle.  ``generators`` decides
per case, from the uniform reference's own numbers, which of the two a case runs:

  * integers where the largest dw allowance is not smaller than the smallest non-zero product |g| * |x| of the
    uniform operands: there a single missing or doubled product can hide inside the allowance;
  * uniform where the largest dw allowance is smaller than the largest single product: there the bounds can see one
    product at least where it is big, and they are what checks non-trivial scale / mean / invstd and real rounding.
With operands that come arbitrarily close to zero the first holds for every case of the table, so every case has the
exact check; the 256-split cases (K ~ 16,000: allowance ~ 8, largest product 1) have only that.

Fault models (``mutants``): what a subtly wrong kernel would produce, applied to the oracle's own result — see
test_wgrad_oracle.py.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import bound_util as B
from golden_util import _hash_u01

Member = collections.namedtuple("Member", "kind N H W Cin Cout k stride pad groups")
# kind: "conv" | "gconv" | "stem"; H, W: INPUT size (stem: image size); pad is also the dilation of a 3x3 conv


def conv(N, H, W, Cin, Cout, k, stride=1, pad=None):
    return Member("conv", N, H, W, Cin, Cout, k, stride, (k // 2 if pad is None else pad), 1)


def gconv(N, H, W, C, groups, k=3, stride=1):
    return Member("gconv", N, H, W, C, C, k, stride, k // 2, groups)


def stem(N, H, W, Cout=64):
    return Member("stem", N, H, W, 3, Cout, 7, 2, 3, 1)


def dilation(m):
    return m.pad if (m.kind != "stem" and m.k == 3) else 1


def out_hw(m):
    d = dilation(m)
    return ((m.H + 2 * m.pad - (d * (m.k - 1) + 1)) // m.stride + 1,
            (m.W + 2 * m.pad - (d * (m.k - 1) + 1)) // m.stride + 1)


def pixels(m):
    ho, wo = out_hw(m)
    return m.N * ho * wo


def wshape(m):
    return (m.Cout, m.Cin // m.groups, m.k, m.k)


def ktot(m):
    """Columns the kernels add per output channel (padded ones included)."""
    if m.kind == "stem":
        return 7 * 32
    return m.k * m.k * (64 if m.kind == "gconv" else m.Cin)


# ---- operands -----------------------------------------------------------------------------------------------------
def _u01(shape, seed):
    return torch.from_numpy(_hash_u01(int(np.prod(shape)), seed).astype(np.float64)).reshape(shape)


def _uni(shape, seed, lo, hi, dtype):
    t = (_u01(shape, seed) * (hi - lo) + lo).float()
    return t.to(dtype).float().contiguous() if dtype is not None else t.contiguous()


def _tri(shape, seed):
    return (torch.floor(_u01(shape, seed) * 3.0) - 1.0).float().contiguous()     # {-1, 0, 1}


Operands = collections.namedtuple("Operands", "x g w scale mean invstd prev")


def make_operands(m, gen, dtype, bn, accumulate, seed):
    """fp32 containers of ``dtype``-representable x, g, w; fp32 scale / mean / invstd (None without BN); ``prev``:
    (dw, dgamma, dbeta) the accumulate call starts from, or None."""
    ho, wo = out_hw(m)
    xs, gs, ws = (m.N, m.Cin, m.H, m.W), (m.N, m.Cout, ho, wo), wshape(m)
    C = m.Cout
    if gen == "integers":
        x, g, w = _tri(xs, seed + 1), _tri(gs, seed + 2), _tri(ws, seed + 3)
        scale = torch.ones(C) if bn else None
        mean = _tri((C,), seed + 5) if bn else None
        invstd = torch.pow(2.0, torch.floor(_u01((C,), seed + 6) * 5.0) - 2.0).float() if bn else None
        prev = None
        if accumulate:
            prev = (torch.floor(_u01(ws, seed + 7) * 7.0).float() - 3.0,
                    (torch.floor(_u01((C,), seed + 8) * 7.0).float() - 3.0) if bn else None,
                    torch.floor(_u01((C,), seed + 9) * 7.0).float() - 3.0)
    else:
        assert gen == "uniform", gen
        x, g, w = _uni(xs, seed + 1, -1, 1, dtype), _uni(gs, seed + 2, -1, 1, dtype), _uni(ws, seed + 3, -0.2, 0.2, dtype)
        scale = _uni((C,), seed + 4, 0.5, 1.5, None) if bn else None
        mean = _uni((C,), seed + 5, -0.2, 0.2, None) if bn else None
        invstd = _uni((C,), seed + 6, 0.7, 1.4, None) if bn else None
        prev = None
        if accumulate:
            prev = (_uni(ws, seed + 7, -1, 1, None), _uni((C,), seed + 8, -1, 1, None) if bn else None,
                    _uni((C,), seed + 9, -1, 1, None))
    return Operands(x, g, w, scale, mean, invstd, prev)


# ---- oracle -------------------------------------------------------------------------------------------------------
class Ref(object):
    """The exact results of one member and everything the checks and fault models need."""

    def __init__(self, m, ops_, gen, G, Gabs):
        self.m, self.o, self.gen = m, ops_, gen
        self.G, self.Gabs = G, Gabs                                    # unscaled gradient and its absolute twin, fp64
        self.colsum = ops_.g.double().sum((0, 2, 3))
        self.colabs = ops_.g.double().abs().sum((0, 2, 3))
        self.K = pixels(m)
        self.bn = ops_.mean is not None

    def assemble(self, G, colsum, drop_mean_term=False):
        """(dw, dgamma, dbeta) in fp64 from an unscaled gradient and column sums (the oracle's, or mutated ones);
        the accumulate call's previous values added."""
        o = self.o
        dw = G if o.scale is None else G * o.scale.double().view(-1, 1, 1, 1)
        dbeta = colsum.clone()
        dgamma = None
        if self.bn:
            dot = (o.w.double() * G).sum((1, 2, 3))
            dgamma = o.invstd.double() * (dot if drop_mean_term else dot - o.mean.double() * colsum)
        if o.prev is not None:
            dw = dw + o.prev[0].double()
            dbeta = dbeta + o.prev[2].double()
            if dgamma is not None:
                dgamma = dgamma + o.prev[1].double()
        return dw, dgamma, dbeta

    def exact(self):
        return self.assemble(self.G, self.colsum)

    def bounds(self):
        """bound_util.Bound of (dw, dgamma, dbeta); dgamma None without BN."""
        o, K = self.o, self.K
        acc = 0 if o.prev is None else 1
        dw, dgamma, dbeta = self.exact()
        sc = None if o.scale is None else o.scale.double().view(-1, 1, 1, 1)
        S = self.Gabs if sc is None else self.Gabs * sc.abs()
        T = K + (sc is not None) * B.EPI_OPS["scale"] + acc
        bw = B.Bound(dw, S + (o.prev[0].double().abs() if acc else 0.0), T, None, "S: exact; v: fp64", activation=False)
        bb = B.Bound(dbeta, self.colabs + (o.prev[2].double().abs() if acc else 0.0), K + acc, None,
                     "dbeta: K * u * sum|g|", activation=False)
        bg = None
        if self.bn:
            Sg = o.invstd.double().abs() * ((o.w.double().abs() * self.Gabs).sum((1, 2, 3)) +
                                            o.mean.double().abs() * self.colabs)
            bg = B.Bound(dgamma, Sg + (o.prev[1].double().abs() if acc else 0.0), K + ktot(self.m) + 3 + acc, None,
                         "dgamma: (K + Ktot + 3) * u * |invstd| * (sum|w|Gabs + |mean| sum|g|)", activation=False)
        return bw, bg, bb


def reference(m, gen, dtype, bn, accumulate=False, seed=0):
    o = make_operands(m, gen, dtype, bn, accumulate, seed)
    # bound_util.wgrad_bound, exact variant, WITHOUT the scale: v = G, S = Gabs (the scale is applied in assemble /
    # bounds so that the fault models can work on the unscaled gradient)
    b = B.wgrad_bound(o.x, o.g, wshape(m), m.stride, m.pad, None, dilation(m), m.groups)
    return Ref(m, o, gen, b.v, b.S)


def generators(m, dtype, bn, accumulate=False, seed=0, ref_uniform=None):
    """Which generators a case runs, decided from the uniform reference's numbers (module docstring)."""
    r = ref_uniform if ref_uniform is not None else reference(m, "uniform", dtype, bn, accumulate, seed)
    bw = r.bounds()[0]
    e_max = float(bw.E.max())
    gx = r.o.g.abs()
    xx = r.o.x.abs()
    p_min = float(gx[gx > 0].min()) * float(xx[xx > 0].min())
    p_max = float(gx.max()) * float(xx.max()) * (1.0 if r.o.scale is None else float(r.o.scale.abs().max()))
    out = []
    if e_max >= p_min:
        out.append("integers")
    if e_max < p_max:
        out.append("uniform")
    return out


# ---- the check ----------------------------------------------------------------------------------------------------
def _unravel(flat, shape):
    idx = []
    for d in reversed(shape):
        idx.append(flat % d)
        flat //= d
    return tuple(reversed(idx))


def _check_equal(got, v, what):
    assert tuple(got.shape) == tuple(v.shape), (what, tuple(got.shape), tuple(v.shape))
    d = got.detach().double().cpu() - v
    bad = (d != 0) | torch.isnan(d)
    a = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d.abs())
    idx = _unravel(int(a.argmax()), v.shape)
    return {"what": what, "mode": "equal", "bad": bool(bad.any()), "count": int(bad.sum()), "index": list(idx),
            "got": float(got[idx]), "v": float(v[idx]), "err": float(a[idx]), "ratio": float("inf") if bool(bad.any()) else 0.0}


def _check_bound(got, b, what):
    r = B.check(got, b, torch.float32, None, what)
    r["mode"] = "bound"
    r["bad"] = not (r["ratio"] <= 1.0)
    return r


def check_member(ref, dw, dgamma, dbeta, what=""):
    """Every element of dw (OIHW), dgamma and dbeta against the oracle: equality for ``integers``, the a-priori
    allowances for ``uniform``.  Returns one record per output; ``rec["bad"]`` marks a failed one.  No element is
    excluded and there is no outlier fraction."""
    recs = []
    if ref.gen == "integers":
        vw, vg, vb = ref.exact()
        recs.append(_check_equal(dw, vw, what + " dw"))
        if vg is not None:
            recs.append(_check_equal(dgamma, vg, what + " dgamma"))
        recs.append(_check_equal(dbeta, vb, what + " dbeta"))
    else:
        bw, bg, bb = ref.bounds()
        recs.append(_check_bound(dw, bw, what + " dw"))
        if bg is not None:
            recs.append(_check_bound(dgamma, bg, what + " dgamma"))
        recs.append(_check_bound(dbeta, bb, what + " dbeta"))
    return recs


def worst(recs):
    return max(recs, key=lambda r: r["ratio"])


# ---- per-pixel terms: the fault models and the failure report -----------------------------------------------------------
def _xpad(ref):
    p = ref.m.pad
    return F.pad(ref.o.x.double(), (p, p, p, p))


def _pix(ref, mflat):
    ho, wo = out_hw(ref.m)
    n, r = divmod(int(mflat), ho * wo)
    return n, r // wo, r % wo


def pixel_term(ref, mflat, xp=None):
    """(dG, dcol): what output pixel ``mflat`` (flattened n, ho, wo) adds to the unscaled gradient and the column sum."""
    m = ref.m
    xp = _xpad(ref) if xp is None else xp
    n, h, w = _pix(ref, mflat)
    d, s, k = dilation(m), m.stride, m.k
    patch = xp[n, :, h * s:h * s + d * (k - 1) + 1:d, w * s:w * s + d * (k - 1) + 1:d]      # [Cin, k, k]
    gv = ref.o.g.double()[n, :, h, w]                                                       # [Cout]
    if m.groups > 1:
        cpg = m.Cin // m.groups
        patch = patch.view(m.groups, cpg, k, k).repeat_interleave(m.Cout // m.groups, 0)    # [Cout, cpg, k, k]
        return gv.view(-1, 1, 1, 1) * patch, gv
    return gv.view(-1, 1, 1, 1) * patch.unsqueeze(0), gv


def element_terms(ref, idx):
    """For one dw element (co, c, kh, kw): its exact term from every output pixel, in pixel order (scale applied)."""
    m = ref.m
    co, c, kh, kw = idx
    ho, wo = out_hw(m)
    d, s = dilation(m), m.stride
    ci = c + (co // (m.Cout // m.groups)) * (m.Cin // m.groups) if m.groups > 1 else c
    xs = _xpad(ref)[:, ci, kh * d:kh * d + s * (ho - 1) + 1:s, kw * d:kw * d + s * (wo - 1) + 1:s]
    t = (ref.o.g.double()[:, co] * xs).reshape(-1)
    return t if ref.o.scale is None else t * float(ref.o.scale[co])


def element_split_terms(ref, idx, mchunk):
    """The same per pixel split of ``mchunk`` pixels: the failure report names the split whose share, or whose one
    pixel, explains the error."""
    t = element_terms(ref, idx)
    return [float(t[i:i + mchunk].sum()) for i in range(0, t.numel(), mchunk)]


def owner(ref, idx, err, mchunk):
    """Which pixels explain a signed error ``err`` of dw element ``idx``: ("pixel", m, split, term) when one pixel's
    term, missing or doubled, is the closest explanation, else ("split", None, split, share)."""
    t = element_terms(ref, idx)
    rp = torch.minimum((t - err).abs(), (t + err).abs())
    mp = int(rp.argmin())
    sh = torch.tensor(element_split_terms(ref, idx, mchunk), dtype=torch.float64)
    rs = torch.minimum((sh - err).abs(), (sh + err).abs())
    sp = int(rs.argmin())
    if float(rp[mp]) <= float(rs[sp]):
        return "pixel", mp, mp // mchunk, float(t[mp])
    return "split", None, sp, float(sh[sp])


def explain(ref, rec, plan_row):
    """One line for a failed record: the worst element, the split whose pixels explain its error, and the tile."""
    variant, bmw, bnw, splitk, mchunk = plan_row[:5]
    msg = "%s: element %s got %.9g, exact %.9g, off by %.6g" % (rec["what"], tuple(rec["index"]), rec["got"], rec["v"],
                                                              rec["err"])
    if rec["mode"] == "bound":
        msg += " = %.3f x its allowance %.6g (T = %d)" % (rec["ratio"], rec["allowance"], rec["T"])
    else:
        msg += " (%d elements differ; must be equal)" % rec["count"]
    co = rec["index"][0]
    msg += "; plan: variant %d, tile %dx%d, %d splits of %d px" % (variant, bmw, bnw, splitk, mchunk)
    if rec["what"].endswith(" dw"):
        _, c, kh, kw = rec["index"]
        e = rec["got"] - rec["v"]
        if e == e:
            kind, mp, sp, val = owner(ref, tuple(rec["index"]), e, mchunk)
            span = "split %d (pixels %d..%d)" % (sp, sp * mchunk, min(ref.K, (sp + 1) * mchunk) - 1)
            if kind == "pixel":
                msg += "; error %.6g is closest to -/+ the term %.6g of pixel %d = (n, ho, wo) %s, owned by %s" % (
                    e, val, mp, _pix(ref, mp), span)
            else:
                msg += "; error %.6g is closest to -/+ the whole share %.6g of %s" % (e, val, span)
        tap = kh * ref.m.k + kw
        if variant:
            msg += "; tile (co %d, ci %d), tap %d" % (co // bmw, c // 64, tap)
        else:
            msg += "; tile (co %d, tap %d, ci %d)" % (co // bmw, tap, 0 if ref.m.kind != "conv" else c // bnw)
    else:
        msg += "; channel %d lies in co tile %d" % (co, co // bmw)
    return msg


# ---- fault models ---------------------------------------------------------------------------------------------------
MUTATIONS = ("drop first pixel of split 1", "drop last pixel of last split", "one pixel twice",
             "dw=-1 tap kept in column 0", "dh=-1 tap of first row from previous image", "one split's colsum missing",
             "dgamma without mean*dbeta")


def mutants(ref, splitk, mchunk):
    """Yields (name, (dw, dgamma, dbeta) or None): the oracle's result as a kernel with one fault would leave it, in
    fp32 like a GPU output.  None: the fault cannot be expressed on this member (no such tap, one image, no BN)."""
    m, o = ref.m, ref.o
    K = ref.K
    xp = _xpad(ref)
    ho, wo = out_hw(m)
    d, s, k, p = dilation(m), m.stride, m.k, m.pad

    def out(G, col, **kw):
        return tuple(None if t is None else t.float() for t in ref.assemble(G, col, **kw))

    def grouped(patch):                                 # [Cin, ...] -> per output channel [Cout, cpg, ...]
        if m.groups == 1:
            return patch.unsqueeze(0)
        cpg = m.Cin // m.groups
        return patch.view(m.groups, cpg, *patch.shape[1:]).repeat_interleave(m.Cout // m.groups, 0)

    first = mchunk if splitk > 1 else 0                 # a single split: its own first pixel
    dG, dc = pixel_term(ref, first, xp)
    yield MUTATIONS[0], out(ref.G - dG, ref.colsum - dc)
    dG, dc = pixel_term(ref, K - 1, xp)
    yield MUTATIONS[1], out(ref.G - dG, ref.colsum - dc)
    dG, dc = pixel_term(ref, min(mchunk, K) - 1, xp)    # the last pixel of split 0, counted by split 1 as well
    yield MUTATIONS[2], out(ref.G + dG, ref.colsum + dc)

    # missing line-end mask: in the flattened pixel order the left neighbour of column 0 is the last pixel of the row
    # above; the taps whose input column is negative at wo = 0 read it instead of zero
    x64, g64 = o.x.double(), o.g.double()
    if p > 0:
        G = ref.G.clone()
        xf = x64.permute(1, 0, 2, 3).reshape(m.Cin, m.N * m.H * m.W)     # pixel-major over the whole batch, as in NHWC
        for kw_ in range(k):
            wi = kw_ * d - p
            if wi >= 0:
                break
            for kh_ in range(k):
                for h in range(ho):
                    hi = h * s + kh_ * d - p
                    if hi < 0 or hi >= m.H:
                        continue
                    for n in range(m.N):
                        q = (n * m.H + hi) * m.W + wi       # row 0 of image n > 0: the last pixels of image n - 1
                        if q >= 0:
                            G[:, :, kh_, kw_] += g64[n, :, h, 0].view(-1, 1) * grouped(xf[:, q])
        yield MUTATIONS[3], out(G, ref.colsum)
    else:
        yield MUTATIONS[3], None
    # missing wrap over H: the rows above image n's first row are image n-1's last rows
    if p > 0 and m.N > 1:
        G = ref.G.clone()
        for kh_ in range(k):
            hi = kh_ * d - p
            if hi >= 0:
                break
            for kw_ in range(k):
                for w in range(wo):
                    wi = w * s + kw_ * d - p
                    if wi < 0 or wi >= m.W or m.H + hi < 0:
                        continue
                    for n in range(1, m.N):
                        G[:, :, kh_, kw_] += g64[n, :, 0, w].view(-1, 1) * grouped(x64[n - 1, :, m.H + hi, wi])
        yield MUTATIONS[4], out(G, ref.colsum)
    else:
        yield MUTATIONS[4], None
    sp = splitk - 1
    gm = g64.permute(1, 0, 2, 3).reshape(m.Cout, -1)
    yield MUTATIONS[5], out(ref.G, ref.colsum - gm[:, sp * mchunk:(sp + 1) * mchunk].sum(1))
    yield MUTATIONS[6], (out(ref.G, ref.colsum, drop_mean_term=True) if ref.bn else None)


@functools.lru_cache(maxsize=None)
def cached_reference(m, gen, dtype, bn, accumulate, seed):
    """One reference per (member, generator, ...), shared by the tests of a process and never modified."""
    return reference(m, gen, dtype, bn, accumulate, seed)
