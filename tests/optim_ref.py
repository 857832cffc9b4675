"""numpy reference of the fused SGD step (include/tdn.h ``tdn_sgd_step``): the arithmetic contract with an
EXACTLY rounded fp32 fma, the float64 norm, the skip rule and the loss-scale state machine.

fma.  a * b of two fp32 values is exact in float64 (48 significant bits).  Adding c in float64 and rounding the sum to
fp32 would round twice; instead the float64 sum is rounded TO ODD (TwoSum gives the exact error term of the addition: if
it is not zero and the sum's last bit is even, the sum moves one step towards the error), and a round-to-odd value with
53 >= 24 + 2 bits rounds to the same fp32 as the exact value does.  ``tests/test_optim_oracle.py`` proves ``fma32``
against ``fractions.Fraction``.
"""
import fractions
import math

import numpy as np

F32 = np.float32


def fma32(a, b, c):
    """round_to_fp32(a * b + c), one rounding; fp32 arrays (or scalars) in, fp32 array out."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b                                    # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)              # TwoSum: p + c = s + err exactly (finite s)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F32)


def round_fraction_f32(fr):
    """``fr`` (a Fraction) rounded to the nearest fp32, ties to even — integer arithmetic only."""
    if fr == 0:
        return F32(0.0)
    sign = -1 if fr < 0 else 1
    fr = abs(fr)
    e = math.floor(math.log2(fr)) - 23
    while fr / fractions.Fraction(2) ** e >= 1 << 24:
        e += 1
    while fr / fractions.Fraction(2) ** e < 1 << 23:
        e -= 1
    e = max(e, -149)                                 # subnormals: fixed spacing 2^-149
    q = fr / fractions.Fraction(2) ** e
    n = q.numerator // q.denominator
    rem = q - n
    if rem > fractions.Fraction(1, 2) or (rem == fractions.Fraction(1, 2) and n & 1):
        n += 1
    v = math.ldexp(n, e)                             # n < 2^25: exact in a double
    return F32(sign * v) if v < 2.0 ** 128 else F32(sign * np.inf)


def fma_fraction(a, b, c):
    return round_fraction_f32(fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c)))


def grad_sumsq(grads):
    """S = sum of g^2 over every gradient, float64."""
    with np.errstate(all="ignore"):
        return float(sum(np.sum(np.asarray(g, dtype=np.float64) ** 2) for g in grads if g is not None))


class RefSGD(object):
    """``groups``: list of dicts lr / weight_decay / momentum / params (indices into the parameter list).  The state
    lives here; ``step(grads, coef=None)`` updates ``params`` / ``bufs`` (lists of fp32 arrays) in place."""

    def __init__(self, params, groups, nesterov=False, max_norm=None, scale=1.0, dynamic=False, growth=2.0, backoff=0.5,
                 interval=2000, skip_nonfinite=True):
        self.params = [np.array(p, dtype=F32) for p in params]
        self.bufs = [np.zeros_like(p) for p in self.params]
        self.groups = groups
        self.nesterov, self.max_norm, self.dynamic = nesterov, max_norm, dynamic
        self.growth, self.backoff, self.interval, self.skip_nonfinite = F32(growth), F32(backoff), interval, skip_nonfinite
        self.scale = F32(scale)
        self.tracker = self.taken = self.skipped = self.last_skipped = 0
        self.buf_init = False
        self.grad_norm = self.clip_coef = F32(0)

    def step(self, grads, coef=None):
        with np.errstate(all="ignore"):
            S = grad_sumsq(grads)
            finite = math.isfinite(S)
            inv = F32(1.0) / self.scale
            n = F32(np.sqrt(np.float64(S)) * np.float64(inv))
            if coef is None:
                coef = F32(1.0)
                if self.max_norm is not None and self.max_norm > 0:
                    c = F32(self.max_norm) / (n + F32(1e-6))
                    coef = F32(1.0) if c > F32(1.0) else c
            coef = F32(coef)
            self.grad_norm, self.clip_coef = n, coef
            skipped = self.skip_nonfinite and not finite
            scale = self.scale
            if self.dynamic:                         # torch._amp_update_scale_
                if not finite:
                    self.scale, self.tracker = F32(scale * self.backoff), 0
                else:
                    ok = self.tracker + 1
                    if ok == self.interval:
                        grown = F32(scale * self.growth)
                        if np.isfinite(grown):
                            self.scale = grown
                        self.tracker = 0
                    else:
                        self.tracker = ok
            self.last_skipped = int(skipped)
            if skipped:
                self.skipped += 1
                return
            self.taken += 1
            m = F32(coef * inv)
            first = not self.buf_init
            for grp in self.groups:
                lr, wd, mom = F32(grp["lr"]), F32(grp["weight_decay"]), F32(grp["momentum"])
                for i in grp["params"]:
                    if grads[i] is None:
                        continue
                    p = self.params[i]
                    gh = np.asarray(grads[i], dtype=F32) * m
                    d = fma32(wd, p, gh) if wd != 0 else gh
                    u = d
                    if mom != 0:
                        b = d.copy() if first else (self.bufs[i] * mom) + d
                        self.bufs[i][...] = b
                        u = fma32(mom, b, d) if self.nesterov else b
                    p[...] = fma32(-lr, u, p)
            self.buf_init = True
