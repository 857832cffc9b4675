"""Inputs that drive the shared selection and NMS cores (csrc/select_core.h, csrc/nms_core.h) to their structural edges,
with answers that are formulas rather than the output of an oracle ("edge inputs").  NumPy only.

Selection.  A key family is a (n,) uint32 array of SELECT keys (what block_radix_threshold sees) and a k.  The answer is
the definition: the k highest by (key desc, index asc).  ``key_floats`` turns select keys into the fp32 values whose
``order_key`` they are, ``caller_keys`` into the int32 keys of ``sample_assigned`` (select key = 0x80000000 |
(0x7FFFFFFF - key)).  ``describe`` says, from the keys alone, which radix pass decides the threshold and how the tie
group is cut, so that a test can assert that a family reaches the edge it is named for.

NMS.  The boxes are intervals on a line, [x, 0, x + w - 1, 15]: two boxes of width w that lie d <= w apart share
(w - d) * 16 pixels of a union of (w + d) * 16, so their '+1' IoU is (w - d) / (w + d) with integer numerator and
denominator below 2^24 — one correctly rounded fp32 division, the same in every implementation.  Each graph states its
keep mask as a formula of the index and lists the (kept suppressor, suppressed) pairs that make it so.
"""
import numpy as np

f32, u32 = np.float32, np.uint32
FIELDS = ((21, 0x7FF), (10, 0x7FF), (0, 0x3FF))     # shift, mask of radix passes 0, 1, 2
STEP = 8192                                          # keys per step of the selection (1024 threads x 8)
CHUNK, SUPER = 64, 1024                              # boxes per mask word / per super-chunk of the keep scan


# ---- keys ----------------------------------------------------------------------------------------------------------
def order_key(values):
    """select_core.h's order_key on the bit patterns of fp32 values: -0 is +0, negatives are inverted."""
    u = np.ascontiguousarray(values, dtype=f32).view(u32).copy()
    u[u == 0x80000000] = 0
    neg = (u & u32(0x80000000)) != 0
    return np.where(neg, ~u, u | u32(0x80000000)).astype(u32)


def key_floats(keys):
    """The fp32 values whose order_key is ``keys`` (the inverse of order_key).  NaN patterns and the one key no float
    has (0x7FFFFFFF: the -0 that order_key folds into +0) are refused."""
    k = np.ascontiguousarray(keys, dtype=u32)
    u = np.where((k & u32(0x80000000)) != 0, k & u32(0x7FFFFFFF), ~k).astype(u32)
    if np.any((u & u32(0x7FFFFFFF)) > u32(0x7F800000)):
        raise ValueError("a key maps to a NaN pattern")
    if np.any(u == u32(0x80000000)):
        raise ValueError("key 0x7FFFFFFF is the order_key of no float")
    v = u.view(f32)
    assert np.array_equal(order_key(v), k)
    return v


def caller_keys(keys):
    """The int32 caller keys of sample_assigned whose select keys are ``keys`` (all need bit 31: they are members)."""
    k = np.ascontiguousarray(keys, dtype=u32)
    if not np.all(k & u32(0x80000000)):
        raise ValueError("a member's select key has bit 31 set")
    return (np.int64(0x7FFFFFFF) - (k & u32(0x7FFFFFFF)).astype(np.int64)).astype(np.int32)


def member_keys(caller):
    """Select keys of members with the given int32 caller keys."""
    return (u32(0x80000000) | (np.int64(0x7FFFFFFF) - np.asarray(caller, np.int64)).astype(u32)).astype(u32)


def expected(keys, k):
    """The definition: the k highest by (key desc, index asc) -> (in that order, in ascending index order)."""
    keys = np.asarray(keys, dtype=u32)
    n = keys.shape[0]
    order = np.lexsort((np.arange(n), -keys.astype(np.int64)))[:k]
    return order.astype(np.int64), np.sort(order).astype(np.int64)


def describe(keys, k):
    """What the radix select meets: threshold T, #(key > T), #(key == T), need = k - #(key > T), and per digit field
    whether the keys that agree with T on the higher fields occupy more than one bin, with T's digit there."""
    keys = np.asarray(keys, dtype=u32)
    assert 1 <= k <= keys.shape[0]
    T = np.sort(keys)[::-1][k - 1]
    gt, eq = int((keys > T).sum()), int((keys == T).sum())
    cand = keys
    fields = []
    for shift, mask in FIELDS:
        digits = (cand >> u32(shift)) & u32(mask)
        d = int((T >> u32(shift)) & u32(mask))
        fields.append(dict(multi=bool(np.unique(digits).shape[0] > 1), digit=d))
        cand = cand[digits == d]
    ties = np.nonzero(keys == T)[0]
    return dict(T=int(T), gt=gt, eq=eq, need=k - gt, fields=fields, last_tie=int(ties[k - gt - 1]))


def decided_in(desc):
    """The fields in which more than one bin is occupied."""
    return [i for i, f in enumerate(desc["fields"]) if f["multi"]]


def bf16_exact(values):
    return bool(np.all((np.ascontiguousarray(values, f32).view(u32) & u32(0xFFFF)) == 0))


def check_selection(keys, k, by_key=None, by_index=None):
    """The comparison of the GPU tests: a selection, in key order and / or ascending index order, against the definition."""
    ek, ei = expected(keys, k)
    if by_key is not None:
        got = np.asarray(by_key, np.int64)
        assert got.shape == ek.shape and np.array_equal(got, ek), \
            "key order differs at %s" % np.nonzero(got != ek)[0][:4].tolist() if got.shape == ek.shape else "length"
    if by_index is not None:
        got = np.asarray(by_index, np.int64)
        assert got.shape == ei.shape and np.array_equal(got, ei), \
            "selection differs at %s" % np.nonzero(got != ei)[0][:4].tolist() if got.shape == ei.shape else "length"


def mask_of(idx, n):
    m = np.zeros((n,), np.uint8)
    m[np.asarray(idx, np.int64)] = 1
    return m


# ---- key families -----------------------------------------------------------------------------------------------------
def _case(name, keys, k, values=None, **edge):
    keys = np.ascontiguousarray(keys, dtype=u32)
    c = dict(name=name, keys=keys, k=int(k), n=int(keys.shape[0]), edge=edge)
    c["int_ok"] = bool(np.all(keys & u32(0x80000000)))
    if values is not None:
        values = np.ascontiguousarray(values, dtype=f32)
        assert np.array_equal(order_key(values), keys)
        c["values"] = values
    else:
        try:
            c["values"] = key_floats(keys)
        except ValueError:
            c["values"] = None
    return c


def k1_cases():
    """All keys equal: the whole selection is the tie rule."""
    out = []
    key = order_key([0.5])[0]
    for n in (8191, 8192, 8193, 16385):
        for k in (1, 1023, 1024, 1025, n - 1):
            out.append(_case("K1_n%d_k%d" % (n, k), np.full((n,), key, u32), k, family="K1"))
    return out


_FIELD_NAMES = ("hi", "mid", "lo")                  # bits 21..31, 10..20, 0..9
_BASE = {"hi": 0x30000000, "mid": 0x3F800000, "lo": 0x3F800000}
_SHIFT = {"hi": 21, "mid": 10, "lo": 0}


def _grouped(field, sign, digits, seed):
    """fp32 patterns base + (j << shift) for j in ``digits`` (negated for sign < 0), value j 5..40 times, in a fixed
    shuffled order -> (keys, values)."""
    g = np.random.default_rng(seed)
    digits = np.asarray(digits, np.int64)
    counts = g.integers(5, 41, digits.shape[0])
    pat = (np.int64(_BASE[field]) + (digits << _SHIFT[field])).astype(u32)
    if sign < 0:
        pat = pat | u32(0x80000000)
    pat = np.repeat(pat, counts)
    pat = pat[g.permutation(pat.shape[0])]
    values = pat.view(f32)
    return order_key(values), values


def _cut_inside(keys, T):
    """k that takes half of T's tie group (at least one, never all)."""
    eq = int((keys == T).sum())
    assert eq >= 2
    return int((keys > T).sum()) + eq // 2


def _pick(keys, field, want):
    """The threshold key whose digit in ``field`` is the top / bottom occupied one, or the first odd / even one a third
    of the way down."""
    shift, mask = FIELDS[_FIELD_NAMES.index(field)]
    uniq = np.unique(keys)[::-1]                     # descending
    if want == "top":
        return uniq[0]
    if want == "bottom":
        return uniq[-1]
    for T in uniq[uniq.shape[0] // 3:]:
        if ((int(T) >> shift) & mask) % 2 == (1 if want == "odd" else 0):
            return T
    raise AssertionError("no such digit")


def k2_cases():
    """One deciding field: ~400 values that differ only there, n ~ 9000 (two steps), the cut inside a tie group."""
    out = []
    for fi, field in enumerate(_FIELD_NAMES):
        for sign in (1, -1):
            g = np.random.default_rng(100 + fi)
            hi_digit = {"hi": 500, "mid": 2048, "lo": 1024}[field]
            digits = np.sort(g.choice(hi_digit, 400, replace=False))
            keys, values = _grouped(field, sign, digits, 200 + 10 * fi + (sign < 0))
            T = np.unique(keys)[::-1][130]
            out.append(_case("K2_%s_%s" % (field, "pos" if sign > 0 else "neg"), keys, _cut_inside(keys, T), values,
                             family="K2", field=fi))
    return out


def k3_cases():
    """Threshold-digit ownership: in the deciding field T's digit is odd (a thread's high bin), even (its low bin), the
    highest occupied bin, the lowest.  ~100 values, n ~ 2200."""
    out = []
    for fi, field in enumerate(_FIELD_NAMES):
        top = {"hi": 500, "mid": 2048, "lo": 1024}[field]
        g = np.random.default_rng(300 + fi)
        digits = np.unique(np.concatenate([[0, top - 1], g.choice(top, 100, replace=False)]))
        for sign in (1, -1):
            keys, values = _grouped(field, sign, digits, 400 + 10 * fi + (sign < 0))
            for want in ("odd", "even", "top", "bottom"):
                T = _pick(keys, field, want)
                out.append(_case("K3_%s_%s_%s" % (field, "pos" if sign > 0 else "neg", want), keys, _cut_inside(keys, T),
                                 values, family="K3", field=fi, want=want))
    # integer keys only: the member digits 2047 (caller key 0) and 1024 (caller key 0x7FFFFFFF) of pass 0
    g = np.random.default_rng(330)
    digits = np.unique(np.concatenate([[0, 1023], g.choice(1024, 100, replace=False)]))
    counts = g.integers(5, 41, digits.shape[0])
    for want, low in (("top", 0x1FFFFF), ("bottom", 0)):
        keys = np.repeat((u32(0x80000000) | (digits.astype(u32) << u32(21)) | u32(low)).astype(u32), counts)
        keys = keys[np.random.default_rng(331).permutation(keys.shape[0])]
        T = _pick(keys, "hi", want)
        out.append(_case("K3_hi_int_%s" % want, keys, _cut_inside(keys, T), family="K3", field=0, want=want,
                         digit=2047 if want == "top" else 1024, caller=0 if want == "top" else 0x7FFFFFFF))
    return out


K4_TIES = (8190, 8191, 8192, 8193, 16382, 16383, 16384, 16385)


def _k4(need, n_above, name):
    n = 2 * STEP + 5
    T = order_key([1.0])[0] + u32(16)               # the neighbours below differ in bits 0..9 only
    idx = np.arange(n)
    rest = np.setdiff1d(idx, K4_TIES)
    above = np.random.default_rng(40).choice(rest, n_above, replace=False)
    keys = (T - u32(1) - (idx % 5).astype(u32)).astype(u32)
    keys[above] = T + u32(1) + (above % 7).astype(u32)
    keys[list(K4_TIES)] = T
    return _case(name, keys, n_above + need, family="K4", last_tie=K4_TIES[need - 1])


def k4_cases():
    """The tie cut on a step boundary: n = 2 * 8192 + 5, eight ties around indices 8192 and 16384, 1000 keys above."""
    return [_k4(need, 1000, "K4_last%d" % K4_TIES[need - 1]) for need in (2, 3, 6, 7)]


def mixed_levels():
    """Two images x two levels of 8193 and 16389 keys that share one k: all-equal keys and a cut on the step boundary
    for image 0, a pass-2 threshold inside a tie group and a cut on the second boundary for image 1."""
    if "mixed" not in _CACHE:
        src = key_case("K2_lo_pos")
        keys = src["keys"][:STEP + 1]
        k = _cut_inside(keys, np.unique(keys)[::-1][130])
        img0 = [_case("M_equal", np.full((STEP + 1,), order_key([0.5])[0], u32), k, family="K1"), _k4(3, k - 3, "M_k4_8192")]
        img1 = [_case("M_lo", keys, k, src["values"][:STEP + 1], family="K2", field=2), _k4(6, k - 6, "M_k4_16383")]
        _CACHE["mixed"] = dict(k=k, sizes=(STEP + 1, 2 * STEP + 5), images=[img0, img1])
    return _CACHE["mixed"]


def k5_cases():
    """Float specials: +-inf, +-FLT_MAX, +-denormals, +-1 and twelve zeros of both signs as the tie group that is cut."""
    pat = [0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF,
           0x3F800000, 0xBF800000] * 2 + [0x00000000, 0x80000000] * 6
    pat = np.asarray(pat, u32)
    pat = pat[np.random.default_rng(50).permutation(pat.shape[0])]
    values = pat.view(f32)
    keys = order_key(values)
    zero = order_key([0.0])[0]
    return [_case("K5_specials", keys, _cut_inside(keys, zero), values, family="K5")]


def k6_cases():
    """Degenerate shapes: n = 1, n = k (no select path), k = n - 1, one thread's eight keys and one more."""
    base = order_key([2.0])[0]
    pat = np.asarray([3, 1, 3, 2, 1, 3, 1, 2, 1], u32)
    out = []
    for n, k in ((1, 1), (8, 8), (8, 7), (8, 3), (9, 9), (9, 8), (9, 1)):
        out.append(_case("K6_n%d_k%d" % (n, k), base + pat[:n], k, family="K6"))
    return out


_CACHE = {}


def key_cases(*families):
    """All cases of the named families (default: all), built once."""
    if "all" not in _CACHE:
        _CACHE["all"] = k1_cases() + k2_cases() + k3_cases() + k4_cases() + k5_cases() + k6_cases()
    fam = families or ("K1", "K2", "K3", "K4", "K5", "K6")
    return [c for c in _CACHE["all"] if c["edge"]["family"] in fam]


def key_case(name):
    return next(c for c in key_cases() if c["name"] == name)


def line_anchors(n):
    """n 16 x 16 boxes 64 px apart on a line (nothing overlaps: NMS keeps everything), and the (h, w) that holds them."""
    x = (64 * np.arange(n)).astype(f32)
    a = np.stack([x, np.zeros(n, f32), x + f32(15), np.full(n, 15, f32)], -1).astype(f32)
    return a, (16, 64 * n)


# ---- suppression graphs ---------------------------------------------------------------------------------------------
W = 32
GAP = 32                                             # pitch of disjoint width-32 boxes: they touch, IoU 0


def _boxes(x, w=W):
    x = np.asarray(x, np.int64)
    assert x.min() >= 0 and x.max() + w - 1 < (1 << 17)
    return np.stack([x, np.zeros_like(x), x + w - 1, np.full_like(x, 15)], -1).astype(f32)


def line_iou(a, b):
    """Exact IoU of two of these boxes as a pair of integers (numerator, denominator)."""
    iw = int(min(a[2], b[2]) - max(a[0], b[0])) + 1
    inter = max(iw, 0) * 16
    area = lambda r: (int(r[2] - r[0]) + 1) * 16
    return inter, area(a) + area(b) - inter


def _graph(name, boxes, keep, pairs, thr=0.5, equal=False, **extra):
    n = boxes.shape[0]
    scores = np.full((n,), 0.5, f32) if equal else np.arange(n, 0, -1).astype(f32)
    keep = np.asarray(keep, bool)
    g = dict(name=name, boxes=boxes, scores=scores, thr=float(thr), keep=keep.astype(np.uint8),
             kept=np.nonzero(keep)[0].astype(np.int64), pairs=[(int(i), int(j)) for i, j in pairs], n=n)
    g.update(extra)
    return g


def shuffled(g, seed=7):
    """The same graph with its rows permuted (row i moves to perm[i]); scores must decide the order."""
    assert np.all(np.diff(g["scores"]) < 0)
    perm = np.random.default_rng(seed).permutation(g["n"])
    boxes, scores = np.empty_like(g["boxes"]), np.empty_like(g["scores"])
    boxes[perm], scores[perm] = g["boxes"], g["scores"]
    keep = np.zeros_like(g["keep"])
    keep[perm] = g["keep"]
    out = dict(g, name=g["name"] + "_shuffled", boxes=boxes, scores=scores, keep=keep, kept=perm[g["kept"]].astype(np.int64),
               perm=perm)
    return out


def g1_chain(n, equal=False, lead=False):
    """Box i at 8i, width 32: neighbours 0.6, next-but-one 1/3 -> exactly the even indices survive.  Every pair that
    straddles a chunk boundary, (63, 64) or (1023, 1024), then has a DEAD first box; with ``lead`` a disjoint box comes
    first, the chain starts at index 1, the odd indices survive and those pairs suppress."""
    i = np.arange(n)
    if lead:
        x = np.where(i == 0, 8 * n + 64, 8 * (i - 1))
        return _graph("G1_lead_n%d%s" % (n, "_eq" if equal else ""), _boxes(x), (i == 0) | (i % 2 == 1),
                      [(j - 1, j) for j in range(2, n, 2)], equal=equal, overlaps=[(j - 1, j) for j in range(2, n)])
    return _graph("G1_n%d%s" % (n, "_eq" if equal else ""), _boxes(8 * i), i % 2 == 0,
                  [(j - 1, j) for j in range(1, n, 2)], equal=equal, overlaps=[(j - 1, j) for j in range(1, n)])


def g2_cover(n, equal=False):
    """n copies of one box: only the first survives."""
    i = np.arange(n)
    return _graph("G2_n%d%s" % (n, "_eq" if equal else ""), _boxes(np.full(n, 100)), i == 0, [(0, j) for j in range(1, n)],
                  equal=equal)


def g3_long(D, extra, equal=False):
    """Disjoint boxes, box i + D a copy of box i (i < D); with ``extra`` a disjoint last box."""
    n = 2 * D + (1 if extra else 0)
    i = np.arange(n)
    x = GAP * np.where(i < 2 * D, i % D, D)
    return _graph("G3_D%d_n%d%s" % (D, n, "_eq" if equal else ""), _boxes(x), (i < D) | (i >= 2 * D),
                  [(j, j + D) for j in range(D)], equal=equal, D=D)


G4_TRIPLES = ((0, 1, 2), (62, 63, 64), (0, 64, 1100), (1022, 1023, 1024), (5, 1029, 2053))


def g4_dead(triple, equal=False):
    """a suppresses b, b alone would suppress c, a does not touch c: c survives.  Everything else is disjoint."""
    a, b, c = triple
    n = max(c + 30, 130)
    x = 56 * np.arange(n)                            # 56-px slots: a, b and c (a + 16 .. a + 47) fit into a's
    x[b], x[c] = x[a] + 8, x[a] + 16
    keep = np.ones(n, bool)
    keep[b] = False
    return _graph("G4_%d_%d_%d%s" % (a, b, c, "_eq" if equal else ""), _boxes(x), keep, [(a, b)], equal=equal, triple=triple)


def g5_disjoint(n, equal=False):
    return _graph("G5_n%d%s" % (n, "_eq" if equal else ""), _boxes(GAP * np.arange(n)), np.ones(n, bool), [], equal=equal)


G6_PAIRS = ((10, 11), (63, 64), (1023, 1024))
THR_BELOW_HALF = float(np.nextafter(f32(0.5), f32(0)))


def g6_threshold(strict, equal=False):
    """Width 24, shift 8: IoU 16/32 = 0.5 exactly.  At thr = 0.5 nothing goes; just below, the second of each pair."""
    n = 1100
    x = GAP * np.arange(n)
    keep = np.ones(n, bool)
    for i, j in G6_PAIRS:
        x[j] = x[i] + 8
        keep[j] = not strict
    return _graph("G6_%s%s" % ("below" if strict else "at", "_eq" if equal else ""), _boxes(x, 24), keep,
                  G6_PAIRS if strict else [], thr=THR_BELOW_HALF if strict else 0.5, equal=equal, exact_pairs=G6_PAIRS)


G1_SIZES = (63, 64, 65, 1023, 1024, 1025, 2049, 4096)
G2_SIZES = (64, 65, 1025, 4096)
G3_D = (1, 63, 64, 65, 1023, 1024, 1025)
G5_SIZES = (64, 65, 1024, 1025, 4096)


def graphs():
    """Every graph at every listed size, with strictly decreasing scores (built once)."""
    if "graphs" not in _CACHE:
        gs = [g1_chain(n, lead=l) for l in (False, True) for n in G1_SIZES] + [g2_cover(n) for n in G2_SIZES]
        gs += [g3_long(D, e) for D in G3_D for e in (False, True)]
        gs += [g4_dead(t) for t in G4_TRIPLES] + [g5_disjoint(n) for n in G5_SIZES]
        gs += [g6_threshold(False), g6_threshold(True)]
        _CACHE["graphs"] = gs
    return _CACHE["graphs"]


def equal_score_graphs():
    """One graph of every kind with all scores equal: index order is the sorted order."""
    if "eq" not in _CACHE:
        _CACHE["eq"] = [g1_chain(1025, True), g2_cover(1025, True), g3_long(1024, True, True), g4_dead((5, 1029, 2053), True),
                        g5_disjoint(1025, True), g6_threshold(False, True), g6_threshold(True, True)]
    return _CACHE["eq"]


def crossings(g):
    """(#pairs, #pairs across a 64-box chunk boundary, #pairs across a 1024-box super-chunk boundary) in sorted order."""
    p = g["pairs"]
    return len(p), sum(i // CHUNK != j // CHUNK for i, j in p), sum(i // SUPER != j // SUPER for i, j in p)


def check_keep(g, keep=None, kept_idx=None, count=None):
    """The comparison of the GPU tests: keep mask, kept indices in score order padded with -1, and the count."""
    if keep is not None:
        keep = np.asarray(keep)
        assert keep.shape == g["keep"].shape and np.array_equal(keep != 0, g["keep"] != 0), \
            "%s: keep mask differs at %s" % (g["name"], np.nonzero((keep != 0) != (g["keep"] != 0))[0][:6].tolist())
    if count is not None:
        assert int(count) == g["kept"].shape[0], "%s: count %d, expected %d" % (g["name"], int(count), g["kept"].shape[0])
    if kept_idx is not None:
        kept_idx = np.asarray(kept_idx, np.int64)
        ref = np.full((g["n"],), -1, np.int64)
        ref[:g["kept"].shape[0]] = g["kept"]
        assert kept_idx.shape == ref.shape and np.array_equal(kept_idx, ref), "%s: kept indices differ" % g["name"]
