"""CPU checks of tests/select_cases.py: the closed-form answers agree with every oracle that restates the selection or
the NMS, every family reaches the edge it is named for (from ``describe`` and from the graphs themselves), and the
comparison helpers of the GPU tests reject the wrong answers these edges would produce."""
import numpy as np
import pytest

import dense_detect_ref as DD
import fcos_ref as F
import proposal_ref as PR
import select_cases as S
import target_ref as TR
from oracle import box_ref as B

u32, f32 = np.uint32, np.float32
KEY_CASES = S.key_cases()
GRAPHS = S.graphs()
EQUAL = S.equal_score_graphs()


def _ids(cases):
    return [c["name"] for c in cases]


# ---- helpers -------------------------------------------------------------------------------------------------------------
def test_order_key_and_its_inverses():
    v = np.asarray([np.inf, 3.0e38, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -3.0e38, -np.inf], f32)
    k = S.order_key(v)
    assert np.all(np.diff(k[:5].astype(np.int64)) < 0) and k[4] == k[5] and np.all(np.diff(k[5:].astype(np.int64)) < 0)
    assert k[4] == 0x80000000 and k[0] == 0xFF800000 and k[-1] == 0x007FFFFF
    back = S.key_floats(k)
    assert np.array_equal(back.view(u32), np.where(v.view(u32) == 0x80000000, 0, v.view(u32)))
    for bad in (0xFFFFFFFF, 0xFF800001, 0x00000000, 0x007FFFFE, 0x7FFFFFFF):        # +NaN, +NaN, -NaN, -NaN, "-0"
        with pytest.raises(ValueError):
            S.key_floats(np.asarray([bad], u32))
    c = np.asarray([0, 1, 12345, 0x7FFFFFFF], np.int32)
    m = S.member_keys(c)
    assert m.tolist() == [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF - 12345, 0x80000000]
    assert np.array_equal(S.caller_keys(m), c)
    with pytest.raises(ValueError):
        S.caller_keys(np.asarray([0x7FFFFFFF], u32))


def test_describe_on_a_hand_made_case():
    keys = np.asarray([0x80000400, 0x80000800, 0x80000400, 0x80000C00, 0x80000400], u32)
    d = S.describe(keys, 3)
    assert (d["T"], d["gt"], d["eq"], d["need"], d["last_tie"]) == (0x80000400, 2, 3, 1, 0)
    assert [f["multi"] for f in d["fields"]] == [False, True, False]
    assert [f["digit"] for f in d["fields"]] == [1024, 1, 0]
    assert S.expected(keys, 3)[0].tolist() == [3, 1, 0] and S.expected(keys, 3)[1].tolist() == [0, 1, 3]


# ---- the closed forms against the oracles ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KEY_CASES, ids=_ids(KEY_CASES))
def test_key_family_equals_every_oracle(case):
    keys, k, n = case["keys"], case["k"], case["n"]
    by_key, by_index = S.expected(keys, k)
    assert by_key.shape == (k,) and np.array_equal(np.sort(by_key), by_index)
    if case["int_ok"]:
        ck = S.caller_keys(keys)
        assert np.array_equal(S.member_keys(ck), keys)
        pm, nm, npos, nneg = TR.sample_assigned(np.ones((1, n), np.int32), k, 1.0, keys=[ck])
        assert np.array_equal(pm[0], S.mask_of(by_index, n)) and not nm.any() and (npos[0], nneg[0]) == (k, 0)
        pm, nm, npos, nneg = TR.sample_assigned(np.zeros((1, n), np.int32), k, 0.25, keys=[ck])
        assert np.array_equal(nm[0], S.mask_of(by_index, n)) and not pm.any() and (npos[0], nneg[0]) == (0, k)
    v = case["values"]
    if v is None:
        return
    assert np.array_equal(S.order_key(v), keys)
    assert np.array_equal(DD.kept_anchors(v, k), by_index)
    assert np.array_equal(F.kept_points(v.astype(np.float64), k), by_index)
    if k <= 4096:
        anchors, shape = S.line_anchors(n)
        with np.errstate(over="ignore"):
            props, aidx, counts = PR.rpn_proposals([v.reshape(1, 1, 1, n)], [np.zeros((1, 4, 1, n), f32)], [anchors], [shape],
                                                   nms_pre=k, nms_post=k, max_num=k, nms_thr=0.7,
                                                   decode=lambda r, d, s: r)
        assert counts[0] == k and np.array_equal(aidx[0], by_key)
        assert np.array_equal(props[0, :, :4], anchors[by_key])


@pytest.mark.parametrize("g", GRAPHS + EQUAL, ids=_ids(GRAPHS + EQUAL))
def test_graph_formula_equals_the_nms_oracles(g):
    forms = [g] if np.all(g["scores"] == g["scores"][0]) and g["n"] > 1 else [g, S.shuffled(g)]
    for h in forms:
        keep, kept, cnt = B.nms(h["boxes"], h["scores"], h["thr"])
        S.check_keep(h, keep, kept, cnt)
        # as the middle segment of three
        pad = S.g5_disjoint(3)
        boxes = np.concatenate([pad["boxes"], h["boxes"], pad["boxes"]])
        scores = np.concatenate([pad["scores"], h["scores"], pad["scores"]])
        keep, kept, counts = PR.batched_nms(boxes, scores, [0, 3, 3 + h["n"], 6 + h["n"]], h["thr"])
        assert counts.tolist() == [3, h["kept"].shape[0], 3]
        S.check_keep(h, keep[3:3 + h["n"]], np.where(kept[3:3 + h["n"]] >= 0, kept[3:3 + h["n"]] - 3, -1), counts[1])


# ---- hollowness: every family reaches its edge ----------------------------------------------------------------------------
K23 = S.key_cases("K2", "K3")


@pytest.mark.parametrize("case", K23, ids=_ids(K23))
def test_k2_k3_decide_in_one_field_inside_a_tie_group(case):
    d = S.describe(case["keys"], case["k"])
    e = case["edge"]
    assert S.decided_in(d) == [e["field"]], d
    assert 0 < d["need"] < d["eq"] and d["eq"] >= 5
    assert case["n"] > case["k"]
    digit = d["fields"][e["field"]]["digit"]
    shift, mask = S.FIELDS[e["field"]]
    occupied = np.unique((case["keys"] >> u32(shift)) & u32(mask))
    if e["family"] == "K2":
        assert case["n"] > S.STEP and occupied.shape[0] == 400          # two steps, plenty of bins
        return
    want = e["want"]
    if want in ("odd", "even"):
        assert digit % 2 == (want == "odd")
        assert occupied.min() < digit < occupied.max()
    else:
        assert digit == (occupied.max() if want == "top" else occupied.min())
        assert (d["gt"] == 0) if want == "top" else (d["gt"] + d["eq"] == case["n"])
    if "digit" in e:                                                         # the extremes of the member keys
        assert digit == e["digit"] and int(S.caller_keys(np.asarray([d["T"]], u32))[0]) == e["caller"]
    if e["field"] == 2 and case["name"].startswith("K3_lo_pos") and want in ("top", "bottom"):
        assert digit == (1023 if want == "top" else 0)


def test_k2_k3_cover_both_signs_and_every_field():
    seen = {(c["edge"]["family"], c["edge"]["field"], bool(c["keys"][0] & u32(0x80000000))) for c in K23}
    assert seen == {(f, i, s) for f in ("K2", "K3") for i in range(3) for s in (True, False)}
    wants = {(c["edge"]["field"], c["edge"]["want"]) for c in S.key_cases("K3")}
    assert wants == {(i, w) for i in range(3) for w in ("odd", "even", "top", "bottom")}


def test_k1_k4_k5_k6_reach_their_edges():
    for c in S.key_cases("K1"):
        d = S.describe(c["keys"], c["k"])
        assert d["gt"] == 0 and d["eq"] == c["n"] and d["need"] == c["k"] and S.decided_in(d) == []
        assert np.array_equal(S.expected(c["keys"], c["k"])[0], np.arange(c["k"]))
    assert {(c["n"], c["k"]) for c in S.key_cases("K1")} == {(n, k) for n in (8191, 8192, 8193, 16385)
                                                           for k in (1, 1023, 1024, 1025, n - 1)}
    lasts = []
    for c in S.key_cases("K4"):
        d = S.describe(c["keys"], c["k"])
        assert c["n"] == 2 * S.STEP + 5 and d["eq"] == 8 and d["gt"] == 1000
        assert tuple(np.nonzero(c["keys"] == u32(d["T"]))[0]) == S.K4_TIES
        assert d["last_tie"] == c["edge"]["last_tie"]
        # the first tie left out is the next member of the group
        assert S.K4_TIES[d["need"]] not in S.expected(c["keys"], c["k"])[1]
        lasts.append(d["last_tie"])
    assert lasts == [S.STEP - 1, S.STEP, 2 * S.STEP - 1, 2 * S.STEP]
    (c,) = S.key_cases("K5")
    d = S.describe(c["keys"], c["k"])
    bits = c["values"].view(u32)
    assert d["T"] == 0x80000000 and d["eq"] == 12 and d["need"] == 6
    taken = S.expected(c["keys"], c["k"])[0][-6:]
    assert set(bits[taken].tolist()) == {0, 0x80000000}, "both zeros among the ties taken"
    assert np.all(np.diff(taken) > 0)
    for p in (0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF):
        assert (bits == p).sum() == 2
    by_key = S.expected(c["keys"], c["n"])[0]
    assert np.all(c["values"][by_key][:-1] >= c["values"][by_key][1:])
    assert {(c["n"], c["k"]) for c in S.key_cases("K6")} >= {(1, 1), (8, 8), (8, 7), (9, 8), (9, 9)}


def test_mixed_levels_share_k_and_keep_their_edges():
    m = S.mixed_levels()
    assert m["sizes"] == (S.STEP + 1, 2 * S.STEP + 5) and 4 <= m["k"] <= 4096
    got = []
    for cases in m["images"]:
        assert tuple(c["n"] for c in cases) == m["sizes"] and all(c["k"] == m["k"] and c["int_ok"] for c in cases)
        for c in cases:
            d = S.describe(c["keys"], c["k"])
            assert 0 < d["need"] < d["eq"]
            got.append((S.decided_in(d), d["last_tie"]))
    assert got[0][0] == [] and got[2][0] == [2] and got[1][1] == S.STEP and got[3][1] == 2 * S.STEP - 1


def _pair_suppresses(g, i, j):
    num, den = S.line_iou(g["boxes"][i], g["boxes"][j])
    return f32(num) / f32(den) > f32(g["thr"])


@pytest.mark.parametrize("g", GRAPHS, ids=_ids(GRAPHS))
def test_graph_pairs_are_what_they_claim(g):
    assert np.all(g["boxes"] == np.round(g["boxes"])) and g["boxes"].max() < (1 << 17) and g["boxes"].min() >= 0
    suppressed = set()
    for i, j in g["pairs"]:
        assert i < j and g["keep"][i] and not g["keep"][j] and _pair_suppresses(g, i, j)
        suppressed.add(j)
    assert suppressed == set(np.nonzero(g["keep"] == 0)[0].tolist())


def test_graph_families_cross_chunks_and_super_chunks():
    by = {}
    for g in GRAPHS:
        fam = g["name"][:2]
        n, c, s = S.crossings(g)
        t = by.setdefault(fam, [0, 0, 0])
        t[0], t[1], t[2] = t[0] + n, t[1] + c, t[2] + s
    for fam in ("G1", "G3", "G4"):
        assert by[fam][1] > 0 and by[fam][2] > 0, (fam, by[fam])
    assert by["G5"] == [0, 0, 0]
    # G1 as a chain from index 0 keeps the even boxes: the overlapping pairs on a boundary, (63, 64) and (1023, 1024),
    # have a dead first box (the scan must NOT apply them); behind a leading box the same pairs suppress
    for n, pair in ((65, (63, 64)), (1025, (1023, 1024))):
        plain, lead = S.g1_chain(n), S.g1_chain(n, lead=True)
        assert pair in plain["overlaps"] and pair not in plain["pairs"] and not plain["keep"][pair[0]] and plain["keep"][pair[1]]
        assert pair in lead["pairs"] and lead["keep"][pair[0]] and not lead["keep"][pair[1]]
        for g in (plain, lead):
            assert all(_pair_suppresses(g, i, j) for i, j in g["overlaps"])
    for g in GRAPHS:
        if g["name"].startswith("G3"):
            D = g["D"]
            if D >= 64:
                assert S.crossings(g)[1] == D
            if D >= 1024:
                assert S.crossings(g)[2] == D
    for t in S.G4_TRIPLES:
        g = S.g4_dead(t)
        a, b, c = t
        assert g["keep"][a] and not g["keep"][b] and g["keep"][c]
        assert _pair_suppresses(g, a, b) and _pair_suppresses(g, b, c) and not _pair_suppresses(g, a, c)
        assert S.line_iou(g["boxes"][b], g["boxes"][c]) == (24 * 16, 40 * 16)
    spans = [(a // 64 != b // 64, b // 64 != c // 64, a // 1024 != b // 1024, b // 1024 != c // 1024) for a, b, c in S.G4_TRIPLES]
    assert any(s[0] for s in spans) and any(s[1] for s in spans) and any(s[2] for s in spans) and any(s[3] for s in spans)
    for strict in (False, True):
        g = S.g6_threshold(strict)
        for i, j in g["exact_pairs"]:
            num, den = S.line_iou(g["boxes"][i], g["boxes"][j])
            assert 2 * num == den and f32(num) / f32(den) == f32(0.5)
            assert _pair_suppresses(g, i, j) == strict
    assert f32(S.THR_BELOW_HALF) < f32(0.5) and float(f32(S.THR_BELOW_HALF)) == S.THR_BELOW_HALF
    assert [i // 64 != j // 64 for i, j in S.G6_PAIRS] == [False, True, True] and S.G6_PAIRS[2][0] // 1024 != S.G6_PAIRS[2][1] // 1024


# ---- the checker rejects wrong answers ------------------------------------------------------------------------------------
def test_check_selection_rejects_wrong_tie_cuts():
    c = S.key_case("K4_last8192")
    keys, k = c["keys"], c["k"]
    by_key, by_index = S.expected(keys, k)
    S.check_selection(keys, k, by_key, by_index)
    d = S.describe(keys, k)
    ties = np.nonzero(keys == u32(d["T"]))[0]
    above = np.nonzero(keys > u32(d["T"]))[0]
    lower = np.nonzero(keys < u32(d["T"]))[0]
    # the cut one tie too early (a lower key fills the place), one too late (a key above is dropped)
    early = np.concatenate([by_key[:-1], lower[:1]])
    late = np.concatenate([by_key[1:], ties[d["need"]:d["need"] + 1]])
    # the right count of ties, but the wrong ones: the first tie past the step boundary instead of the last before it
    skipped = np.concatenate([by_key[:-1], ties[d["need"]:d["need"] + 1]])
    swapped = by_key.copy()
    swapped[-1], swapped[-2] = by_key[-2], by_key[-1]
    assert keys[swapped[-1]] == keys[swapped[-2]] and above.shape[0] == d["gt"]
    for wrong in (early, late, skipped, swapped):
        assert wrong.shape == by_key.shape
        with pytest.raises(AssertionError):
            S.check_selection(keys, k, by_key=wrong)
    for wrong in (early, late, skipped):
        with pytest.raises(AssertionError):
            S.check_selection(keys, k, by_index=np.sort(wrong))
    with pytest.raises(AssertionError):
        S.check_selection(keys, k, by_index=by_index[:-1])


def test_check_keep_rejects_wrong_masks():
    g = S.g1_chain(130)
    kept_pad = np.full(g["n"], -1, np.int64)
    kept_pad[:g["kept"].shape[0]] = g["kept"]
    S.check_keep(g, g["keep"], kept_pad, g["kept"].shape[0])
    # a scan that forgets removals across a chunk boundary: every suppressor of G3 with D = 64 sits one chunk back
    h = S.g3_long(64, False)
    blind = h["keep"].copy()
    blind[64:] = 1                                                           # no word of chunk 0 reaches chunk 1
    with pytest.raises(AssertionError):
        S.check_keep(h, keep=blind)
    with pytest.raises(AssertionError):
        S.check_keep(h, count=int(blind.sum()))
    with pytest.raises(AssertionError):
        S.check_keep(h, kept_idx=np.nonzero(blind)[0])
    # a dead box that suppresses: c of a G4 triple goes
    t = S.g4_dead((62, 63, 64))
    dead = t["keep"].copy()
    dead[64] = 0
    with pytest.raises(AssertionError):
        S.check_keep(t, keep=dead)
    kp = np.full(t["n"], -1, np.int64)
    kp[:int(dead.sum())] = np.nonzero(dead)[0]
    with pytest.raises(AssertionError):
        S.check_keep(t, kept_idx=kp)
    with pytest.raises(AssertionError):
        S.check_keep(t, count=int(dead.sum()))
    # and such a scan is what the chain looks like when every box suppresses its neighbour, dead or not
    all_suppress = np.zeros(g["n"], np.uint8)
    all_suppress[0] = 1
    with pytest.raises(AssertionError):
        S.check_keep(g, keep=all_suppress)
