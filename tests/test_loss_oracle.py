"""CPU: the loss oracle (tests/loss_ref.py) against an independent torch float64 restatement with
autograd, hand-worked values, the struct mirrors against the header, and the host refusals (which need no GPU)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [(5, 7), (3, 4), (1, 1)]


def dense_case(B, A, C, levels, seed, pos=0.05):
    g = np.random.default_rng(seed)
    N = sum(h * w for h, w in levels) * A
    cls = [g.normal(0, 1.5, (B, A * C, h, w)).astype(np.float32) for h, w in levels]
    reg = [g.normal(0, 0.5, (B, 4 * A, h, w)).astype(np.float32) for h, w in levels]
    labels = np.where(g.random((B, N)) < pos, g.integers(1, C + 1, (B, N)), 0).astype(np.int64)
    lw = g.choice(np.array([0, 1, 0.5], np.float32), (B, N), p=[0.3, 0.5, 0.2])
    bt = g.normal(0, 0.5, (B, N, 4)).astype(np.float32)
    bw = np.where((labels > 0)[..., None], g.choice(np.array([1, 0.5], np.float32), (B, N, 4)), 0).astype(np.float32)
    bt[..., 0] = np.where(labels > 0, 0.0, bt[..., 0])          # with preds near 0: both smooth-L1 branches
    return cls, reg, labels, lw, bt, bw


def torch_dense(cls, reg, labels, lw, bt, bw, avg, C, beta, gamma, alpha, g):
    """mmdetection's composition in float64: permute / reshape, expanded one-hot targets, F.* losses, autograd."""
    A = cls[0].shape[1] // C
    tc = [torch.tensor(c, dtype=torch.float64, requires_grad=True) for c in cls]
    tr = [torch.tensor(r, dtype=torch.float64, requires_grad=True) for r in reg]
    x = torch.cat([c.permute(0, 2, 3, 1).reshape(c.shape[0], -1, C) for c in tc], 1)
    r = torch.cat([c.permute(0, 2, 3, 1).reshape(c.shape[0], -1, 4) for c in tr], 1)
    onehot = torch.tensor(labels[..., None] == np.arange(1, C + 1), dtype=torch.float64)
    w = torch.tensor(lw, dtype=torch.float64)[..., None]
    if gamma is None:
        l = F.binary_cross_entropy_with_logits(x, onehot, reduction="none")
    else:
        gm, al = float(np.float32(gamma)), float(np.float32(alpha))
        p = torch.sigmoid(x)
        pt = (1 - p) * onehot + p * (1 - onehot)
        fw = (al * onehot + float(np.float32(1) - np.float32(alpha)) * (1 - onehot)) * pt.pow(gm)
        l = F.binary_cross_entropy_with_logits(x, onehot, reduction="none") * fw
    loss_cls = (l * w).sum() / avg
    lr = F.smooth_l1_loss(r, torch.tensor(bt, dtype=torch.float64), beta=float(np.float32(beta)), reduction="none")
    loss_reg = (lr * torch.tensor(bw, dtype=torch.float64)).sum() / avg
    (loss_cls * g[0] + loss_reg * g[1]).backward()
    return (loss_cls.item(), loss_reg.item()), [c.grad.numpy() for c in tc], [c.grad.numpy() for c in tr]


@pytest.mark.parametrize("A,C,gamma", [(3, 1, None), (2, 5, None), (2, 5, 2.0), (3, 4, 0.0), (1, 3, 1.5)])
def test_dense_oracle_vs_torch(A, C, gamma):
    cls, reg, labels, lw, bt, bw = dense_case(2, A, C, LEVELS, 3)
    g = (1.5, 0.75)
    ref = R.anchor_head_loss(cls, reg, labels, lw, bt, bw, 37.0, C, 1.0 / 9.0, gamma, 0.25, g)
    gs = (float(np.float32(g[0])), float(np.float32(g[1])))
    (lc, lr), dc, dr = torch_dense(cls, reg, labels, lw, bt, bw, 37.0, C, 1.0 / 9.0, gamma, 0.25, gs)
    assert ref["losses"][0] == pytest.approx(lc, rel=1e-12) and ref["losses"][1] == pytest.approx(lr, rel=1e-12)
    for a, b in zip(ref["dcls"] + ref["dreg"], dc + dr):
        # the oracle's s = g / avg is a float32 division: up to 2^-24 relative from torch's float64 one
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-7, atol=1e-14)
    for a, b in zip(ref["dreg32"], ref["dreg"]):
        assert a.dtype == np.float32 and np.allclose(a, b, rtol=3e-7, atol=0)
        assert np.array_equal(a == 0, b == 0)
    assert ref["mag"][0] >= abs(ref["losses"][0]) and ref["mag"][1] > 0


def roi_case(Rn, C, cols, seed):
    g = np.random.default_rng(seed)
    cls = g.normal(0, 2, (Rn, C)).astype(np.float32)
    reg = g.normal(0, 1, (Rn, cols)).astype(np.float32)
    labels = np.where(g.random(Rn) < 0.3, g.integers(1, max(C, 2), Rn), 0).astype(np.int64)
    lw = g.choice(np.array([0, 1, 0.5], np.float32), Rn, p=[0.2, 0.6, 0.2])
    bt = g.normal(0, 1, (Rn, 4)).astype(np.float32)
    bw = np.where((labels > 0)[:, None], np.float32(1), np.float32(0)) * lw[:, None]
    return cls, reg, labels, lw, bt, np.ascontiguousarray(np.broadcast_to(bw, (Rn, 4)), np.float32)


@pytest.mark.parametrize("C,specific", [(7, True), (7, False), (2, True)])
def test_roi_oracle_vs_torch(C, specific):
    Rn = 40
    cls, reg, labels, lw, bt, bw = roi_case(Rn, C, 4 * C if specific else 4, 5)
    ref = R.bbox_head_loss(cls, reg, labels, lw, bt, bw, None, 1.0, (2.0, 0.5))
    avg = max(int((lw > 0).sum()), 1)
    assert ref["avg"] == avg
    x = torch.tensor(cls, dtype=torch.float64, requires_grad=True)
    r = torch.tensor(reg, dtype=torch.float64, requires_grad=True)
    lc = (F.cross_entropy(x, torch.tensor(labels), reduction="none") * torch.tensor(lw, dtype=torch.float64)).sum() / avg
    if specific:                                    # mmdetection's expanded (R, 4C) targets and weights
        T = torch.zeros(Rn, 4 * C, dtype=torch.float64)
        Wt = torch.zeros(Rn, 4 * C, dtype=torch.float64)
        for i in range(Rn):
            T[i, 4 * labels[i]:4 * labels[i] + 4] = torch.tensor(bt[i], dtype=torch.float64)
            Wt[i, 4 * labels[i]:4 * labels[i] + 4] = torch.tensor(bw[i], dtype=torch.float64)
    else:
        T, Wt = torch.tensor(bt, dtype=torch.float64), torch.tensor(bw, dtype=torch.float64)
    lr = (F.smooth_l1_loss(r, T, beta=1.0, reduction="none") * Wt).sum() / avg
    (lc * 2.0 + lr * 0.5).backward()
    assert ref["losses"][0] == pytest.approx(lc.item(), rel=1e-12)
    assert ref["losses"][1] == pytest.approx(lr.item(), rel=1e-12)
    assert np.allclose(ref["dcls"], x.grad.numpy(), rtol=1e-7, atol=1e-14)
    assert np.allclose(ref["dreg"], r.grad.numpy(), rtol=1e-7, atol=1e-14)
    assert np.array_equal(ref["dreg32"] == 0, ref["dreg"] == 0)


def _one(x, t, w=1.0, gamma=None, alpha=0.25, avg=1.0):
    """One anchor, one class, one level."""
    cls = [np.full((1, 1, 1, 1), x, np.float32)]
    reg = [np.zeros((1, 4, 1, 1), np.float32)]
    return R.anchor_head_loss(cls, reg, np.array([[t]], np.int64), np.array([[w]], np.float32),
                              np.zeros((1, 1, 4), np.float32), np.zeros((1, 1, 4), np.float32), avg, 1, 1.0, gamma, alpha)


def test_hand_values():
    ln2 = math.log(2.0)
    for t in (0, 1):
        o = _one(0.0, t)
        assert o["losses"][0] == pytest.approx(ln2, rel=1e-15)
        assert o["dcls"][0].item() == pytest.approx(0.5 if t == 0 else -0.5, rel=1e-15)
    o = _one(0.0, 1, gamma=2.0, alpha=0.25)
    assert o["losses"][0] == pytest.approx(0.0625 * ln2, rel=1e-15)
    # smooth L1 at |d| = beta: 0.5 beta from both branches, gradient +-1
    beta = 0.25
    for d in (beta, -beta):
        just_in = np.nextafter(np.float32(abs(d)), np.float32(0)) * np.sign(d)
        l_out, g_out = R.smooth_l1(np.float32(d), np.float32(0), beta)
        l_in, g_in = R.smooth_l1(np.float32(just_in), np.float32(0), beta)
        assert l_out == 0.5 * beta and g_out == np.sign(d)
        assert l_in == pytest.approx(0.5 * beta, rel=1e-6) and g_in == pytest.approx(np.sign(d), rel=1e-6)
        assert 0.5 * d * d / beta == 0.5 * beta                      # the quadratic branch's value at the knee
        g32 = R.smooth_l1_grad32(np.array([d], np.float32), np.zeros(1, np.float32), np.ones(1, np.float32), 1.0, beta)
        assert g32[0] == np.sign(d)
    # uniform softmax logits: ln C
    C = 81
    o = R.bbox_head_loss(np.full((3, C), 1.25, np.float32), np.zeros((3, 4), np.float32), np.array([0, 5, 80]),
                         np.ones(3, np.float32), np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32))
    assert o["avg"] == 3 and o["losses"][0] == pytest.approx(math.log(C), rel=1e-14)
    assert o["dcls"][1, 5] == pytest.approx((1.0 / C - 1.0) / 3, rel=1e-7)


def test_weight_zero_hides_nan_and_zero_avg_divides_by_one():
    cls, reg, labels, lw, bt, bw = dense_case(2, 2, 3, LEVELS, 9)
    avg = (np.array([0, 0], np.int32), np.array([0], np.int32))
    clean = R.anchor_head_loss(cls, reg, labels, lw, bt, bw, avg, 3, 1.0 / 9.0, 2.0)
    assert clean["avg"] == 1.0
    A = 2
    for l, c in enumerate(cls):                                  # poison every logit / delta whose weight is 0
        w0 = R.unflatten_head(np.broadcast_to(lw[:, sum(h * w for h, w in LEVELS[:l]) * A:
                                                 sum(h * w for h, w in LEVELS[:l + 1]) * A, None],
                                              (2, LEVELS[l][0] * LEVELS[l][1] * A, 3)), A, 3, *LEVELS[l])
        c[w0 == 0] = np.nan
        b0 = R.unflatten_head(bw[:, sum(h * w for h, w in LEVELS[:l]) * A:sum(h * w for h, w in LEVELS[:l + 1]) * A],
                              A, 4, *LEVELS[l])
        reg[l][b0 == 0] = np.inf
    dirty = R.anchor_head_loss(cls, reg, labels, lw, bt, bw, avg, 3, 1.0 / 9.0, 2.0)
    assert np.array_equal(clean["losses"], dirty["losses"]) and np.all(np.isfinite(dirty["losses"]))
    for k in ("dcls", "dreg", "dreg32"):
        for a, b in zip(clean[k], dirty[k]):
            assert np.array_equal(a, b)
    assert R.divisor((np.array([3, 4], np.int32),)) == 7 and R.divisor(None, 0) == 1 and R.divisor(2.5) == 2.5
    r = R.bbox_head_loss(np.full((2, 4), np.nan, np.float32), np.zeros((2, 16), np.float32), np.zeros(2, np.int64),
                         np.zeros(2, np.float32), np.zeros((2, 4), np.float32), np.zeros((2, 4), np.float32))
    assert r["avg"] == 1 and np.all(r["losses"] == 0) and np.all(r["dcls"] == 0)


def test_struct_mirrors_match_the_header(tmp_path):
    from torch_detection_amd import _lib
    mirrors = {"tdn_loss_level": _lib.LossLevel, "tdn_loss_config": _lib.LossConfig, "tdn_loss_avg": _lib.LossAvg}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {']
    for cname, cls in mirrors.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)]).decode().split("\n"):
        if not ln:
            continue
        cname, fname, val = ln.split()
        cls = mirrors[cname]
        got = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert got == int(val), (cname, fname, got, val)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in mirrors.values())
    assert (_lib.LOSS_MAX_LEVELS, _lib.LOSS_MAX_CLASSES, _lib.LOSS_MAX_ROWS, _lib.LOSS_MAX_AVG) == (8, 1024, 1 << 20, 64)
    lib = _lib.load()                                           # the queries are host-only
    assert lib.tdn_loss_roi_workspace_bytes(1031) > 0 and lib.tdn_loss_roi_workspace_bytes((1 << 20) + 1) < 0
    assert lib.tdn_loss_roi_workspace_bytes(-1) < 0


def test_workspace_sizes_are_the_design_table():
    """DESIGN.md §5d worked by hand: 32 bytes per workgroup of the forward launch, rounded up to 256."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    # RoI head: a workgroup takes 16 rows, 256 workgroups at most
    assert lib.tdn_loss_roi_workspace_bytes(1031) == 2304              # 65 workgroups: 2080 -> 2304
    assert lib.tdn_loss_roi_workspace_bytes(0) == 256                  # still one workgroup
    assert lib.tdn_loss_roi_workspace_bytes(1 << 20) == 256 * 32
    assert lib.tdn_loss_roi_workspace_bytes((1 << 20) + 1) == -1 and lib.tdn_loss_roi_workspace_bytes(-1) == -1
    # dense heads, B = 2, A = 3, C = 80, levels 13 x 21 and 7 x 11: a workgroup takes 1024 chunks of 16 bytes.
    # fp32 (4 per chunk): 131040 / 4 + 6552 / 4 + 36960 / 4 + 1848 / 4 = 32760 + 1638 + 9240 + 462 = 44100 chunks,
    # 44 workgroups: 1408 -> 1536.  bf16 (8 per chunk): 16380 + 819 + 4620 + 231 = 22050 chunks, 22: 704 -> 768
    lv = (_lib.LossLevel * 2)()
    (lv[0].H, lv[0].W), (lv[1].H, lv[1].W) = (13, 21), (7, 11)        # a size query does not look at the pointers
    cfg = _lib.LossConfig(dtype=_lib.TDN_F32, num_anchors=3, num_classes=80, beta=1.0)
    assert lib.tdn_loss_dense_workspace_bytes(lv, 2, 2, ctypes.byref(cfg)) == 1536
    cfg.dtype = _lib.TDN_BF16
    assert lib.tdn_loss_dense_workspace_bytes(lv, 2, 2, ctypes.byref(cfg)) == 768
    assert lib.tdn_loss_dense_workspace_bytes(lv, 2, 65, ctypes.byref(cfg)) == -1
    assert lib.tdn_loss_dense_workspace_bytes(lv, 9, 2, ctypes.byref(cfg)) == -1
    cfg.num_classes = 1025
    assert lib.tdn_loss_dense_workspace_bytes(lv, 2, 2, ctypes.byref(cfg)) == -1
    cfg.num_classes, lv[1].W = 80, 0
    assert lib.tdn_loss_dense_workspace_bytes(lv, 2, 2, ctypes.byref(cfg)) == -1


def test_host_refusals_need_no_gpu():
    import torch_detection_amd as T
    cls, reg, labels, lw, bt, bw = [[torch.from_numpy(a) for a in v] if isinstance(v, list) else torch.from_numpy(v)
                                    for v in dense_case(2, 3, 1, LEVELS, 1)]

    def dense(cls=cls, reg=reg, labels=labels, lw=lw, bt=bt, bw=bw, avg=8.0, **kw):
        return T.anchor_head_loss(cls, reg, labels, lw, bt, bw, avg, **kw)

    sliced = [c[:, :, :, ::1].transpose(2, 3).contiguous().transpose(2, 3) for c in cls]       # W-major strides
    bad = [
        (lambda: dense(cls=sliced), "NCHW-contiguous or channels_last"),
        (lambda: dense(beta=0.0), "beta"),
        (lambda: dense(beta=-1.0), "beta"),
        (lambda: dense(labels=labels[:, :-1].contiguous()), "N = %d" % labels.shape[1]),
        (lambda: dense(bt=bt[:, :, :3].contiguous()), "bbox_targets"),
        (lambda: dense(reg=reg[:-1] + [reg[-1][:, :8].contiguous()]), r"bbox_preds\[2\]"),
        (lambda: dense(cls=cls[:2]), "2 cls_scores but 3 bbox_preds"),
        (lambda: dense(cls=cls * 3, reg=reg * 3), "levels"),                                      # 9 levels
        (lambda: dense(cls=[c.double() for c in cls]), "float32 / bfloat16 / float16"),
        (lambda: dense(cls=[torch.zeros(65, 3, 1, 1)], reg=[torch.zeros(65, 12, 1, 1)]), "batch size"),
        (lambda: dense(num_classes=2), "multiple of num_classes"),
        (lambda: dense(num_classes=1025), "num_classes"),
        (lambda: dense(cls=[torch.zeros(1, 3, 600, 600)], reg=[torch.zeros(1, 12, 600, 600)],
                       labels=torch.zeros(1, 1080000, dtype=torch.int64)), "anchors per image"),
        (lambda: dense(avg=torch.zeros(65, dtype=torch.int32)), "at most 64"),
        (lambda: dense(avg=torch.zeros(2)), "int32"),
        (lambda: dense(avg=0.0), "avg_factor"),
        (lambda: dense(avg=None), "avg_factor"),
        (lambda: dense(gamma=-1.0), "gamma"),
        (lambda: dense(), "must be a CUDA tensor"),                                               # and only then
    ]
    rc, rr, rl, rw, rt, rbw = [torch.from_numpy(a) for a in roi_case(12, 5, 20, 2)]
    out = rl.clone()
    out[3] = 5
    rw2 = rw.clone()
    rw2[3] = 1.0
    neg = rl.clone()
    neg[4] = -1
    rw3 = rw.clone()
    rw3[4] = 0.5
    bad += [
        (lambda: T.bbox_head_loss(rc, rr, out, rw2, rt, rbw), r"labels outside \[0, 5\)"),
        (lambda: T.bbox_head_loss(rc, rr, neg, rw3, rt, rbw), r"labels outside \[0, 5\)"),
        (lambda: T.bbox_head_loss(rc, rr[:, :8].contiguous(), rl, rw, rt, rbw), "bbox_pred"),
        (lambda: T.bbox_head_loss(rc, rr, rl, rw, rt, rbw, beta=0), "beta"),
        (lambda: T.bbox_head_loss(torch.zeros(12, 1025), torch.zeros(12, 4), rl, rw, rt, rbw), "classes"),
        (lambda: T.bbox_head_loss(rc, rr, rl[:-1], rw, rt, rbw), "labels"),
        (lambda: T.bbox_head_loss(rc, rr, rl.int(), rw, rt, rbw), "labels"),
        (lambda: T.bbox_head_loss(rc.t().contiguous().t(), rr, rl, rw, rt, rbw), "cls_score"),
        (lambda: T.bbox_head_loss(rc, rr, rl, rw, rt, rbw), "must be a CUDA tensor"),
    ]
    rw0 = rw2.clone()
    rw0[3] = 0.0                                # an out-of-range label on a weight-0 row passes the label check
    bad.append((lambda: T.bbox_head_loss(rc, rr, out, rw0, rt, rbw), "must be a CUDA tensor"))
    for i, (f, msg) in enumerate(bad):
        with pytest.raises(ValueError, match=msg):
            f()
            pytest.fail("case %d was accepted" % i)
