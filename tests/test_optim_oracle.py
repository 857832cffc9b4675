"""CPU: the numpy reference of the fused SGD step (tests/optim_ref.py) against torch.optim.SGD(foreach=False),
clip_grad_norm_ and torch._amp_update_scale_; its exactly rounded fma against fractions.Fraction; the C ABI of
tdn_sgd_item, the host-only planning call and the wrappers' refusals.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SIZES = [1, 7, 64, 1000, 100003]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def _rand(rng, n, scale=1.0):
    return (rng.standard_normal(n) * scale).astype(F32)


# ---- the fma ---------------------------------------------------------------------------------------------------------
def test_fma32_equals_the_exact_rational_result():
    rng = np.random.default_rng(5)
    n = 4000
    a = _rand(rng, n) * F32(2.0) ** rng.integers(-20, 20, n).astype(F32)
    b = _rand(rng, n) * F32(2.0) ** rng.integers(-20, 20, n).astype(F32)
    c = _rand(rng, n) * F32(2.0) ** rng.integers(-40, 40, n).astype(F32)
    c[::5] = -(a[::5] * b[::5])                     # heavy cancellation
    # ties of the product that a small addend must break: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies halfway between two
    # fp32 values; rounding the float64 sum first would lose an addend below 2^-53 and then round the tie to even
    t = F32(1.0) + F32(2.0) ** -12
    ties = [(t, t, F32(s) * F32(2.0) ** e) for e in (-60, -80, -100, -126, -149) for s in (1, -1)]
    ties += [(t, t, F32(0.0)), (t, -t, F32(2.0) ** -70), (F32(3.0), F32(2.0) ** -149, F32(2.0) ** -149),
             (F32(1.5), F32(2.0) ** -149, F32(2.0) ** -150 * 0), (F32(3.4e38), F32(2.0), F32(-3.4e38))]
    for x, y, z in ties:
        a, b, c = (np.append(u, F32(w)).astype(F32) for u, w in ((a, x), (b, y), (c, z)))
    got = R.fma32(a, b, c)
    want = np.array([R.fma_fraction(x, y, z) for x, y, z in zip(a, b, c)], dtype=F32)
    assert np.array_equal(_bits(got), _bits(want))
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert not np.array_equal(_bits(naive), _bits(want))      # the tie cases do catch the double rounding


# ---- against torch.optim.SGD -----------------------------------------------------------------------------------------
def _torch_run(ps, grads_per_step, groups, nesterov, max_norm=None):
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.SGD([dict(params=[tp[i] for i in g["params"]], lr=g["lr"], weight_decay=g["weight_decay"],
                                momentum=g["momentum"]) for g in groups], lr=0.1, momentum=0.9, nesterov=nesterov,
                          foreach=False)
    norms, coefs = [], []
    for grads in grads_per_step:
        for p, g in zip(tp, grads):
            p.grad = torch.from_numpy(g.copy())
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
            norms.append(float(total))
            coefs.append(F32(min(1.0, float(torch.tensor(max_norm, dtype=torch.float32) / (total + 1e-6)))))
        opt.step()
    bufs = [opt.state[p].get("momentum_buffer") for p in tp]
    return [p.detach().numpy() for p in tp], [b.numpy() if b is not None else None for b in bufs], norms, coefs


VARIANTS = {
    "plain": dict(groups=lambda n: [dict(lr=0.05, weight_decay=1e-4, momentum=0.9, params=list(range(n)))], nesterov=False),
    "nesterov": dict(groups=lambda n: [dict(lr=0.05, weight_decay=1e-4, momentum=0.9, params=list(range(n)))], nesterov=True),
    "two_groups": dict(groups=lambda n: [dict(lr=0.05, weight_decay=1e-4, momentum=0.9, params=list(range(0, n, 2))),
                                         dict(lr=0.013, weight_decay=0.0, momentum=0.8, params=list(range(1, n, 2)))],
                       nesterov=False),
    "no_momentum": dict(groups=lambda n: [dict(lr=0.05, weight_decay=3e-3, momentum=0.0, params=list(range(n)))], nesterov=False),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS) + ["negative_zero"])
def test_reference_equals_torch_sgd_bitwise(variant):
    rng = np.random.default_rng(11)
    ps = [_rand(rng, n) for n in SIZES]
    steps = [[_rand(rng, n, 0.3) for n in SIZES] for _ in range(4)]
    v = VARIANTS["plain" if variant == "negative_zero" else variant]
    groups = v["groups"](len(ps))
    if variant == "negative_zero":
        groups[0]["weight_decay"] = 0.0
        for g in steps[0]:
            g[::3] = -0.0                                   # the first step copies: the sign must survive in the buffer
    tp, tb, _, _ = _torch_run(ps, steps, groups, v["nesterov"])
    ref = R.RefSGD(ps, groups, nesterov=v["nesterov"])
    for i, grads in enumerate(steps):
        ref.step(grads)
        if variant == "negative_zero" and i == 0:
            assert np.signbit(ref.bufs[2][::3]).all()
    for i in range(len(ps)):
        assert np.array_equal(_bits(ref.params[i]), _bits(tp[i])), (variant, SIZES[i])
        if tb[i] is not None:
            assert np.array_equal(_bits(ref.bufs[i]), _bits(tb[i])), (variant, SIZES[i])
    assert ref.taken == 4 and ref.skipped == 0


def test_reference_with_max_norm():
    rng = np.random.default_rng(12)
    ps = [_rand(rng, n) for n in SIZES]
    steps = [[_rand(rng, n, 0.3) for n in SIZES] for _ in range(4)]
    groups = VARIANTS["plain"]["groups"](len(ps))
    max_norm = 35.0
    tp, tb, norms, coefs = _torch_run(ps, steps, groups, False, max_norm)
    assert any(c < 1 for c in coefs)
    ref = R.RefSGD(ps, groups, max_norm=max_norm)
    free = R.RefSGD(ps, groups, max_norm=max_norm)
    for grads, n, c in zip(steps, norms, coefs):
        ref.step(grads, coef=c)                              # fed torch's coefficient: the update is torch's, bitwise
        free.step(grads)
        assert abs(float(free.grad_norm) - n) <= 1e-6 * n
        assert abs(float(free.clip_coef) - float(c)) <= 2e-6 * float(c)
    for i in range(len(ps)):
        assert np.array_equal(_bits(ref.params[i]), _bits(tp[i]))
        assert np.array_equal(_bits(ref.bufs[i]), _bits(tb[i]))


def test_scale_state_machine_equals_amp_update_scale():
    scale = torch.full((1,), 512.0)
    tracker = torch.zeros(1, dtype=torch.int32)
    ref = R.RefSGD([np.zeros(3, F32)], [dict(lr=0.1, weight_decay=0.0, momentum=0.9, params=[0])], scale=512.0,
                   dynamic=True, growth=2.0, backoff=0.5, interval=2)
    g_ok, g_bad = np.ones(3, F32), np.array([1, np.inf, 1], F32)
    seq = [0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0]
    for i, bad in enumerate(seq):
        torch._amp_update_scale_(scale, tracker, torch.full((1,), float(bad)), 2.0, 0.5, 2)
        ref.step([g_bad if bad else g_ok])
        assert float(ref.scale) == float(scale) and ref.tracker == int(tracker), i
        assert ref.last_skipped == bad
    assert ref.skipped == sum(seq) and ref.taken == len(seq) - sum(seq)
    # a static scale never moves, a skipped step leaves parameters and buffers alone
    st = R.RefSGD([np.ones(3, F32)], [dict(lr=0.1, weight_decay=0.0, momentum=0.9, params=[0])], scale=8.0)
    st.step([g_bad])
    assert float(st.scale) == 8.0 and st.skipped == 1 and np.array_equal(st.params[0], np.ones(3, F32))
    st.step([g_ok * 8])
    assert np.array_equal(_bits(st.params[0]), _bits(R.fma32(-F32(0.1), np.ones(3, F32), np.ones(3, F32))))


# ---- ABI, planning, refusals -----------------------------------------------------------------------------------------
def test_sgd_item_layout_matches_the_header(tmp_path):
    from torch_detection_amd import _lib
    cls = _lib.SgdItem
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(tdn_sgd_item));']
    for fname, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(tdn_sgd_item, %s));' % (fname, fname))
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)]).decode().split("\n"):
        if ln:
            fname, val = ln.split()
            got = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
            assert got == int(val), (fname, got, val)
            seen += 1
    assert seen == len(cls._fields_) + 1
    hdr = open(os.path.join(ROOT, "include", "tdn.h")).read()
    for name in ("SGD_MAX_ITEMS", "SGD_MAX_GROUPS", "SGD_PATH_LINEAR", "SGD_PATH_TRANSPOSED", "SGD_PATH_GENERAL",
                 "SGD_NESTEROV", "SGD_SKIP_NONFINITE", "SGD_DYNAMIC_SCALE", "SGD_F_SCALE", "SGD_F_NORM", "SGD_F_COEF",
                 "SGD_F_SNAP_SCALE", "SGD_F_COUNT", "SGD_I_TRACKER", "SGD_I_TAKEN", "SGD_I_SKIPPED",
                 "SGD_I_LAST_SKIPPED", "SGD_I_BUF_INIT", "SGD_I_SNAP_FIRST", "SGD_I_COUNT"):
        m = re.search(r"#define TDN_%s \(?([0-9 <]+)\)?" % name, hdr)
        assert m and eval(m.group(1)) == getattr(_lib, name), name


def _item(ptr, shape, ps, gs, group=0, buf=True):
    from torch_detection_amd import _lib
    it = _lib.SgdItem()
    it.p, it.g, it.buf = ptr, ptr + (1 << 30), (ptr + (2 << 30)) if buf else None
    it.shape = (ctypes.c_int64 * 4)(*shape)
    it.p_stride = (ctypes.c_int64 * 4)(*ps)
    it.g_stride = (ctypes.c_int64 * 4)(*gs)
    it.group = group
    return it


def test_planning_call_on_a_known_list():
    """Host only (the pointers are never followed).  Update chunks hold 4096 elements, norm chunks 16384; the
    transposed path takes one chunk per output channel while taps x Cin fits a chunk, else Cin is cut in multiples
    of 4."""
    from torch_detection_amd import _lib, optim_ops
    L, T, G = _lib.SGD_PATH_LINEAR, _lib.SGD_PATH_TRANSPOSED, _lib.SGD_PATH_GENERAL
    base = 1 << 40
    items = [
        _item(base, (1, 1, 1, 100003), (0, 0, 0, 1), (0, 0, 0, 1)),                                  # 25 + 7
        _item(base, (64, 64, 3, 3), (576, 9, 3, 1), (576, 1, 192, 64), group=1),                     # 64 + 3
        _item(base, (4, 512, 3, 3), (4608, 9, 3, 1), (4608, 1, 1536, 512)),                          # 4 * 2 + 2
        _item(base, (64, 64, 1, 1), (64, 1, 1, 1), (64, 1, 64, 64)),                                 # 1x1: one layout
        _item(base, (8, 6, 3, 3), (54, 1, 18, 6), (54, 9, 3, 1), buf=False),                         # channels_last p
        _item(base + 4, (1, 1, 1, 5), (0, 0, 0, 1), (0, 0, 0, 1)),
    ]
    pl = optim_ops.sgd_plan(items, 2)
    assert pl.paths == [L, T, T, L, G, L]
    assert pl.update_chunks == 25 + 64 + 8 + 1 + 1 + 1 and pl.norm_chunks == 7 + 3 + 2 + 1 + 1 + 1
    assert pl.norm_wgs == pl.norm_chunks and pl.update_wgs == pl.update_chunks and (pl.n, pl.n_groups) == (6, 2)
    assert pl.workspace_bytes == 256 and pl.table_bytes % 256 == 0 and pl.table_host.numel() == pl.table_bytes
    assert pl.table_bytes >= 6 * 100 + 8 * pl.norm_chunks + 16 * pl.update_chunks
    many = optim_ops.sgd_plan([_item(base, (1, 1, 1, 4096 * 3000), (0, 0, 0, 1), (0, 0, 0, 1))], 1)
    assert many.update_chunks == 3000 and many.update_wgs == 2048 and many.norm_wgs == 750
    # the table is the same bytes for the same list
    again = optim_ops.sgd_plan(items, 2)
    assert torch.equal(again.table_host, pl.table_host)
    for bad, what in ((_item(base, (4, 4, 1, 1), (4, 2, 1, 1), (4, 1, 1, 1)), "parameter is not a dense"),
                      (_item(base, (4, 4, 1, 1), (4, 1, 1, 1), (1, 1, 1, 1)), "gradient is not a dense"),
                      (_item(base, (4, 4, 1, 1), (4, 1, 1, 1), (4, 1, 1, 1), group=2), "group 2"),
                      (_item(base, (1 << 16, 1 << 15, 1, 1), (1 << 15, 1, 1, 1), (1 << 15, 1, 1, 1)), "2\\^31")):
        with pytest.raises(ValueError, match=what):
            optim_ops.sgd_plan([bad], 2)


def test_wrapper_refusals_name_the_argument():
    from torch_detection_amd import optim_ops
    p = torch.zeros(4, 6)
    with pytest.raises(ValueError, match="^params must be a dense float32"):
        optim_ops.sgd_item(p.half(), p.half(), None, 0, name="params")
    with pytest.raises(ValueError, match="^params.grad must be a dense float32"):
        optim_ops.sgd_item(p, p.double(), None, 0, name="params")
    with pytest.raises(ValueError, match="^params must be a dense, non-overlapping"):
        optim_ops.sgd_item(torch.zeros(6).as_strided((4, 6), (0, 1)), p, None, 0, name="params")
    with pytest.raises(ValueError, match="^params must be a dense, non-overlapping"):
        optim_ops.sgd_item(p[:, ::2], p[:, ::2], None, 0, name="params")
    with pytest.raises(ValueError, match="^params.grad must have the parameter's shape"):
        optim_ops.sgd_item(p, p.t(), None, 0, name="params")
    with pytest.raises(ValueError, match="momentum buffer must have the parameter's strides"):
        optim_ops.sgd_item(p, p, p.t().contiguous().t(), 0, name="params")
    with pytest.raises(ValueError, match="^params must be a CUDA tensor"):
        optim_ops.sgd_item(p, p.clone(), None, 0, name="params")
    with pytest.raises(ValueError, match="group must be"):
        optim_ops.sgd_item(p, p, None, -1, name="params")
    with pytest.raises(ValueError, match="params must be float32 CUDA tensors"):
        from torch_detection_amd import SGD
        SGD([torch.nn.Parameter(p)], lr=0.1)
