"""The memory guard of tests/guard_util.py checks itself on host tensors, so that a clean GPU run means something.
Every "overrun" here is an index into the guard's own base buffer made from Python: no memory error of any kind."""
import types

import pytest
import torch

import guard_util as G

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64, torch.uint8]


def _rec(g, t):
    return next(r for r in g.recs if r.tensor is t)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_alignment_and_poison(dtype):
    g = G.GuardAlloc()
    t = g.alloc((3, 5, 7), dtype, "cpu", label="op: out")
    assert t.shape == (3, 5, 7) and t.dtype == dtype and t.is_contiguous()
    assert t.data_ptr() % 512 == 0
    r = _rec(g, t)
    assert r.off >= G.BAND_MIN and r.buf.numel() - r.off - r.nbytes >= G.BAND_MIN
    if dtype.is_floating_point:
        assert bool(t.float().isnan().all())
    else:
        assert bool((t.view(torch.uint8) == 0x5A).all())
        assert not bool((t == -1).any()) and not bool((t == 0).any()) and not bool((t == 1).any())
    found = g.check()                   # nothing written: bands clean, every element still poison
    assert len(found) == 1 and "105 of 105 elements never written" in found[0] and found[0].startswith("op: out")


def test_band_is_at_least_one_image_row():
    g = G.GuardAlloc()
    t = g.alloc((1, 2, 1400, 512), torch.float32, "cpu")     # a row of 1400 x 512 floats is 2.7 MiB
    r = _rec(g, t)
    assert r.off >= 1400 * 512 * 4 and r.buf.numel() - r.off - r.nbytes >= 1400 * 512 * 4
    assert t.data_ptr() % 512 == 0


def test_clean_run_reports_nothing():
    g = G.GuardAlloc()
    a = g.alloc((4, 9), torch.float32, "cpu")
    b = g.alloc((17,), torch.uint8, "cpu")
    c = g.alloc((0, 4), torch.float32, "cpu")
    z = g.alloc((5,), torch.int32, "cpu", interior="zero")
    a.copy_(torch.arange(36.0).view(4, 9))
    b.fill_(1)
    assert c.numel() == 0 and int(z.abs().sum()) == 0
    assert g.check() == []
    assert g.recs == [] and g.check() == []


def test_byte_just_before_the_payload_is_reported():
    g = G.GuardAlloc()
    t = g.alloc((30,), torch.uint8, "cpu", label="op: y")
    t.fill_(0)
    r = _rec(g, t)
    r.buf[r.off - 1] = 0
    found = g.check()
    assert found == ["op: y: 1 bytes changed in the LOWER band, payload offsets -1 .. -1"]


def test_byte_just_after_the_payload_is_reported():
    g = G.GuardAlloc()
    t = g.alloc((15,), torch.bfloat16, "cpu", label="op: y")       # 30 bytes: the next byte is NOT 512-aligned
    t.fill_(1.0)
    r = _rec(g, t)
    r.buf[r.off + 30] = 0
    found = g.check()
    assert len(found) == 1 and "1 bytes changed in the UPPER band, payload offsets 30 .. 30" in found[0]


def test_byte_at_the_far_end_of_a_band_is_reported():
    for where in ("low", "high"):
        g = G.GuardAlloc()
        t = g.alloc((8, 8), torch.float32, "cpu")
        t.zero_()
        r = _rec(g, t)
        if where == "low":
            r.buf[0] = 7
            off = -r.off
        else:
            r.buf[r.buf.numel() - 1] = 7
            off = r.buf.numel() - 1 - r.off
        found = g.check()
        assert len(found) == 1 and ("payload offsets %d .. %d" % (off, off)) in found[0]
        assert abs(off) >= G.BAND_MIN


def test_first_and_last_offending_offsets():
    g = G.GuardAlloc()
    t = g.alloc((64,), torch.float32, "cpu")
    t.zero_()
    r = _rec(g, t)
    r.buf[r.off + 256 + 3] = 0
    r.buf[r.off + 256 + 700] = 0
    found = g.check()
    assert len(found) == 1 and "2 bytes changed in the UPPER band, payload offsets 259 .. 956" in found[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_unwritten_element_is_reported(dtype):
    g = G.GuardAlloc()
    t = g.alloc((2, 3, 4), dtype, "cpu", label="op: out")
    keep = t.flatten()[17].clone()
    t.fill_(1)
    t.flatten()[17] = keep
    found = g.check()
    assert len(found) == 1 and "1 of 24 elements never written" in found[0]
    assert "flat index 17 = (1, 1, 1) of (2, 3, 4)" in found[0]


def test_int64_minus_one_counts_as_written():
    g = G.GuardAlloc()
    t = g.alloc((100,), torch.int64, "cpu")          # tdn_nms pads kept_idx with -1
    t.fill_(-1)
    assert g.check() == []
    t = g.alloc((100,), torch.int64, "cpu")
    t[:40] = torch.arange(40)
    t[40:99] = -1                                    # ... and an unwritten tail element is still seen
    found = g.check()
    assert len(found) == 1 and "1 of 100 elements never written" in found[0] and "flat index 99" in found[0]


def test_not_must_write_and_zero_interior_are_not_reported():
    g = G.GuardAlloc()
    g.alloc((10,), torch.float32, "cpu", must_write=False)
    g.alloc((10,), torch.int32, "cpu", interior="zero")
    g.alloc((10,), torch.float32, "cpu", interior=2.5)
    assert g.check() == []


def test_shortened_payload_turns_the_last_row_into_band():
    g = G.GuardAlloc()
    t = g.alloc((4, 6), torch.float32, "cpu", label="op: out")
    t.copy_(torch.arange(24.0).view(4, 6) + 1)        # a legitimate, complete write
    g.shorten(t, 3 * 6 * 4)
    found = g.check()
    assert len(found) == 1 and "UPPER band, payload offsets 72 .. 95" in found[0]


def test_guard_copy_keeps_values_and_has_nan_bands():
    g = G.GuardAlloc()
    src = torch.arange(24.0).view(2, 3, 4).bfloat16()
    c = g.guard_copy(src)
    assert torch.equal(c, src) and c.is_contiguous() and c.data_ptr() % 512 == 0
    r = _rec(g, c)
    before = r.buf[r.off - 2:r.off].view(torch.bfloat16)
    after = r.buf[r.off + r.nbytes:r.off + r.nbytes + 2].view(torch.bfloat16)
    assert bool(before.float().isnan().all()) and bool(after.float().isnan().all())
    assert g.check() == []


def test_workspace_is_exact_fresh_and_poisoned():
    g = G.GuardAlloc()
    w1 = g.workspace(1000, "cpu", 16, "gn_fwd")
    w2 = g.workspace(1000, "cpu", 256, "nms")
    assert w1.numel() == 1008 and w2.numel() == 1024 and w1.data_ptr() % 512 == 0 and w2.data_ptr() % 512 == 0
    assert w1.data_ptr() != w2.data_ptr()
    assert bool(w1[:1008 // 4 * 4].view(torch.float32).isnan().all())
    assert g.ws_log == [("gn_fwd", 1000, 1008), ("nms", 1000, 1024)] and g.ws_calls["nms"] == 1
    r = _rec(g, w1)
    r.buf[r.off + 1008] = 0                            # one byte past the exact size
    found = g.check()
    assert len(found) == 1 and found[0].startswith("gn_fwd: workspace") and "offsets 1008 .. 1008" in found[0]
    assert len(g.retired) == 2                         # kept referenced until the next check has synchronised


def _fake_ops(tmp_path):
    src = tmp_path / "fakeops.py"
    src.write_text(
        "import torch\n"
        "def _helper(n, dev):\n"
        "    o1 = torch.empty(n, 3, dtype=torch.bfloat16, device=dev)\n"
        "    return o1\n"
        "def op(n, dev='cpu'):\n"
        "    y = _helper(n, dev)\n"
        "    keep = torch.zeros(n, dtype=torch.uint8, device=dev)\n"
        "    like = torch.empty_like(y)\n"
        "    f = torch.full((n,), 7, dtype=torch.int64, device=dev)\n"
        "    ws = _workspace(100, dev)\n"
        "    return y, keep, like, f, ws\n"
        "def nms(n, dev='cpu'):\n"
        "    ws, wp = _aligned_ws(n, dev)\n"
        "    return ws\n"
        "def _workspace(nbytes, device):\n"
        "    return torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)\n"
        "def _aligned_ws(nbytes, dev):\n"
        "    return None, None\n")
    mod = types.ModuleType("fakeops")
    mod.__file__ = str(src)
    exec(compile(src.read_text(), str(src), "exec"), mod.__dict__)
    return mod


def test_proxy_guards_allocations_and_names_them(tmp_path, monkeypatch):
    mod = _fake_ops(tmp_path)
    g = G.GuardAlloc()
    proxy = G.install(monkeypatch, mod, g)
    assert mod.torch is proxy
    y, keep, like, f, ws = mod.op(5)
    assert y.shape == (5, 3) and y.dtype == torch.bfloat16 and bool(y.float().isnan().all())
    assert int(keep.sum()) == 0 and bool(like.float().isnan().all()) and f.tolist() == [7] * 5
    assert ws.numel() == 112 and ws.dtype == torch.uint8               # exactly 100 bytes, rounded up to 16
    assert [r.label.split("@")[0] for r in g.recs] == ["op: o1", "op: keep", "op: like", "op: f", "op: workspace"]
    assert g.calls["op"] == 4 and g.ws_calls["op"] == 1
    found = g.check()                  # y and like are never written; zeros / full / workspace are not "must write"
    assert len(found) == 2 and found[0].startswith("op: o1@3") and found[1].startswith("op: like@8")
    w = mod.nms(1000)                  # the workspace of ops.nms: exact, 256-aligned size, no slack
    assert w.numel() == 1024 and g.ws_log[-1] == ("nms", 1000, 1024) and g.check() == []


def test_proxy_leaves_every_other_attribute_alone():
    proxy = G.TorchProxy(G.GuardAlloc(), __file__)
    own = {"empty", "empty_like", "zeros", "full"}
    for name in dir(torch):
        if name in own or name.startswith("__"):
            continue
        assert getattr(proxy, name) is getattr(torch, name), name
    assert proxy.cuda is torch.cuda and proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor
    for name in own:
        assert getattr(proxy, name) is not getattr(torch, name)
    with pytest.raises(AttributeError):
        proxy.no_such_attribute


def test_install_is_undone_with_the_fixture(tmp_path):
    mod = _fake_ops(tmp_path)
    real_ws = mod._workspace
    mp = pytest.MonkeyPatch()
    G.install(mp, mod, G.GuardAlloc())
    assert mod.torch is not torch
    mp.undo()
    assert mod.torch is torch and mod._workspace is real_ws
