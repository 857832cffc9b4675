"""CPU: the float64 oracle of the pyramid GroupNorm (tests/pyramid_gn_ref.py) against torch float64 autograd, and the
host-only plan / workspace queries of csrc/pyramid_gn.hip through ctypes."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

import pyramid_gn_ref as R

SIZES = [(9, 8), (5, 4), (3, 2), (1, 1)]


def test_oracle_equals_torch_float64_autograd_over_a_pyramid():
    B, C, G, eps = 2, 16, 4, 1e-5
    g = torch.Generator().manual_seed(5)
    zs = [(torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * (l + 1) + 0.3 * l).requires_grad_(True)
          for l, (H, W) in enumerate(SIZES)]
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.rand(C, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    cots = [torch.randn(B, C, H, W, generator=g, dtype=torch.float64) for H, W in SIZES]
    for relu in (True, False):
        ys = [F.group_norm(z, G, gamma, beta, eps) for z in zs]
        if relu:
            ys = [F.relu(y) for y in ys]
        grads = torch.autograd.grad(ys, zs + [gamma, beta], cots)
        np_ = lambda ts: [t.detach().numpy() for t in ts]
        rys, means, rstds = R.fwd(np_(zs), gamma.detach().numpy(), beta.detach().numpy(), G, eps, relu)
        dzs, dg, db = R.bwd(np_(cots), np_(zs), gamma.detach().numpy(), beta.detach().numpy(), G, eps, relu)
        for l in range(len(SIZES)):
            assert np.allclose(rys[l], ys[l].detach().numpy(), rtol=1e-12, atol=1e-12)
            assert np.allclose(dzs[l], grads[l].numpy(), rtol=1e-10, atol=1e-12)
            zg = zs[l].detach().reshape(B, G, -1)
            assert np.allclose(means[l], zg.mean(-1).numpy(), rtol=1e-12, atol=1e-14)
            assert np.allclose(rstds[l], (zg.var(-1, unbiased=False) + eps).rsqrt().numpy(), rtol=1e-12)
        assert np.allclose(dg, grads[-2].numpy(), rtol=1e-10, atol=1e-12)
        assert np.allclose(db, grads[-1].numpy(), rtol=1e-10, atol=1e-12)


def test_oracle_skips_an_empty_level():
    B, C, G = 2, 8, 2
    g = torch.Generator().manual_seed(6)
    mk = lambda H, W: torch.randn(B, C, H, W, generator=g, dtype=torch.float64).numpy()
    zs, gs = [mk(3, 2), mk(0, 4), mk(1, 1)], [mk(3, 2), mk(0, 4), mk(1, 1)]
    gamma, beta = np.linspace(0.5, 1.5, C), np.linspace(-0.5, 0.5, C)
    dzs, dg, db = R.bwd(gs, zs, gamma, beta, G, 1e-5, True)
    dzs2, dg2, db2 = R.bwd(gs[::2], zs[::2], gamma, beta, G, 1e-5, True)
    assert dzs[1].shape == (B, C, 0, 4) and np.array_equal(dg, dg2) and np.array_equal(db, db2)
    assert np.array_equal(dzs[0], dzs2[0]) and np.array_equal(dzs[2], dzs2[1])


def _lib():
    from torch_detection_amd import _lib
    return _lib.load()


def _hw(sizes):
    return (ctypes.c_int32 * (2 * len(sizes)))(*[v for hw in sizes for v in hw])


def _plan(kind, B, sizes, C, G):
    out = (ctypes.c_int32 * 32)()
    rc = _lib().tdn_pyr_gn_plan(kind, B, _hw(sizes), len(sizes), C, G, out)
    return rc, list(out)


def test_plan_and_workspace_refuse_what_the_kernels_do_not_take():
    lib = _lib()
    ok = [(9, 8), (5, 4)]
    for kind in (0, 1):
        assert _plan(kind, 2, ok, 64, 32)[0] == 0
        assert lib.tdn_pyr_gn_workspace_bytes(kind, 2, _hw(ok), 2, 64, 32) > 0
        for C, G, sizes, what in ((96, 32, ok, b"C=96"), (64, 48, ok, b"do not divide"), (512, 1, ok, b"per group"),
                                  (64, 32, [(2, 2)] * 9, b"num_levels=9"), (1024, 32, ok, b"C=1024")):
            assert _plan(kind, 2, sizes, C, G)[0] != 0
            assert what in lib.tdn_last_error(), (what, lib.tdn_last_error())
            assert lib.tdn_pyr_gn_workspace_bytes(kind, 2, _hw(sizes), len(sizes), C, G) == -1
    assert _plan(2, 2, ok, 64, 32)[0] != 0 and b"kind" in lib.tdn_last_error()
    assert _plan(0, -1, ok, 64, 32)[0] != 0
    assert _plan(0, 2, [(4, -1)], 64, 32)[0] != 0
    # every channels-per-group count of the single-map kernels within the channel set, above 32 included
    for C, G in ((64, 64), (64, 1), (128, 2), (256, 1), (512, 2), (512, 32)):
        assert _plan(0, 2, ok, C, G)[0] == 0, (C, G)


def test_the_cut_is_a_function_of_the_shapes_and_of_each_level_alone():
    sizes = [(37, 41), (9, 8), (1, 1)]
    rc, a = _plan(0, 2, sizes, 64, 32)
    rc2, b = _plan(0, 2, sizes, 64, 32)
    assert rc == rc2 == 0 and a == b
    chunks, px = a[:8], a[8:16]
    assert chunks[3:] == [0] * 5 and px[3:] == [0] * 5
    for l, (H, W) in enumerate(sizes):
        assert chunks[l] >= 1 and (chunks[l] - 1) * px[l] < H * W <= chunks[l] * px[l]     # covers, last chunk not empty
        _, alone = _plan(0, 2, [sizes[l]], 64, 32)
        assert (alone[0], alone[8]) == (chunks[l], px[l])              # the level's cut does not depend on the others
    assert chunks[0] >= 3 and (37 * 41) % px[0] != 0                   # several chunks, a ragged last one
    assert a[16] == 2 * sum(chunks) and a[19] == 3 and a[20] > 0
    # forward and backward cut alike; the backward workspace also holds the per-(level, image) channel sums
    _, bw = _plan(1, 2, sizes, 64, 32)
    assert bw[:16] == a[:16] and bw[22] + (bw[23] << 31) > a[22] + (a[23] << 31)
    lib = _lib()
    for kind, o in ((0, a), (1, bw)):
        assert lib.tdn_pyr_gn_workspace_bytes(kind, 2, _hw(sizes), 3, 64, 32) == o[22] + (o[23] << 31)
    # the batch size enters the rule: at most about 1024 workgroups per level
    _, big = _plan(0, 512, sizes, 64, 32)
    assert big[0] == 2


def test_a_single_level_is_cut_like_the_single_map_kernels():
    """A one-level plan reports the `chunks` that tdn_gn_workspace(B, H, W, C, G) implies: its size is
    256 + 4 * (B * chunks * 2 * C + 3 * B * C) bytes (the layout restated in tests/test_norm_oracle.py), solved for chunks."""
    lib = _lib()
    for B, H, W, C, G in ((2, 6, 10, 64, 32), (1, 37, 41, 64, 32), (2, 3, 2, 512, 2), (512, 9, 8, 64, 32),
                          (1, 1, 1, 256, 32)):
        size = lib.tdn_gn_workspace(B, H, W, C, G)
        assert size > 0 and (size - 256 - B * C * 12) % (B * 2 * C * 4) == 0, (B, H, W, C, G)
        rc, plan = _plan(0, B, [(H, W)], C, G)
        assert rc == 0 and plan[0] == (size - 256 - B * C * 12) // (B * 2 * C * 4), (B, H, W, C, G)


def test_an_empty_level_contributes_no_chunks():
    full = [(9, 8), (5, 4), (3, 2)]
    hole = [(9, 8), (0, 4), (3, 2)]
    _, a = _plan(1, 2, [full[0], full[2]], 64, 32)
    _, b = _plan(1, 2, hole, 64, 32)
    assert b[1] == 0 and b[9] == 0 and (b[0], b[2]) == (a[0], a[1]) and b[16] == a[16] and b[18] == a[18]
    _, none = _plan(0, 2, [(0, 0)], 64, 32)
    assert none[16:20] == [0, 0, 0, 0] and none[22] == 0
    _, noneb = _plan(1, 0, full, 64, 32)
    assert noneb[16:20] == [0, 0, 1, 1]                                 # only the launch that writes the zero sums
    assert _lib().tdn_pyr_gn_workspace_bytes(0, 2, _hw([(0, 0)]), 1, 64, 32) == 0
