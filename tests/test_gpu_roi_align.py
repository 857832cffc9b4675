"""GPU tests of multi-level RoIAlign (roi_align, map_roi_levels, SingleRoIExtractor, rois_from_proposals) against
the CPU oracle (tests/roi_ref.py)."""
import numpy as np
import pytest
import torch

import roi_ref as R

pytestmark = pytest.mark.gpu

STRIDES = (4, 8, 16, 32)
C4 = [(200, 336), (100, 168), (50, 84), (25, 42)]          # 800 x 1344


@pytest.fixture(scope="module")
def T():
    assert torch.cuda.is_available()
    import torch_detection_amd
    return torch_detection_amd


def feats_of(B, C, shapes, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, C, h, w, generator=g) * scale).to(dtype).cuda().contiguous(
        memory_format=torch.channels_last) for h, w in shapes]


def mixed_rois(n, B, seed, canvas=(800, 1344)):
    """A realistic scale mix over every level, plus degenerate, out-of-image and invalid-batch rows."""
    g = np.random.default_rng(seed)
    side = np.exp(g.uniform(np.log(8), np.log(900), (n, 2)))
    x1 = g.uniform(-0.1 * canvas[1], canvas[1], n)
    y1 = g.uniform(-0.1 * canvas[0], canvas[0], n)
    rois = np.stack([g.integers(0, B, n), x1, y1, x1 + side[:, 0], y1 + side[:, 1]], 1).astype(np.float32)
    k = n // 20
    rois[:k, 3] = rois[:k, 1] - 1                        # zero '+1' width
    rois[k:2 * k, 3] = rois[k:2 * k, 1] - 5              # negative width
    rois[2 * k:3 * k, 1:] += np.float32(5000)            # far outside
    rois[3 * k:4 * k, 0] = -1                            # padding rows
    rois[4 * k:4 * k + 3, 0] = [B, 1e9, np.nan]
    return rois


def np_feats(fs):
    return [f.float().cpu().numpy() for f in fs]


def to16(ref, dtype):
    return torch.from_numpy(np.ascontiguousarray(ref)).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("S,sr", [(7, 2), (7, 0), (14, 2), (14, 0)])
def test_forward_bit_identical_to_oracle(T, dtype, S, sr):
    B, C = 2, 32
    fs = feats_of(B, C, C4, dtype, 1)
    rois = mixed_rois(1000, B, 2)
    out = T.roi_align(fs, torch.from_numpy(rois).cuda(), S, STRIDES, sr)
    assert out.shape == (1000, C, S, S) and out.dtype == dtype
    assert out.permute(0, 2, 3, 1).is_contiguous()
    ref = to16(R.roi_align_forward(np_feats(fs), rois, STRIDES, S, sr), dtype)
    got = out.cpu()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert int((got != 0).flatten(1).any(1).sum()) > 700          # zero-width rows with sr = 0 have no samples


def test_forward_bit_identical_256_channels(T):
    B, C = 2, 256
    fs = feats_of(B, C, C4, torch.bfloat16, 3)
    rois = mixed_rois(400, B, 4)
    out = T.roi_align(fs, torch.from_numpy(rois).cuda()).cpu()
    ref = to16(R.roi_align_forward(np_feats(fs), rois, STRIDES, 7, 2), torch.bfloat16)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))


def test_map_roi_levels_bit_identical(T):
    rois = mixed_rois(5000, 2, 5)
    for L in (1, 3, 4, 8):
        got = T.map_roi_levels(torch.from_numpy(rois).cuda(), L).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, R.map_levels(rois, L))
    assert len(np.unique(R.map_levels(rois, 4))) == 4


def _grads(T, fs, rois_t, dout, S, sr):
    leaves = [f.detach().requires_grad_(True) for f in fs]
    out = T.roi_align(leaves, rois_t, S, STRIDES, sr)
    return torch.autograd.grad(out, leaves, dout)


@pytest.mark.parametrize("dtype,S,sr", [(torch.bfloat16, 7, 2), (torch.float16, 14, 0)])
def test_backward_matches_float64_oracle(T, dtype, S, sr):
    B, C = 2, 32
    shapes = [(100, 168), (50, 84), (25, 42), (13, 21)]   # a 400 x 672 image: more rows per pixel
    fs = feats_of(B, C, shapes, dtype, 6)
    rois = mixed_rois(600, B, 7, canvas=(400, 672))
    rois_t = torch.from_numpy(rois).cuda()
    g = torch.Generator().manual_seed(8)
    dout = torch.randn(len(rois), C, S, S, generator=g).to(dtype).cuda()
    grads = _grads(T, fs, rois_t, dout, S, sr)
    ref, n, absum = R.roi_align_backward([(B, C, h, w) for h, w in shapes], rois, dout.float().cpu().numpy(),
                                         STRIDES, S, sr)
    for l, (gr, rf, nn, ab) in enumerate(zip(grads, ref, n, absum)):
        assert gr.dtype == dtype and gr.shape == (B, C) + shapes[l]
        assert gr.permute(0, 2, 3, 1).is_contiguous()
        got = gr.double().cpu().numpy()
        sp = np.spacing(np.abs(rf).astype(np.float32).astype(np.float16 if dtype == torch.float16 else np.float32))
        if dtype == torch.bfloat16:
            sp = np.spacing(np.abs(rf).astype(np.float32)) * 65536.0
        tol = sp.astype(np.float64) + nn * 2.0 ** -23 * ab
        assert np.all(np.abs(got - rf) <= tol), (l, np.max(np.abs(got - rf) - tol))
        assert np.all(got[np.broadcast_to(nn == 0, got.shape)] == 0)       # untouched pixels are exactly 0
    # invalid rows add nothing: the same gradients, bit for bit, without them
    valid = np.array([R.batch_index(v, B) >= 0 for v in rois[:, 0]])
    keep = torch.from_numpy(np.nonzero(valid)[0]).cuda()
    alone = _grads(T, fs, rois_t[keep].contiguous(), dout[keep].contiguous(), S, sr)
    for a, b in zip(grads, alone):
        assert torch.equal(a, b)


def test_adjoint_on_the_gpu(T):
    """Dyadic RoIs (corners on multiples of 32 px, sides of 64..256 px, S = 2, two samples per side: every sample on
    a quarter-pixel grid of every level), features and cotangents in {-1, 0, 1}: every forward output and every
    gradient is exact in fp16, so <fwd(f), g> == <f, bwd(g)> holds to fp32 accuracy."""
    B, C, S = 2, 16, 2
    shapes = [(40, 64), (20, 32), (10, 16), (5, 8)]
    g = np.random.default_rng(9)
    n = 40
    x1 = g.integers(0, 8, n) * 32.0
    y1 = g.integers(0, 5, n) * 32.0
    side = g.choice([64, 128, 256], (n, 2)) * 1.0
    rois = np.stack([g.integers(0, B, n), x1, y1, x1 + side[:, 0] - 1, y1 + side[:, 1] - 1], 1).astype(np.float32)
    assert len(np.unique(R.map_levels(rois, 4))) >= 3
    fs = [torch.from_numpy(g.integers(-1, 2, (B, C, h, w)).astype(np.float32)).half().cuda()
          .contiguous(memory_format=torch.channels_last) for h, w in shapes]
    leaves = [f.detach().requires_grad_(True) for f in fs]
    out = T.roi_align(leaves, torch.from_numpy(rois).cuda(), S, STRIDES, 2)
    dout = torch.from_numpy(g.integers(-1, 2, tuple(out.shape)).astype(np.float32)).half().cuda()
    grads = torch.autograd.grad(out, leaves, dout)
    out = out.detach()
    lhs = float((out.double() * dout.double()).sum())
    rhs = float(sum((f.double() * gr.double()).sum() for f, gr in zip(fs, grads)))
    assert abs(lhs) > 1 and abs(lhs - rhs) <= 2.0 ** -23 * abs(lhs), (lhs, rhs)
    ref = R.roi_align_forward(np_feats(fs), rois, STRIDES, S, 2, exact64=True)
    assert np.array_equal(out.double().cpu().numpy(), ref)                 # the construction is exact
    gref, _, _ = R.roi_align_backward([tuple(f.shape) for f in fs], rois, dout.double().cpu().numpy(), STRIDES, S, 2)
    assert all(np.array_equal(a.double().cpu().numpy(), b) for a, b in zip(grads, gref))


def test_two_eager_calls_and_graph_replay_are_byte_identical(T):
    B, C, S = 2, 256, 7
    fs = feats_of(B, C, C4, torch.bfloat16, 10)
    rois_t = torch.from_numpy(mixed_rois(1024, B, 11)).cuda()
    dout = torch.randn(1024, C, S, S, generator=torch.Generator().manual_seed(12)).bfloat16().cuda()
    leaves = [f.detach().requires_grad_(True) for f in fs]

    def step():     # nothing of the autograd graph outlives the call: a captured backward may not join a live one
        out = T.roi_align(leaves, rois_t, S, STRIDES, 2)
        return (out.detach(),) + torch.autograd.grad(out, leaves, dout)

    a = step()
    b = step()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        c = step()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, c):
        assert torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16))


def test_fpn_chain_backward(T):
    B = 2
    fpn = T.FPN([64, 128, 256, 512], 256, 5).cuda()
    g = torch.Generator().manual_seed(13)
    xs = [torch.randn(B, c, 128 // s, 192 // s, generator=g).cuda() for c, s in ((64, 4), (128, 8), (256, 16),
                                                                                  (512, 32))]
    rois = torch.from_numpy(mixed_rois(200, B, 14, canvas=(128, 192))).cuda()
    ext = T.SingleRoIExtractor(dict(type='RoIAlign', out_size=7, sample_num=2), 256, [4, 8, 16, 32])
    assert len(list(ext.parameters())) == 0
    feats = fpn(xs)
    out = ext(feats, rois)
    dout = torch.randn(tuple(out.shape), generator=g).to(out.dtype).cuda()
    params = list(fpn.parameters())
    g_chain = torch.autograd.grad(out, params, dout)
    # the cotangents the extractor hands to the FPN: NHWC 16-bit, and P6 gets none
    feats = fpn(xs)
    leaves = [f.detach().requires_grad_(True) for f in feats[:4]]
    cots = torch.autograd.grad(ext(leaves + [feats[4].detach()], rois), leaves, dout)
    for c, f in zip(cots, feats):
        assert c.dtype == f.dtype and c.shape == f.shape and c.permute(0, 2, 3, 1).is_contiguous()
    g_direct = torch.autograd.grad(feats[:4], params, cots)
    for a, b in zip(g_chain, g_direct):
        assert torch.equal(a, b)


def test_proposals_to_extractor_in_one_graph(T):
    levels = [((50, 84), 4), ((25, 42), 8), ((13, 21), 16), ((7, 11), 32)]
    gens = [T.AnchorGenerator(st, [8], [0.5, 1.0, 2.0]) for _, st in levels]
    anchors, _ = T.anchor_pyramid(gens, [fs for fs, _ in levels], [st for _, st in levels], "cuda")
    B = 2
    g = torch.Generator().manual_seed(15)
    cls = [torch.randn(B, 3, h, w, generator=g).bfloat16().cuda() for (h, w), _ in levels]
    reg = [(torch.randn(B, 12, h, w, generator=g) * 0.5).bfloat16().cuda() for (h, w), _ in levels]
    ish = torch.tensor([(200, 336), (180, 300)], dtype=torch.int32).cuda()
    fs = feats_of(B, 64, [fs for fs, _ in levels], torch.bfloat16, 16)
    ext = T.SingleRoIExtractor(out_channels=64)

    def run():
        props, _, counts = T.rpn_proposals(cls, reg, anchors, ish, nms_pre=300, nms_post=300, max_num=200)
        rois = T.rois_from_proposals(props, counts)
        return props, counts, rois, ext(fs, rois)

    eager = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        graphed = run()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)
    props, counts, rois = (t.cpu().numpy() for t in eager[:3])
    assert rois.shape == (B * 200, 5)
    for b in range(B):
        rows = rois[b * 200:(b + 1) * 200]
        assert np.array_equal(rows[:, 1:], props[b, :, :4])
        assert np.all(rows[:counts[b], 0] == b) and np.all(rows[counts[b]:, 0] == -1)
    ref = to16(R.roi_align_forward(np_feats(fs), rois, STRIDES, 7, 2), torch.bfloat16)
    assert torch.equal(eager[3].cpu().view(torch.int16), ref.view(torch.int16))


def test_empty_one_level_and_nchw_features(T):
    B, C = 2, 16
    fs = feats_of(B, C, [(30, 40)], torch.float16, 17)
    rois = mixed_rois(100, B, 18, canvas=(120, 160))
    rois_t = torch.from_numpy(rois).cuda()
    out = T.roi_align(fs, rois_t, 5, (4,), 0)
    ref = to16(R.roi_align_forward(np_feats(fs), rois, (4,), 5, 0), torch.float16)
    assert torch.equal(out.cpu().view(torch.int16), ref.view(torch.int16))
    # NCHW-contiguous 16-bit features go through the transpose: same result and gradients
    nchw = [f.contiguous() for f in fs]
    assert not nchw[0].permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(T.roi_align(nchw, rois_t, 5, (4,), 0), out)
    dout = torch.randn(tuple(out.shape), generator=torch.Generator().manual_seed(19)).half().cuda()
    ga = _grads_levels(T, fs, rois_t, dout, (4,))
    gb = _grads_levels(T, nchw, rois_t, dout, (4,))
    assert torch.equal(ga[0], gb[0])
    # R = 0: an empty output, zero gradients
    empty = torch.zeros(0, 5, dtype=torch.float32, device="cuda")
    leaves = [f.detach().requires_grad_(True) for f in feats_of(B, C, C4[2:], torch.bfloat16, 20)]
    out0 = T.roi_align(leaves, empty, 7, (16, 32))
    assert out0.shape == (0, C, 7, 7)
    g0 = torch.autograd.grad(out0, leaves, torch.zeros_like(out0))
    assert all(int(t.abs().sum()) == 0 and t.shape == f.shape for t, f in zip(g0, leaves))


def _grads_levels(T, fs, rois_t, dout, strides):
    leaves = [f.detach().requires_grad_(True) for f in fs]
    return torch.autograd.grad(T.roi_align(leaves, rois_t, dout.shape[2], strides, 0), leaves, dout)


def test_bad_inputs_raise_before_any_launch(T):
    B, C = 2, 16
    fs = feats_of(B, C, C4[:2], torch.bfloat16, 21)
    rois = torch.from_numpy(mixed_rois(10, B, 22)).cuda()
    bad = [
        (lambda: T.roi_align([f.float() for f in fs], rois, 7, (4, 8)),
         r"feats\[0\] must be a bfloat16 / float16"),                                               # fp32 features
        (lambda: T.roi_align([f.cpu() for f in fs], rois, 7, (4, 8)), r"feats\[0\] must be a CUDA tensor"),  # CPU features
        (lambda: T.roi_align([fs[0], fs[1].half()], rois, 7, (4, 8)),
         r"feats\[1\] must be a bfloat16 .* got float16"),                                          # mixed dtypes
        (lambda: T.roi_align([fs[0], fs[1][:1]], rois, 7, (4, 8)),
         r"feats\[1\] must be a bfloat16 \(2, 16, H, W\)"),                                         # mismatched batch
        (lambda: T.roi_align([fs[0], fs[1][:, :8]], rois, 7, (4, 8)),
         r"feats\[1\] must be a bfloat16 \(2, 16, H, W\)"),                                         # mismatched channels
        (lambda: T.roi_align([f[:, :12] for f in fs], rois, 7, (4, 8)), "C a positive multiple of 8"),  # C % 8
        (lambda: T.roi_align(fs, rois, 7, (4, 8, 16)), "2 feature levels but 3 featmap strides"),     # levels vs strides
        (lambda: T.roi_align(fs, rois, 17, (4, 8)), "out_size must be in 1..16"),                     # out_size
        (lambda: T.roi_align(fs, rois, 7, (4, 8), -1), "sampling_ratio must be in 0..512"),           # sampling_ratio
        (lambda: T.roi_align(fs, rois, 7, (4, 8), 2, 0), "finest_scale must be finite and > 0"),      # finest_scale
        (lambda: T.roi_align(fs, rois[:, 1:].contiguous(), 7, (4, 8)),
         r"rois must be a contiguous float32 \(R, 5\)"),                                             # (R, 4) rois
        (lambda: T.roi_align(fs, rois.double(), 7, (4, 8)), r"rois must be a contiguous float32 \(R, 5\)"),
        (lambda: T.roi_align(fs, rois.cpu(), 7, (4, 8)), "rois must be a CUDA tensor"),
        (lambda: T.roi_align(fs, rois.t().contiguous().t(), 7, (4, 8)),
         r"rois must be a contiguous float32 \(R, 5\)"),                                             # not contiguous
        (lambda: T.map_roi_levels(rois, 9), "num_levels must be in 1..8"),
        (lambda: T.SingleRoIExtractor(dict(type='RoIPool', out_size=7)), "roi_layer type 'RoIAlign' only"),
        (lambda: T.SingleRoIExtractor(out_channels=32)(fs + fs, rois), "out_channels is 32"),
        (lambda: T.rois_from_proposals(torch.zeros(2, 10, 4, device="cuda"),
                                       torch.zeros(2, dtype=torch.int32, device="cuda")),
         r"proposals must be a contiguous float32 \(B, M, 5\)"),
        (lambda: T.rois_from_proposals(torch.zeros(2, 10, 5, device="cuda"),
                                       torch.zeros(3, dtype=torch.int32, device="cuda")),
         r"counts must be a contiguous int32 \(2,\)"),
    ]
    for i, (fn, msg) in enumerate(bad):
        with pytest.raises(ValueError, match=msg):
            fn()
            pytest.fail("case %d did not raise" % i)
