"""CPU: known answers of the multi-level RoIAlign oracle (tests/roi_ref.py), its adjointness and the
C-ABI layout of the new structs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import roi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
STRIDES = (4, 8, 16, 32)
SHAPES = [(50, 84), (25, 42), (13, 21), (7, 11)]          # a 200 x 336 image


def pyramid(B, C, fill):
    return [np.stack([np.stack([fill(h, w, b, c) for c in range(C)]) for b in range(B)]).astype(f32)
            for h, w in SHAPES]


def rand_rois(n, seed, B=2, lo=4.0, hi=200.0, canvas=(200, 336), spill=0.0):
    g = np.random.default_rng(seed)
    wh = g.uniform(lo, hi, (n, 2))
    x1 = g.uniform(-spill * hi, canvas[1] - wh[:, 0] * (1 - spill), n)
    y1 = g.uniform(-spill * hi, canvas[0] - wh[:, 1] * (1 - spill), n)
    b = g.integers(0, B, n)
    return np.stack([b, x1, y1, x1 + wh[:, 0], y1 + wh[:, 1]], 1).astype(f32)


def test_constant_map_gives_the_constant():
    feats = pyramid(2, 8, lambda h, w, b, c: np.full((h, w), 1.5 + c))
    rois = rand_rois(300, 0)
    for sr, S in ((2, 7), (0, 7), (1, 14)):
        out = R.roi_align_forward(feats, rois, STRIDES, S, sr)
        want = (1.5 + np.arange(8, dtype=f32))[None, :, None, None]
        assert np.all(np.abs(out - want) <= 8 * np.spacing(want)), (sr, S)


def _expected_linear(roi, stride, S, sr, H, W, a, b):
    """Mean over a bin's samples of a*x + b*y at the clamped sample positions (0 outside [-1, n]), float64."""
    x1, y1, x2, y2 = (float(v) for v in roi)
    sc = 1.0 / stride
    sw, sh = x1 * sc, y1 * sc
    bw, bh = max((x2 + 1) * sc - sw, 0) / S, max((y2 + 1) * sc - sh, 0) / S
    gw = sr if sr > 0 else int(np.ceil(bw))
    gh = sr if sr > 0 else int(np.ceil(bh))
    out = np.zeros((S, S))
    for ph in range(S):
        for pw in range(S):
            acc = 0.0
            for iy in range(gh):
                y = sh + ph * bh + (iy + 0.5) * bh / gh
                for ix in range(gw):
                    x = sw + pw * bw + (ix + 0.5) * bw / gw
                    if y < -1 or y > H or x < -1 or x > W:
                        continue
                    acc += a * min(max(x, 0), W - 1) + b * min(max(y, 0), H - 1)
            out[ph, pw] = acc / max(gh * gw, 1)
    return out


def test_linear_map_gives_the_mean_sample_position_at_borders_and_outside():
    a, b = 1.0, 2.0
    feats = pyramid(1, 8, lambda h, w, bb, c: a * np.arange(w)[None, :] + b * np.arange(h)[:, None])
    rois = np.array([[0, 10, 20, 60, 70],                  # inside, level 0
                     [0, -30, -20, 40, 30],                # over the top-left corner: x, y < -1 and in [-1, 0)
                     [0, 300, 170, 360, 215],              # over the bottom-right: clamp at W-1 / H-1 and x > W
                     [0, 100, 50, 299, 199],               # level 2
                     [0, 150, 60, 155.5, 64],              # tiny: 4 samples per bin on 1.5 px
                     [0, -500, -400, -200, -100]],         # entirely outside: zeros
                    f32)
    levels = R.map_levels(rois, 4)
    for sr in (2, 0, 3):
        out = R.roi_align_forward(feats, rois, STRIDES, 7, sr)
        for r in range(len(rois)):
            lv = int(levels[r])
            H, W = SHAPES[lv]
            want = _expected_linear(rois[r, 1:], STRIDES[lv], 7, sr, H, W, a, b)
            assert np.allclose(out[r, 0], want, rtol=2e-6, atol=2e-5), (sr, r)
    assert np.array_equal(out[5], np.zeros_like(out[5]))


def test_level_boundaries():
    rows = []
    for side in (56, 111.9, 112, 223.9, 224, 447.9, 448, 1000, 20):
        rows.append([0, 10, 10, 10 + side - 1, 10 + side - 1])
    got = R.map_levels(np.array(rows, f32), 4)
    assert got.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 0]
    assert R.map_levels(np.array(rows, f32), 2).tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0]
    # degenerate boxes (x2 < x1 - 1: negative '+1' width) map to 0, as do non-finite ones
    bad = np.array([[0, 10, 10, 5, 50], [0, 0, 0, np.inf, 10], [0, 0, 0, np.nan, 10]], f32)
    assert R.map_levels(bad, 4).tolist() == [0, 0, 0]


def test_levels_agree_with_torch_log2_away_from_powers_of_two():
    rois = rand_rois(5000, 3, lo=2, hi=900, canvas=(1000, 1400))
    ours = R.map_levels(rois, 4)
    t = torch.from_numpy(rois)
    scale = torch.sqrt((t[:, 3] - t[:, 1] + 1) * (t[:, 4] - t[:, 2] + 1))
    s = scale / 56 + 1e-6
    ref = torch.floor(torch.log2(s)).clamp(min=0, max=3).long().numpy()
    near = np.abs(np.log2(s.numpy()) - np.round(np.log2(s.numpy()))) < 1e-5
    assert np.array_equal(ours[~near], ref[~near])
    assert len(np.unique(ours)) == 4


def test_invalid_batch_rows_give_zeros():
    feats = pyramid(2, 8, lambda h, w, b, c: np.ones((h, w)))
    rois = rand_rois(6, 4)
    rois[:, 0] = [0, -1, 2, 1.7, -0.5, np.nan]          # (int)1.7 = 1, (int)-0.5 = 0 are valid
    out = R.roi_align_forward(feats, rois, STRIDES, 7, 2)
    assert [bool(np.any(out[r])) for r in range(6)] == [True, False, False, True, True, False]


def test_backward_is_the_adjoint_of_the_forward_in_float64():
    g = np.random.default_rng(5)
    feats = [g.standard_normal((2, 16, h, w)) for h, w in SHAPES]
    rois = rand_rois(150, 6, spill=0.3)
    rois[::17, 0] = -1
    for sr, S in ((2, 7), (0, 5)):
        out = R.roi_align_forward(feats, rois, STRIDES, S, sr, exact64=True)
        dout = g.standard_normal(out.shape)
        grads, n, absum = R.roi_align_backward([f.shape for f in feats], rois, dout, STRIDES, S, sr)
        lhs = float((out * dout).sum())
        rhs = float(sum((f * gr).sum() for f, gr in zip(feats, grads)))
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
        assert all(np.all(a >= np.abs(gr)) for a, gr in zip(absum, grads))
        assert all(np.all((nn == 0) <= (gr == 0)) for nn, gr in zip(n, grads))


def test_roi_struct_mirrors_match_the_header(tmp_path):
    """sizeof / offsetof of tdn_roi_level and tdn_roi_config as gcc lays them out == the ctypes mirrors."""
    from torch_detection_amd import _lib
    mirrors = {"tdn_roi_level": _lib.RoiLevel, "tdn_roi_config": _lib.RoiConfig}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "tdn.h"', 'int main(void) {']
    for cname, cls in mirrors.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['printf("const LVL %d\\n", TDN_ROI_MAX_LEVELS);', 'printf("const OUT %d\\n", TDN_ROI_MAX_OUT);',
              'printf("const SMP %d\\n", TDN_ROI_MAX_SAMPLES);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    consts = {"LVL": _lib.ROI_MAX_LEVELS, "OUT": _lib.ROI_MAX_OUT, "SMP": _lib.ROI_MAX_SAMPLES}
    seen = 0
    for ln in subprocess.check_output([str(exe)]).decode().split("\n"):
        if not ln:
            continue
        cname, fname, val = ln.split()
        if cname == "const":
            assert consts[fname] == int(val), (fname, val)
            continue
        cls = mirrors[cname]
        got = ctypes.sizeof(cls) if fname == "sizeof" else getattr(cls, fname).offset
        assert got == int(val), (cname, fname, got, val)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in mirrors.values())
    assert len(_lib.RoiConfig().scales) == _lib.ROI_MAX_LEVELS


def test_roi_host_validation_without_a_gpu():
    """tdn_roi_align_* validate on the host before any launch; limits are reported through tdn_last_error."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    lv = (_lib.RoiLevel * 2)()
    for v, (h, w) in zip(lv, [(50, 84), (25, 42)]):
        v.data, v.H, v.W, v.dtype = 256, h, w, _lib.TDN_BF16       # never dereferenced on the host
        v.strides[:] = [h * w * 64, 1, w * 64, 64]
    cfg = _lib.RoiConfig(out_size=7, sampling_ratio=2, finest_scale=56.0)
    cfg.scales[0], cfg.scales[1] = 0.25, 0.125
    assert lib.tdn_roi_align_fwd(lv, 2, 2, 64, None, 0, ctypes.byref(cfg), None, None) == 0   # R = 0: no launch
    cfg.out_size = 17
    assert lib.tdn_roi_align_fwd(lv, 2, 2, 64, None, 0, ctypes.byref(cfg), None, None) < 0
    assert b"out_size" in lib.tdn_last_error()
    cfg.out_size = 7
    assert lib.tdn_roi_align_fwd(lv, 2, 2, 60, None, 0, ctypes.byref(cfg), None, None) < 0      # C % 8
    assert lib.tdn_roi_align_fwd(lv, 9, 2, 64, None, 0, ctypes.byref(cfg), None, None) < 0
    lv[1].dtype = _lib.TDN_F16
    assert lib.tdn_roi_align_fwd(lv, 2, 2, 64, None, 0, ctypes.byref(cfg), None, None) < 0
    assert b"dtype" in lib.tdn_last_error()
    lv[1].dtype = _lib.TDN_BF16
    lv[1].strides[1] = 42 * 25                                     # NCHW memory
    assert lib.tdn_roi_align_fwd(lv, 2, 2, 64, None, 0, ctypes.byref(cfg), None, None) < 0
    assert b"channel stride" in lib.tdn_last_error()
    lv[1].strides[1] = 1
    cfg.scales[1] = 0.0
    assert lib.tdn_roi_align_fwd(lv, 2, 2, 64, None, 0, ctypes.byref(cfg), None, None) < 0
    assert lib.tdn_roi_align_bwd_workspace(1000) >= 1000 * 48 and lib.tdn_roi_align_bwd_workspace(-1) < 0
    assert lib.tdn_roi_map_levels(None, 0, 9, 56.0, None, None) < 0


def test_bwd_workspace_size_is_the_design_table():
    """DESIGN.md §5d worked by hand: a 32-byte record and a 16-byte geometry vector per row, each region rounded up
    to 256 bytes."""
    from torch_detection_amd import _lib
    lib = _lib.load()
    assert lib.tdn_roi_align_bwd_workspace(1001) == 32256 + 16128      # 32032 -> 126 * 256, 16016 -> 63 * 256
    assert lib.tdn_roi_align_bwd_workspace(0) == 2 * 256               # R = 0 counts as one row
    assert lib.tdn_roi_align_bwd_workspace(-1) == -1 and lib.tdn_roi_align_bwd_workspace(1 << 31) == -1


# ---- host refusals (no GPU: shapes, dtypes, limits and scalars come first, the device last) --------------------------
def _refusals():
    import torch_detection_amd as T
    fs = [torch.zeros(2, 16, 8, 12, dtype=torch.bfloat16), torch.zeros(2, 16, 4, 6, dtype=torch.bfloat16)]
    rois = torch.zeros(10, 5)
    props, counts = torch.zeros(2, 10, 5), torch.zeros(2, dtype=torch.int32)
    return [
        (lambda: T.roi_align([f.float() for f in fs], rois, 7, (4, 8)), r"feats\[0\] must be a bfloat16 / float16"),
        (lambda: T.roi_align([fs[0], fs[1].half()], rois, 7, (4, 8)), r"feats\[1\] must be a bfloat16 .* got float16"),
        (lambda: T.roi_align([fs[0], fs[1][:1]], rois, 7, (4, 8)), r"feats\[1\] must be a bfloat16 \(2, 16, H, W\)"),
        (lambda: T.roi_align([fs[0], fs[1][:, :8]], rois, 7, (4, 8)), r"feats\[1\] must be a bfloat16 \(2, 16, H, W\)"),
        (lambda: T.roi_align([f[:, :12] for f in fs], rois, 7, (4, 8)), "C a positive multiple of 8"),
        (lambda: T.roi_align(fs, rois, 7, (4, 8, 16)), "2 feature levels but 3 featmap strides"),
        (lambda: T.roi_align(fs, rois, 17, (4, 8)), "out_size must be in 1..16"),
        (lambda: T.roi_align(fs, rois, 7, (4, 8), -1), "sampling_ratio must be in 0..512"),
        (lambda: T.roi_align(fs, rois, 7, (4, 8), 2, 0), "finest_scale must be finite and > 0"),
        (lambda: T.roi_align(fs, rois[:, 1:].contiguous(), 7, (4, 8)), r"rois must be a contiguous float32 \(R, 5\)"),
        (lambda: T.roi_align(fs, rois.double(), 7, (4, 8)), r"rois must be a contiguous float32 \(R, 5\)"),
        (lambda: T.roi_align(fs, rois.t().contiguous().t(), 7, (4, 8)), r"rois must be a contiguous float32 \(R, 5\)"),
        (lambda: T.roi_align(fs, rois, 7, (4, 8)), r"feats\[0\] must be a CUDA tensor"),
        (lambda: T.map_roi_levels(rois, 9), "num_levels must be in 1..8"),
        (lambda: T.map_roi_levels(rois[:, 1:].contiguous(), 4), r"rois must be a contiguous float32 \(R, 5\)"),
        (lambda: T.map_roi_levels(rois, 4, float("inf")), "finest_scale must be finite and > 0"),
        (lambda: T.map_roi_levels(rois, 4), "rois must be a CUDA tensor"),
        (lambda: T.SingleRoIExtractor(dict(type='RoIPool', out_size=7)), "roi_layer type 'RoIAlign' only"),
        (lambda: T.SingleRoIExtractor(out_channels=32)(fs + fs, rois), "out_channels is 32"),
        (lambda: T.rois_from_proposals(props[..., :4].contiguous(), counts),
         r"proposals must be a contiguous float32 \(B, M, 5\)"),
        (lambda: T.rois_from_proposals(props, torch.zeros(3, dtype=torch.int32)),
         r"counts must be a contiguous int32 \(2,\)"),
        (lambda: T.rois_from_proposals(props, counts), "proposals must be a CUDA tensor"),
    ]


def test_host_refusal_table_is_run_in_full():
    assert len(_refusals()) == 22


@pytest.mark.parametrize("case", range(22))
def test_host_refusals_need_no_gpu(case):
    fn, msg = _refusals()[case]
    with pytest.raises(ValueError, match=msg):
        fn()
