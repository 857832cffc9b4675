"""bench.py's measurement contract: the plain run's result line and --dump-outputs (the last timed step's FPN outputs
and parameter gradients as float32 .npy files, large ones as a fixed sample).  The sampling is checked on CPU
tensors; the end-to-end run needs the MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_and_sampled(tmp_path):
    big = torch.randn(2, 8, 30, 40, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    small = torch.randn(2, 8, 3, 5, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    arrays = [("P2", big, 1000), ("P6", small, 1000)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = np.load(str(tmp_path / "a" / "P2.npy"))
    idx = np.sort(np.random.default_rng(0).choice(big.numel(), 1000, replace=False))
    assert got.dtype == np.float32 and got.shape == (1000,)
    assert np.array_equal(got, big.float().reshape(-1).numpy()[idx])           # row-major (NCHW) positions
    assert np.array_equal(got, np.load(str(tmp_path / "b" / "P2.npy")))       # same positions every run
    whole = np.load(str(tmp_path / "a" / "P6.npy"))
    assert whole.dtype == np.float32 and np.array_equal(whole, small.float().numpy())


def test_dump_outputs_refuses_over_limit(tmp_path):
    n = bench.DUMP_MAX_BYTES // 4 + 1
    with pytest.raises(SystemExit, match="limit"):
        bench.dump_outputs(str(tmp_path), [("x", torch.zeros(n), n)])
    assert not os.listdir(str(tmp_path))


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, stdout=subprocess.PIPE, timeout=600)
    assert r.returncode == 0
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert line["steps"] == 3 and line["unit"] == "images/sec" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
    for k in ("cpu_baseline", "secondary", "ms_per_step_with_repack"):   # side measurements are --full only
        assert k not in line
    assert line["roofline"] is None
    files = sorted(os.listdir(str(out)))
    assert [f for f in files if not f.startswith("grad.")] == ["P%d.npy" % l for l in range(2, 7)]
    grads = [f for f in files if f.startswith("grad.")]
    assert "grad.backbone.conv1.weight.npy" in grads and "grad.neck.fpn_convs.0.conv.bias.npy" in grads
    assert sum(os.path.getsize(str(out / f)) for f in files) <= bench.DUMP_MAX_BYTES
    p6 = np.load(str(out / "P6.npy"))
    assert p6.dtype == np.float32 and p6.shape == (2, 256, 13, 21)
    assert np.load(str(out / "P2.npy")).shape == (bench.DUMP_CAP["level"],)
    for f in ("P2.npy", "P6.npy", "grad.backbone.conv1.weight.npy"):
        a = np.load(str(out / f))
        assert np.isfinite(a).all() and np.abs(a).max() > 0
