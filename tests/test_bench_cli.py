"""bench.py's command line: a plain run does the timed steps alone, `--full` adds the checks and secondary measurements,
`--dump-outputs DIR` writes the last timed step's output so that two builds can be compared on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
EXTRAS = ("a8", "int8", "cpu_baseline")


def run_bench(*args):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_keeps_a_small_output_whole_and_samples_a_large_one(tmp_path):
    import bench
    small = torch.randn(100, 2048).bfloat16()
    bench.dump_outputs(small, str(tmp_path / "small"))
    got = np.load(tmp_path / "small" / "out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.float().numpy())
    # 5000 rows of 2048 floats are above the 32 MiB cap: 4096 of the rows, in their order, the same ones every time
    big = torch.arange(5000, dtype=torch.float32).unsqueeze(1).expand(5000, 2048)     # row r holds r
    bench.dump_outputs(big, str(tmp_path / "big1"))
    bench.dump_outputs(big, str(tmp_path / "big2"))
    b1, b2 = np.load(tmp_path / "big1" / "out.npy"), np.load(tmp_path / "big2" / "out.npy")
    assert b1.dtype == np.float32 and b1.shape == (4096, 2048) and b1.nbytes <= bench.DUMP_MAX_BYTES
    assert np.array_equal(b1, b2)
    rows = b1[:, 0]
    assert (np.diff(rows) > 0).all() and (b1 == rows[:, None]).all()
    assert set(rows.tolist()) <= set(big[:, 0].float().tolist())


@pytest.mark.gpu
def test_plain_run_times_the_steps_alone_and_dumps_the_same_output_every_time(tmp_path):
    """Two plain runs with different --steps: the second goes beyond the 96 input clones, whose reuse (inplace=True) must
    not reach the step that is written.  Same seeded inputs, same kernels: the two files are equal bit for bit."""
    a = run_bench("--steps", 3, "--warmup", 1, "--tokens", 512, "--dump-outputs", tmp_path / "a")
    b = run_bench("--steps", 110, "--warmup", 1, "--tokens", 512, "--dump-outputs", tmp_path / "b")
    for line, steps in ((a, 3), (b, 110)):
        assert line["metric"] == "fused_experts_fp8_w8a16_tflops" and line["unit"] == "TFLOP/s"
        assert line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert line["steps"] == steps and line["roofline"]["launches"] == steps
        assert line["ms_per_step"] > 0 and line["value"] > 0
        assert line["verified"] is None and not any(k in line for k in EXTRAS)
    xa, xb = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert os.listdir(tmp_path / "a") == ["out.npy"]
    assert xa.dtype == np.float32 and xa.shape == (512, 2048)
    assert np.isfinite(xa).all() and np.abs(xa).max() > 0
    assert np.array_equal(xa, xb)


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_secondary_measurements():
    line = run_bench("--full", "--steps", 3, "--warmup", 1, "--tokens", 512, "--cpu-tokens", 64)
    assert line["verified"] is True and line["verification"]["rows"] >= 64
    assert all(k in line for k in EXTRAS)
    assert line["int8"]["verification"]["ok"] is True
    assert line["cpu_baseline"]["value"] > 0
