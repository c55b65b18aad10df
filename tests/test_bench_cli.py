"""bench.py's plain N = 1 run: `--steps` timed steps, the result line's contract fields, and
`--dump-outputs` (what the last timed step returned, from seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_float32_and_seeded_sample(tmp_path):
    """dump_outputs writes float32 <name>.npy; an array over its share of the byte limit is cut to
    a sample that is the same on every call."""
    import bench
    small = torch.arange(12, dtype=torch.float16).reshape(3, 4)
    big = torch.arange(1000, dtype=torch.float16)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big}, limit=2 * 4 * 100)
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(s, small.float().numpy())
    assert b.shape == (100,) and len(set(b.tolist())) == 100 and np.all(np.diff(b) > 0)
    assert s.nbytes + b.nbytes <= 2 * 4 * 100
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_step_output(tmp_path):
    """`bench.py --gpus 1 --steps 203 --warmup 2 --dump-outputs DIR` (one whole 200-step graph and
    one of the 3 steps left): the line carries the contract fields and none of --full's
    measurements, and DIR/C.npy is, bit for bit, what the drop-in call returns for inputs made
    again here from the benchmark's seeds."""
    import bench
    from kernels.mmq_q8_0 import mmq_q8_0
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "203",
                        "--warmup", "2", "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True,
                       timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 203 and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "TFLOP/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["metric"].startswith("effective fp16 TFLOPS")
    fmt, M, K, N = bench.CONFIGS[bench.DEFAULT]
    assert d["config"]["workload"] == bench.DEFAULT and d["config"]["weight_bytes_rotated"] >= 1 << 30
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(2.0 * M * N * K / (d["ms_per_step"] * 1e-3) / 1e12, rel=1e-3)
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert not {"eager_us", "per_type", "cpu_baseline_variants"} & set(d)
    assert sorted(os.listdir(tmp_path)) == ["C.npy"]
    got = np.load(tmp_path / "C.npy")
    assert got.dtype == np.float32 and got.shape == (N, M)
    dev = torch.device("cuda", 0)
    A = bench.device_random_blocks(fmt, M, K, dev, 0)
    g = torch.Generator(device=dev).manual_seed(1)
    B = torch.randn(N, K, device=dev, generator=g).to(torch.float16)
    want = mmq_q8_0(A, B, M, N, K).float().cpu().numpy()
    assert np.abs(want).max() > 0
    assert np.array_equal(got, want)
