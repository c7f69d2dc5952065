"""GPU: a plain `bench.py` run (no --full) prints the headline line alone; what the headline does not need waits for --full."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# objects only `bench.py --full` computes (each takes runs of its own after the timed steps)
FULL_ONLY = ("roofline", "launches_per_step", "kernels", "clock_power", "cpu_baseline", "parity", "also")


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_alone(tmp_path):
    steps, warmup = 2, 1
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "patches/sec encode+decode" and line["unit"] == "patches/s" and line["higher_is_better"] is True
    assert line["dtype"].startswith("f32") and line["steps"] == steps and line["warmup"] == warmup
    # value and ms_per_step describe the same timed region: 32 clips x 5120 patches per step
    assert line["value"] == pytest.approx(32 * 5120 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not set(FULL_ONLY) & set(line), sorted(set(FULL_ONLY) & set(line))
    assert line["native_gather_probe"] is None
    assert sorted(os.listdir(tmp_path)) == ["ids.npy", "pixels_sample.npy"]
    print(f"plain bench run: {wall:.1f} s wall, {wall - (steps + warmup) * line['ms_per_step'] * 1e-3:.1f} s outside its steps")
