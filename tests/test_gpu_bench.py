"""bench.py's plain run on the GPU: `--steps` timed steps and nothing beside them in the line, and `--dump-outputs`
writing the same beams for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _plain(steps, out_dir):
    # config 4 with one buffer set: the smallest input of the three workloads (1 GiB), int8 beams of 128 MiB (sampled)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3",
           "--settle-ms", "0", "--workload", "cfg4", "--nbuf", "1", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "beams.npy"))


def test_plain_bench_line_and_repeatable_dump(tmp_path):
    line, a = _plain(3, tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "Gsamples/s" and line["dtype"] == "int8"
    # the step's time and the rate are one measurement: samples per step / ms_per_step
    assert line["value"] == pytest.approx(256 * 2 * 4096 * 256 / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-2)
    for key in ("secondary", "ceiling", "int8_contract_check"):  # --full only
        assert key not in line
    assert line["cpu_baseline"] is None and line["roofline"]["traffic"] is None and "rocprof" not in line["roofline"]
    assert a.dtype == np.float32 and 0 < a.nbytes <= 64 << 20
    assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 128 and len(np.unique(a)) > 16  # int8 beams, not blank
    more, b = _plain(12, tmp_path / "b")  # the same input and delay model, whatever the step count
    np.testing.assert_array_equal(a, b)
    # --steps sets the number of timed launches: four times the steps take the same time per step.  Were the option
    # ignored, the two ms_per_step (timed wall time / --steps) would differ by that factor of 4; the few-step run's
    # share of the queue's launch and sync latency and of the clock ramp stays far inside a factor of 2.
    assert more["steps"] == 12
    assert 0.5 < more["ms_per_step"] / line["ms_per_step"] < 2.0, (line["ms_per_step"], more["ms_per_step"])
