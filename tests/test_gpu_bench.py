"""bench.py at N=1 on the GPU: a plain run prints the headline line and nothing that needs a run of its own; --full adds the
per-kernel timing pass and its roofline figures, the driver leg and cpu_baseline.  Small grid, few steps: the form of the line, not
its figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels_ms_per_launch", "kernels_ms_per_step", "kernels_GBs", "driver", "cpu_baseline")


def _bench(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", "256", "--steps", "3", "--warmup", "1"] + list(extra)
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{")                         # stdout is the line and nothing else
    d = json.loads(lines[0])
    assert all(k in d for k in HEADLINE), d
    assert d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3                 # the same K steps behind both figures
    return d


def test_plain_run_prints_the_headline_only(tmp_path):
    d = _bench(tmp_path, "--dump-outputs", "dump")
    assert not [k for k in FULL_ONLY if k in d], d
    assert d["dumped_outputs"]["after_steps"] == 4
    v = np.load(str(tmp_path / "dump" / "vort.npy"))
    assert v.shape == (256, 256) and np.isfinite(v).all()


def test_full_run_adds_every_leg(tmp_path):
    d = _bench(tmp_path, "--full", "--cpu-steps", "1", "--driver-steps", "200", "--dump-outputs", "dump")
    assert d["roofline"]["kernel"] in d["kernels_ms_per_launch"] and d["roofline"]["achieved"] > 0
    assert all(v > 0 for v in d["kernels_ms_per_step"].values())
    assert d["driver"]["steps"] == 200 and d["driver"]["records"] == 2 and d["driver"]["driver_steps_per_s"] > 0, d["driver"]
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 1
    # the extra legs run after the dump: the same W + K steps from the same initial field as a plain run
    plain = tmp_path / "plain"
    plain.mkdir()
    _bench(plain, "--dump-outputs", "dump")
    a, b = np.load(str(tmp_path / "dump" / "vort.npy")), np.load(str(plain / "dump" / "vort.npy"))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
