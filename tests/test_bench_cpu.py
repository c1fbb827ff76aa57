"""bench.py's command line and its --dump-outputs writer, on the host (no GPU)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_steps_and_dump_arguments():
    a = bench.parse_args(["--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 2, "out")
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "out"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True
    a = bench.parse_args(["--gpus", "2", "--full", "--also-grid", "256"])
    assert (a.gpus, a.full, a.also_grid) == (2, True, "256")


@pytest.mark.parametrize("n", [256, 4096, 8192])
def test_dump_outputs_is_bounded_and_repeatable(tmp_path, n):
    v = np.random.default_rng(n).standard_normal((n, n), dtype=np.float32)
    shapes = bench.dump_outputs(str(tmp_path / "a"), v)
    bench.dump_outputs(str(tmp_path / "b"), v)
    total = 0
    for name in ("vort", "vort_rows"):
        pa, pb = tmp_path / "a" / (name + ".npy"), tmp_path / "b" / (name + ".npy")
        assert pa.read_bytes() == pb.read_bytes()                      # the same rows on every run
        total += pa.stat().st_size
    assert total <= 64 * 10**6
    got, rows = np.load(str(tmp_path / "a" / "vort.npy")), np.load(str(tmp_path / "a" / "vort_rows.npy"))
    assert got.dtype == np.float32 and rows.dtype == np.float64
    assert shapes == {"vort": list(got.shape), "vort_rows": list(rows.shape)}
    idx = rows.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(got, v[idx])
    if n == 256:
        assert got.shape == (n, n)                                      # small fields are written whole
