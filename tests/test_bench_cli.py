"""bench.py without a GPU: the output dump of --dump-outputs and the argument checks that run before any device work."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tallies(rows):
    g = np.random.default_rng(7)
    return g.integers(0, 10 ** 12, size=(rows, 13), dtype=np.uint64)


def test_dump_writes_the_whole_matrix_in_float64(tmp_path):
    t = _tallies(300)
    bench.dump_outputs(str(tmp_path / "d"), t)
    assert sorted(os.listdir(tmp_path / "d")) == ["tallies.npy"]
    got = np.load(tmp_path / "d" / "tallies.npy")
    assert got.dtype == np.float64 and np.array_equal(got, t.astype(np.float64))
    assert np.array_equal(got.astype(np.uint64), t)   # counts below 2^53 survive the conversion exactly


def test_dump_samples_a_large_matrix_with_a_fixed_seed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 * 1024)
    t = _tallies(5000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), t)
    rows_a, rows_b = (np.load(tmp_path / d / "tallies_rows.npy") for d in ("a", "b"))
    got = np.load(tmp_path / "a" / "tallies.npy")
    assert np.array_equal(rows_a, rows_b) and np.array_equal(got, np.load(tmp_path / "b" / "tallies.npy"))
    assert got.nbytes + rows_a.nbytes <= bench.DUMP_MAX_BYTES and 0 < len(rows_a) < len(t)
    idx = rows_a.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < len(t)
    assert np.array_equal(got, t[idx].astype(np.float64))


def test_steps_must_be_positive():
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, (bad, r.stderr[-500:])
        assert not [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("{")]
