"""bench.py's command line and its --dump-outputs writer, without a GPU (the argument checks run before torch is imported)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_help_names_full_and_dump_outputs():
    r = _bench("--help")
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


@pytest.mark.parametrize("args", [("--steps", "0"), ("--steps", "-1"), ("--warmup", "-1")])
def test_step_counts_are_checked(args):
    r = _bench(*args)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def test_dump_outputs_writes_float64_arrays(tmp_path):
    import bench

    labels = np.arange(1000, dtype=np.int32) % 7 + 1
    bench.dump_outputs(str(tmp_path / "out"), {"pred_clusters": labels, "n_pred_clusters": 7, "reduced_dim": 474})
    assert sorted(os.listdir(tmp_path / "out")) == ["n_pred_clusters.npy", "pred_clusters.npy", "reduced_dim.npy"]
    got = np.load(tmp_path / "out" / "pred_clusters.npy")
    assert got.dtype == np.float64 and np.array_equal(got, labels)
    assert np.load(tmp_path / "out" / "n_pred_clusters.npy") == 7.0 and np.load(tmp_path / "out" / "reduced_dim.npy") == 474.0


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 100)
    a = np.arange(1000) * 3
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"x": a})
    x, idx = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "x_sample_index.npy")
    assert x.shape == (100,) and x.dtype == np.float64 and np.array_equal(x, a[idx.astype(np.int64)])
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(x, np.load(tmp_path / "b" / "x.npy")) and np.array_equal(idx, np.load(tmp_path / "b" / "x_sample_index.npy"))


def test_dump_budget_stays_under_64_mb():
    import bench

    assert bench.DUMP_MAX_VALUES * 8 * 2 <= 56 * 2 ** 20         # a sampled array and its positions, with room for the scalars
