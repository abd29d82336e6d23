"""bench.py's --dump-outputs writer, without a GPU: float32 files, whole while they fit the budget, a fixed seeded sample of the
pixels (with their indices) when they do not."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_outputs", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_outputs_within_budget_are_written_whole(tmp_path):
    b = _bench()
    film = np.random.default_rng(1).random((108, 192, 4)).astype(np.float32)
    b.write_outputs(str(tmp_path / "o"), {"film": film})
    assert sorted(os.listdir(tmp_path / "o")) == ["film.npy"]
    got = np.load(tmp_path / "o" / "film.npy")
    assert got.dtype == np.float32 and got.tobytes() == film.tobytes()


def test_outputs_over_budget_are_a_fixed_sample(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "OUTPUT_BUDGET_BYTES", 1 << 20)
    film = np.random.default_rng(2).random((512, 768, 4)).astype(np.float32)      # 6 MB against a 1 MB budget
    for d in ("a", "b"):
        b.write_outputs(str(tmp_path / d), {"film": film})
    sizes = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert sizes <= (1 << 20) + 1024                    # (+ the two .npy headers)
    got, idx = np.load(tmp_path / "a" / "film.npy"), np.load(tmp_path / "a" / "film_index.npy")
    assert got.dtype == np.float32 and idx.dtype == np.float64 and got.shape == (len(idx), 4) and len(idx) > 30000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 512 * 768
    assert got.tobytes() == film.reshape(-1, 4)[idx.astype(np.int64)].tobytes()
    for f in ("film.npy", "film_index.npy"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
