"""bench.py's command line without a GPU: the output dump (float32 / float64 .npy, a seeded sample past the size cap) and the
argument checks that run before any device work."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_dtypes(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), {"a": np.arange(6, dtype=np.float64).reshape(2, 3),
                                             "b": np.arange(4, dtype=np.int32), "c": np.float32(2.5)})
    a, b, c = (np.load(tmp_path / "d" / f"{n}.npy") for n in "abc")
    assert a.dtype == np.float64 and a.shape == (2, 3) and np.array_equal(a, np.arange(6).reshape(2, 3))
    assert b.dtype == np.float32 and np.array_equal(b, np.arange(4))
    assert c.dtype == np.float32 and c == 2.5
    assert sorted(os.listdir(tmp_path / "d")) == ["a.npy", "b.npy", "c.npy"]


def test_dump_outputs_caps_with_a_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = np.arange(10000, dtype=np.float64)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"small": np.ones(8, np.float32), "big": big})
    small = np.load(tmp_path / "x" / "small.npy")
    got, idx = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "x" / "big_sample_index.npy")
    assert small.size == 8 and 0 < got.size < big.size and idx.dtype == np.float64
    assert np.array_equal(got, big[idx.astype(np.int64)]) and np.all(np.diff(idx) > 0)
    assert small.nbytes + got.nbytes + idx.nbytes <= 4096
    # the same sample every run
    assert np.array_equal(got, np.load(tmp_path / "y" / "big.npy"))


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr and r.stdout.strip() == ""
