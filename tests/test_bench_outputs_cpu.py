"""bench.py's --dump-outputs on the CPU: the sample of a long per-path output is fixed by its length alone, the files
are float32 / float64 and stay under 64 MB; and --steps must name at least one timed step."""
import os
import subprocess
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_sample_positions_are_fixed_sorted_and_bounded():
    import bench
    assert bench.sample_positions(bench.DUMP_SAMPLE) is None and bench.sample_positions(1000) is None
    n = 10 ** 8
    a, b = bench.sample_positions(n), bench.sample_positions(n)
    assert np.array_equal(a, b)
    assert 0.9 * bench.DUMP_SAMPLE < a.size <= bench.DUMP_SAMPLE
    assert a[0] >= 0 and a[-1] < n and np.all(np.diff(a) > 0)


def test_dump_outputs_writes_float_arrays_under_64_mb(tmp_path):
    import bench
    n = 3 * bench.DUMP_SAMPLE
    final = np.arange(n, dtype=np.float32)
    nc = bench.DUMP_SAMPLE + 7  # longer than the sample too
    cm, cv = np.full(nc, 2.0, dtype=np.float32), np.full(nc, 3.0, dtype=np.float32)
    hist = np.array([5, 0, 7], dtype=np.uint64)
    stats = types.SimpleNamespace(count=13, below=4, underflow=1, overflow=0, sum=130.5, sumsq=1500.25, min=1.0, max=20.0,
                                  hist=hist)
    names = bench.dump_outputs(str(tmp_path), final=final, chunk_mean=cm, chunk_var=cv, stats=stats)
    assert names == ["chunk_mean", "chunk_var", "final_values", "histogram", "stats"]
    assert sum(os.path.getsize(tmp_path / f"{k}.npy") for k in names) <= 64 << 20
    got = {k: np.load(tmp_path / f"{k}.npy") for k in names}
    assert np.array_equal(got["final_values"], final[bench.sample_positions(n)])
    assert got["final_values"].dtype == got["chunk_mean"].dtype == np.float32
    assert got["chunk_mean"].size == bench.sample_positions(nc).size and np.all(got["chunk_var"] == 3.0)
    assert got["histogram"].dtype == np.float64 and got["histogram"].tolist() == [5.0, 0.0, 7.0]
    assert got["stats"].tolist() == [13, 4, 1, 0, 130.5, 1500.25, 1.0, 20.0]
    # only what the workload produced: a statistics-only run writes the record alone
    assert bench.dump_outputs(str(tmp_path / "stats_only"), stats=stats) == ["histogram", "stats"]


def test_steps_must_be_at_least_one():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr
