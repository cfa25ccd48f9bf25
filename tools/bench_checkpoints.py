"""Checkpoint statistics beside the final-value step and beside keepdata + column passes, in ONE process.

Per mode (Gaussian, table) at n_paths x n_periods (default 1e8 x 360), warm-up 1, median of --reps (>= 5) steps;
per step the wall time (enqueue to drained stream) and the HIP-event time between the step's first and last
launch.  Outputs are allocated once, outside the timed region.
  A  simulate(final + statistics, 100 buckets)          -- the final-value step, the yardstick
  B  simulate_checkpoints, yearly x 100 buckets         -- with and without the final values
  C  simulate_checkpoints, one checkpoint at n_periods  -- the fixed cost of the kernel over A
  D  keepdata of --keep-rows rows + one column copy and values_stats pass per yearly column -- today's way, at
     the size that fits; compared PER PATH with B
One JSON line per measurement and one per mode with the ratios B/A, C/A, D/B (event times).  Usage:
  python tools/bench_checkpoints.py [--paths N] [--periods P] [--keep-rows R] [--reps K] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import stock_market_monte_carlo_amd as S  # noqa: E402
from stock_market_monte_carlo_amd import _lib  # noqa: E402


def measure(eng, fn, reps):
    """fn() enqueues one step on torch's current stream.  -> (median wall ms, median event ms, all event ms)."""
    stream = torch.cuda.current_stream(eng.tdevice)
    wall, dev = [], []
    for it in range(reps + 1):  # the first one is the warm-up
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng.sync()
        w0 = time.perf_counter()
        t0.record(stream)
        fn()
        t1.record(stream)
        eng.sync()
        w1 = time.perf_counter()
        if it:
            wall.append((w1 - w0) * 1e3)
            dev.append(t0.elapsed_time(t1))
    return statistics.median(wall), statistics.median(dev), dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100_000_000)
    ap.add_argument("--periods", type=int, default=360)
    ap.add_argument("--keep-rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 5)
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    eng.set_table(S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv")))
    yearly = np.arange(12, p + 1, 12, dtype=np.uint32)[: _lib.MAX_CHECKPOINTS]
    last = np.array([p], dtype=np.uint32)
    rec = int(L.smmc_stats_bytes(bins))
    final = torch.empty(n, dtype=torch.float32, device=dev)
    records = torch.empty(max(yearly.size, 1) * rec, dtype=torch.uint8, device=dev)
    traj = torch.empty((a.keep_rows, p + 1), dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for mode_name, mode in (("gaussian", S.MODE_GAUSSIAN), ("table", S.MODE_TABLE)):
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
        ksim = S.Engine.make_sim(a.keep_rows, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(records)))

        def checkpoints(periods, fin):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_checkpoints(h, C.byref(sim), periods.ctypes.data_as(C.c_void_p), periods.size,
                                                              ptr(fin), ptr(records)))
            return step

        def step_d():
            eng._enter()
            _lib.check(L.smmc_engine_simulate_keepdata(h, C.byref(ksim), ptr(traj), None))
            for k, q in enumerate(yearly):
                col = traj[:, int(q)].contiguous()
                _lib.check(L.smmc_engine_values_stats(h, ptr(col), col.numel(), 1000.0, bins, 0.0, 20000.0,
                                                      C.c_void_p(records.data_ptr() + k * rec)))

        res = {}
        for name, fn, paths in (("A_simulate_final_stats", step_a, n),
                                ("B_checkpoints_yearly_final", checkpoints(yearly, final), n),
                                ("B_checkpoints_yearly", checkpoints(yearly, None), n),
                                ("C_checkpoint_last_final", checkpoints(last, final), n),
                                ("D_keepdata_column_passes", step_d, a.keep_rows)):
            wall, ev, all_ev = measure(eng, fn, reps)
            res[name] = ev / paths
            emit({"mode": mode_name, "step": name, "n_paths": paths, "n_periods": p, "n_bins": bins,
                  "checkpoints": int(yearly.size) if name[0] in "BD" else (1 if name[0] == "C" else 0), "reps": reps,
                  "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev],
                  "ns_per_path": round(ev / paths * 1e6, 4)})
        emit({"mode": mode_name, "ratios": {
            "B/A": round(res["B_checkpoints_yearly_final"] / res["A_simulate_final_stats"], 4),
            "B_without_final/A": round(res["B_checkpoints_yearly"] / res["A_simulate_final_stats"], 4),
            "C/A": round(res["C_checkpoint_last_final"] / res["A_simulate_final_stats"], 4),
            "D/B per path": round(res["D_keepdata_column_passes"] / res["B_checkpoints_yearly_final"], 3)}})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
