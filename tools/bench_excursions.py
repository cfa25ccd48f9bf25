"""Excursion statistics beside the final-value step, in ONE process.

n_paths x n_periods (default 1e8 x 360: configs[1] / configs[2] of bench.py), Gaussian and table mode, warm-up 1,
median of --reps (>= 5) steps; per step the wall time (enqueue to drained stream) and the HIP-event time between the
step's first and last launch.  Outputs are allocated once, outside the timed region.
  A  simulate(final + statistics, 100 buckets)              -- the final-value step (paths_kernel), the yardstick
  B  simulate_excursions, all twelve outputs                -- eight per-path arrays, two records, two count arrays
  C  simulate_excursions, records and count arrays only     -- no per-path output
  K  simulate_keepdata + one values_stats pass over a column, at the largest n_paths whose trajectories fit in
     --keepdata-gib of device memory: what the host-pass route costs, for scale (per path, not per step)
One JSON line per measurement and one per mode with the ratios B/A, C/A (event times) beside the instruction-count
ratio DESIGN.md expects (38.0 / 17.5 VALU per Gaussian period, 31.0 / 10.5 per dense-table period).  A is the same
code as in the commit before this feature: its paths_kernel instructions did not move.  Usage:
  python tools/bench_excursions.py [--paths N] [--periods P] [--modes gaussian,table] [--reps K] [--out FILE]
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
import torch  # noqa: E402

import stock_market_monte_carlo_amd as S  # noqa: E402
from stock_market_monte_carlo_amd import _lib  # noqa: E402

EXPECTED_VALU_RATIO = {"gaussian": 38.0 / 17.5, "table": 31.0 / 10.5}  # profiles/excursions/isa.txt: per period, as compiled


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
    ap.add_argument("--modes", default="gaussian,table")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--keepdata-gib", type=float, default=8.0, help="0 skips step K")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 5)
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    eng.set_table(S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv")))
    f32 = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)]
    u32 = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
    rec = [torch.empty(int(L.smmc_stats_bytes(bins)), dtype=torch.uint8, device=dev) for _ in range(2)]
    at = [torch.empty(p + 1, dtype=torch.int64, device=dev) for _ in range(2)]
    x = S.Engine.make_excursions(800.0, 2000.0, 0.2)

    def outputs(per_path):
        o = _lib.ExcursionOutputs()
        o.struct_size = C.sizeof(_lib.ExcursionOutputs)
        if per_path:
            for name, t in zip(_lib.EXCURSION_OUTPUTS[:8], f32 + u32):
                setattr(o, name, t.data_ptr())
        o.stats, o.drawdown_stats = rec[0].data_ptr(), rec[1].data_ptr()
        o.first_below_at, o.first_reach_at = at[0].data_ptr(), at[1].data_ptr()
        return o

    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for mode_name in a.modes.split(","):
        mode = S.MODE_GAUSSIAN if mode_name == "gaussian" else S.MODE_TABLE
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), C.c_void_p(f32[0].data_ptr()), None, None,
                                              C.c_void_p(rec[0].data_ptr())))

        def excursions(o):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_excursions(h, C.byref(sim), C.byref(x), C.byref(o)))
            return step

        res = {}
        for name, fn in (("A_simulate_final_stats", step_a), ("B_excursions_all_outputs", excursions(outputs(True))),
                         ("C_excursions_records_and_counts", excursions(outputs(False)))):
            wall, ev, all_ev = measure(eng, fn, reps)
            res[name] = ev
            emit({"mode": mode_name, "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps,
                  "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "event_ms_all": [round(v, 4) for v in all_ev],
                  "ns_per_path": round(ev / n * 1e6, 4),
                  "divide": ("fast", "exact", "checked")[L.smmc_engine_divide_kind(h, C.byref(sim), 0 if name[0] == "A" else 1)]})
        base = res["A_simulate_final_stats"]
        emit({"mode": mode_name, "build_digest": _lib.build_digest(), "ratios": {
            "B/A": round(res["B_excursions_all_outputs"] / base, 4),
            "C/A": round(res["C_excursions_records_and_counts"] / base, 4),
            "expected VALU per period, excursions / plain": round(EXPECTED_VALU_RATIO[mode_name], 4)}})
        if a.keepdata_gib > 0:  # keepdata + one pass over the last column, at the largest size that fits
            nk = min(n, int(a.keepdata_gib * 2 ** 30) // (4 * (p + 1)))
            ksim = S.Engine.make_sim(nk, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
            traj = torch.empty(nk * (p + 1), dtype=torch.float32, device=dev)
            col = torch.empty(nk, dtype=torch.float32, device=dev)

            def step_k():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_keepdata(h, C.byref(ksim), C.c_void_p(traj.data_ptr()), C.c_void_p(col.data_ptr())))
                _lib.check(L.smmc_engine_values_stats(h, C.c_void_p(col.data_ptr()), C.c_uint64(nk), C.c_float(1000.0),
                                                      C.c_uint32(bins), C.c_float(0.0), C.c_float(20000.0),
                                                      C.c_void_p(rec[0].data_ptr())))

            wall, ev, all_ev = measure(eng, step_k, reps)
            emit({"mode": mode_name, "step": "K_keepdata_plus_one_pass", "n_paths": nk, "n_periods": p, "reps": reps,
                  "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "ns_per_path": round(ev / max(nk, 1) * 1e6, 4),
                  "ns_per_path_B": round(res["B_excursions_all_outputs"] / n * 1e6, 4)})
            del traj, col
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
