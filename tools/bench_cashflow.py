"""Cash-flow schedules beside the final-value step, in ONE process.

Gaussian mode at n_paths x n_periods (default 1e8 x 360: configs[1] of bench.py), warm-up 1, median of --reps
(>= 5) steps; per step the wall time (enqueue to drained stream) and the HIP-event time between the step's first and
last launch.  Outputs are allocated once, outside the timed region.
  A  simulate(final + statistics, 100 buckets)                   -- the final-value step (paths_kernel), the yardstick
  B  simulate_cashflow, constant amount, all five outputs        -- 6.0 per period, floor 0.01
  C  the same with per-period arrays                             -- the amount grows 0.2 % per period
  D  simulate_cashflow, statistics and depletion counts only     -- no per-path output
One JSON line per measurement and one with the ratios B/A, C/A, D/A (event times) beside the instruction-count
ratio DESIGN.md expects (27.5 / 17.5 VALU per period).  A is the same code as in the commit before this feature: run
this tool's step A there (or bench.py) on the same box for the parent's figure.  Usage:
  python tools/bench_cashflow.py [--paths N] [--periods P] [--mode gaussian|table] [--reps K] [--out FILE]
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

EXPECTED_VALU_RATIO = {"gaussian": 27.5 / 17.5, "table": 20.5 / 10.5}  # DESIGN.md, "Cash flows": per period, counted in the ISA


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
    ap.add_argument("--mode", choices=("gaussian", "table"), default="gaussian")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 5)
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    eng.set_table(S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv")))
    mode = S.MODE_GAUSSIAN if a.mode == "gaussian" else S.MODE_TABLE
    sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
    final = torch.empty(n, dtype=torch.float32, device=dev)
    paid = torch.empty(n, dtype=torch.float32, device=dev)
    ruin = torch.empty(n, dtype=torch.int32, device=dev)
    record = torch.empty(int(L.smmc_stats_bytes(bins)), dtype=torch.uint8, device=dev)
    depleted = torch.empty(p + 1, dtype=torch.int64, device=dev)
    amounts = (6.0 * 1.002 ** np.arange(p)).astype(np.float32)
    cf_const, keep_const = S.Engine.make_cashflow(p, amount=6.0, floor=0.01)
    cf_arrays, keep_arrays = S.Engine.make_cashflow(p, amounts=amounts, fractions=np.zeros(p, np.float32), floor=0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def step_a():
        eng._enter()
        _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

    def cashflow(cf, per_path):
        def step():
            eng._enter()
            _lib.check(L.smmc_engine_simulate_cashflow(h, C.byref(sim), C.byref(cf), ptr(final if per_path else None),
                                                       ptr(paid if per_path else None), ptr(ruin if per_path else None),
                                                       ptr(record), ptr(depleted)))
        return step

    res = {}
    for name, fn in (("A_simulate_final_stats", step_a), ("B_cashflow_constant_all_outputs", cashflow(cf_const, True)),
                     ("C_cashflow_arrays_all_outputs", cashflow(cf_arrays, True)),
                     ("D_cashflow_constant_stats_and_counts", cashflow(cf_const, False))):
        wall, ev, all_ev = measure(eng, fn, reps)
        res[name] = ev
        line = {"mode": a.mode, "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps,
                "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev],
                "ns_per_path": round(ev / n * 1e6, 4)}
        if name[0] != "A":
            line["depleted_share"] = round(1.0 - int(depleted.cpu().numpy().view(np.uint64)[0]) / max(n, 1), 6)
            line["divide"] = "fast" if L.smmc_engine_cashflow_divide_kind(
                h, C.byref(sim), C.byref(cf_arrays if name[0] == "C" else cf_const)) == _lib.DIV_FAST else "exact"
        emit(line)
    base = res["A_simulate_final_stats"]
    emit({"mode": a.mode, "build_digest": _lib.build_digest(), "ratios": {
        "B/A": round(res["B_cashflow_constant_all_outputs"] / base, 4),
        "C/A": round(res["C_cashflow_arrays_all_outputs"] / base, 4),
        "D/A": round(res["D_cashflow_constant_stats_and_counts"] / base, 4),
        "expected VALU per period, cash flow / plain": round(EXPECTED_VALU_RATIO[a.mode], 4)}})
    del keep_const, keep_arrays
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
