"""Cash-flow sweeps beside the same scenarios as single calls and beside the final-value step, in ONE process.

n_paths x n_periods (default 1e8 x 360: configs[1] of bench.py), Gaussian and the bundled table, warm-up 1, median of
--reps (>= 5) steps; per step the wall time (enqueue to drained stream) and the HIP-event time between the step's first
and last launch.  Outputs are allocated once, outside the timed region.  Scenarios: amounts 0, 2, 3, 4, 5, 6, 8, 12 per
period on floor 0.01 (the first S of them reordered so that S = 1 is 6.0: 6, 4, 8, 2, 5, 3, 12, 0).
  A        simulate(final + statistics)                                -- the final-value step (paths_kernel)
  sweep S  smmc_engine_simulate_cashflow_sweep, S = 1, 2, 4, 8         -- statistics and depletion counts only ("counts"),
                                                                          and again with final, paid and ruin_period ("all")
  single S S calls of smmc_engine_simulate_cashflow, the same outputs  -- the baseline: unchanged code
A and the single calls are the same code as in the commit before this feature.  One JSON line per measurement; per
mode the clock the chip held under step A (smmc_engine_kernel_clock) and the ratios sweep S / single S beside the
instruction-count ratio DESIGN.md expects ((14.5 + 13 S) / 27.5 S Gaussian, (7.5 + 13 S) / 20.5 S table).  Usage:
  python tools/bench_sweep.py [--paths N] [--periods P] [--modes gaussian,table] [--reps K] [--out FILE]
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

AMOUNTS = (6.0, 4.0, 8.0, 2.0, 5.0, 3.0, 12.0, 0.0)
DRAW, STEP = {"gaussian": 14.5, "table": 7.5}, 13.0  # VALU per period: DESIGN.md, "Cash-flow sweeps"


def expected_ratio(mode, s):
    return (DRAW[mode] + STEP * s) / ((DRAW[mode] + STEP) * s)


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 5)
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    eng.set_table(S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv")))
    rec = int(L.smmc_stats_bytes(bins))
    smax = len(AMOUNTS)
    final = torch.empty((smax, n), dtype=torch.float32, device=dev)
    paid = torch.empty((smax, n), dtype=torch.float32, device=dev)
    ruin = torch.empty((smax, n), dtype=torch.int32, device=dev)
    record = torch.empty((smax, rec), dtype=torch.uint8, device=dev)
    depleted = torch.empty((smax, p + 1), dtype=torch.int64, device=dev)
    cfs, _, _, _ = S.Engine.make_sweep(AMOUNTS, 0.0, 0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for mode_name in a.modes.split(","):
        mode = S.MODE_GAUSSIAN if mode_name == "gaussian" else S.MODE_TABLE
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final[0]), None, None, ptr(record[0])))

        def sweep(s, per_path):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_cashflow_sweep(
                    h, C.byref(sim), cfs, s, ptr(final if per_path else None), ptr(paid if per_path else None),
                    ptr(ruin if per_path else None), ptr(record), ptr(depleted)))
            return step

        def singles(s, per_path):
            def step():
                eng._enter()
                for i in range(s):
                    _lib.check(L.smmc_engine_simulate_cashflow(
                        h, C.byref(sim), C.byref(cfs[i]), ptr(final[i] if per_path else None), ptr(paid[i] if per_path else None),
                        ptr(ruin[i] if per_path else None), ptr(record[i]), ptr(depleted[i])))
            return step

        def line(step, ev, wall, all_ev, **more):
            d = {"mode": mode_name, "step": step, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps, "wall_ms": round(wall, 4),
                 "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev]}
            d.update(more)
            emit(d)

        eng.timing(True)
        wall, base, all_ev = measure(eng, step_a, reps)
        clock = eng.kernel_clock_ghz()
        eng.timing(False)
        line("A_simulate_final_stats", base, wall, all_ev)
        ratios = {}
        for per_path in (False, True):
            outputs = "all" if per_path else "counts"
            for s in (1, 2, 4, 8):
                wall, ev_sweep, all_ev = measure(eng, sweep(s, per_path), reps)
                share = [round(1.0 - int(x) / max(n, 1), 6) for x in depleted.cpu().numpy().view(np.uint64)[:s, 0]]
                kind = "fast" if L.smmc_engine_cashflow_sweep_divide_kind(h, C.byref(sim), cfs, s) == _lib.DIV_FAST else "exact"
                line(f"sweep_{s}_{outputs}", ev_sweep, wall, all_ev, scenarios=s, outputs=outputs, depleted_share=share, divide=kind)
                wall, ev_single, all_ev = measure(eng, singles(s, per_path), reps)
                line(f"single_x{s}_{outputs}", ev_single, wall, all_ev, scenarios=s, outputs=outputs)
                ratios[f"S={s} {outputs}"] = {"sweep/singles": round(ev_sweep / ev_single, 4), "sweep/A": round(ev_sweep / base, 4),
                                              "expected VALU ratio": round(expected_ratio(mode_name, s), 4)}
        emit({"mode": mode_name, "build_digest": _lib.build_digest(), "held_clock_ghz_step_A": round(clock, 4), "ratios": ratios})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
