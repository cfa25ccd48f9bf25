"""Allocation sweeps beside the single portfolio cash-flow calls they replace, in ONE process.

Both modes at n_paths x n_periods (default 1e8 x 360), K = 1, 2, 4 assets, S = 1, 2, 4, 8 scenarios that differ in their
weights; every scenario takes the constant amount (default 6.0) with floor 0.01 and is rebalanced every 12 periods.  Warm-up
1, median of --reps (>= 5) steps; per step the wall time (enqueue to drained stream) and the HIP-event time between the
step's first and last launch.  Outputs are allocated once, outside the timed region.
  A        simulate(final + statistics, 100 buckets): the plain step, whose clock probe gives the clock held
  C<K>s<i> simulate_portfolio_cashflow of scenario i alone: final + statistics + depletion counts
  W<K>x<S> simulate_allocation_sweep of the scenarios 0 .. S - 1: final [S][n] + S records + S rows of depletion counts
Table mode: column k of the joint table is the bundled table rotated by 97 k months.  Gaussian mode: means 0.5 %,
standard deviations 0.83333 %, every correlation 0.3.  One JSON line per measurement (with the divide form the launch
used), then per mode the clock the chip held under step A (smmc_engine_kernel_clock) and, per (K, S), the ratio of one
sweep to the sum of its S single calls.

The condition the feature states: for S >= 2 that ratio is below 1 in every measured cell.  No cell has been measured
yet (profiles/allocation_sweep/README.md); a cell that misses the condition is to be named there and here.
Usage:
  python tools/bench_allocation_sweep.py [--paths N] [--periods P] [--reps K] [--every R] [--amount A] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import stock_market_monte_carlo_amd as S  # noqa: E402
from bench_cashflow import measure  # noqa: E402
from stock_market_monte_carlo_amd import _lib  # noqa: E402

KIND = {0: "fast", 1: "exact", 2: "checked"}
SWEEPS = (1, 2, 4, 8)


def weights(K, s):
    """Scenario s of 8: the first asset's share falls from 1 to 1/8, the others share the rest equally."""
    if K == 1:
        return [1.0]
    first = 1.0 - s / 8.0
    return [first] + [(1.0 - first) / (K - 1)] * (K - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100_000_000)
    ap.add_argument("--periods", type=int, default=360)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--every", type=int, default=12)
    ap.add_argument("--amount", type=float, default=6.0)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 5)
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    table = S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv"))
    eng.set_table(table)
    rec = int(L.smmc_stats_bytes(bins))
    final = torch.empty((max(SWEEPS), n), dtype=torch.float32, device=dev)
    record = torch.empty((max(SWEEPS), rec), dtype=torch.uint8, device=dev)
    depleted = torch.empty((max(SWEEPS), p + 1), dtype=torch.int64, device=dev)
    cf, keep = S.Engine.make_cashflow(p, amount=a.amount, floor=0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out_c = _lib.PortfolioCashflowOutputs()
    out_c.struct_size = C.sizeof(_lib.PortfolioCashflowOutputs)
    out_c.final, out_c.stats, out_c.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    out_w = _lib.AllocationSweepOutputs()
    out_w.struct_size = C.sizeof(_lib.AllocationSweepOutputs)
    out_w.final, out_w.stats, out_w.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def joint_table(K):
        return np.stack([np.roll(table, 97 * k) for k in range(K)], axis=1)

    for mode_name, mode in (("table", S.MODE_TABLE), ("gaussian", S.MODE_GAUSSIAN)):
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)

        def law(K):
            if mode == S.MODE_TABLE:
                return {}
            corr = np.full((K, K), 0.3) + 0.7 * np.eye(K)
            return dict(means=[0.5] * K, factor=S.cholesky_factor([0.83333] * K, corr))

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

        def step_c(pf):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(out_c)))
            return step

        def step_w(pfs, cfs, n_scenarios):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_allocation_sweep(h, C.byref(sim), pfs, cfs, n_scenarios, C.byref(out_w)))
            return step

        def line(name, wall, ev, all_ev, divide, **more):
            emit(dict({"mode": mode_name, "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps,
                       "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev],
                       "divide": divide}, **more))

        wall, ev, all_ev = measure(eng, step_a, reps)
        line("A_simulate_final_stats", wall, ev, all_ev, KIND[eng.divide_kind(sim)], ns_per_path=round(ev / n * 1e6, 4))
        ratios = {}
        for K in (1, 2, 4):
            if mode == S.MODE_TABLE:
                eng.set_asset_table(joint_table(K))
            single = []
            for s in range(max(SWEEPS)):
                pf = S.Engine.make_portfolio(weights(K, s), a.every, **law(K))
                wall, ev, all_ev = measure(eng, step_c(pf), reps)
                single.append(ev)
                line(f"C{K}s{s}_portfolio_cashflow_final_stats_counts", wall, ev, all_ev,
                     KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf))], n_assets=K, scenario=s,
                     rebalance_every=a.every, amount=a.amount)
            for n_scenarios in SWEEPS:
                pfs, cfs = S.Engine.make_allocation_sweep([weights(K, s) for s in range(n_scenarios)], a.every, a.amount, 0.0, 0.01, **law(K))[:2]
                wall, ev, all_ev = measure(eng, step_w(pfs, cfs, n_scenarios), reps)
                total = sum(single[:n_scenarios])
                ratios[f"W{K}x{n_scenarios}"] = round(ev / total, 4)
                line(f"W{K}x{n_scenarios}_allocation_sweep_final_stats_counts", wall, ev, all_ev,
                     KIND[L.smmc_engine_allocation_sweep_divide_kind(h, C.byref(sim), pfs, cfs, n_scenarios)], n_assets=K,
                     n_scenarios=n_scenarios, rebalance_every=a.every, amount=a.amount, sum_of_single_calls_ms=round(total, 4),
                     ratio_to_single_calls=round(ev / total, 4))
        eng.timing(True)
        step_a()
        eng.kernel_ms()
        step_a()
        clock = eng.kernel_clock_ghz()
        eng.timing(False)
        emit({"mode": mode_name, "build_digest": _lib.build_digest(), "held_clock_ghz_step_A": round(clock, 4),
              "sweep_over_sum_of_single_calls": ratios})
    del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
