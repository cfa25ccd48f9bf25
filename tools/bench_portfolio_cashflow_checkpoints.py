"""Portfolio cash-flow checkpoints beside the portfolio cash-flow step of the same K, in ONE process.

Both modes at n_paths x n_periods (default 1e8 x 360), rebalanced every 12 periods, a constant amount, floor 0.01,
warm-up 1, median of --reps (>= 5) steps; per step the wall time (enqueue to drained stream) and the HIP-event time
between the step's first and last launch.  Outputs are allocated once, outside the timed region.
  A           simulate(final + statistics, 100 buckets): the final-value step, whose clock probe gives the clock held
  C1, C2, C4  simulate_portfolio_cashflow with K = 1, 2, 4 assets, final + statistics + depletion counts
  K1, K2, K4  simulate_portfolio_cashflow_checkpoints with the same requests and --checkpoints (default 30) checkpoints,
              every n_periods / checkpoints periods ("yearly" at 360 / 30), the same buckets per record
The C and K steps of one K alternate (C1, K1, C2, K2, ...), so that a drift of the board's clock meets both.  Table mode:
column k of the joint table is the bundled table rotated by 97 k months.  Gaussian mode: means 0.5 %, standard deviations
0.83333 %, every correlation 0.3.  One JSON line per measurement (with the divide form the launch used and the spread of
its repetitions), then the clock the chip held under step A (smmc_engine_kernel_clock) sampled before and after the
mode's steps, then the ratios K_K / C_K.
Usage:
  python tools/bench_portfolio_cashflow_checkpoints.py [--paths N] [--periods P] [--reps K] [--every R] [--amount A]
                                                        [--checkpoints N] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100_000_000)
    ap.add_argument("--periods", type=int, default=360)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--every", type=int, default=12)
    ap.add_argument("--amount", type=float, default=6.0)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--checkpoints", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 5)
    n, p, bins = a.paths, a.periods, a.bins
    stride = max(p // a.checkpoints, 1)
    periods = np.arange(stride, p + 1, stride, dtype=np.uint32)[: a.checkpoints]
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    table = S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv"))
    eng.set_table(table)
    rec = int(L.smmc_stats_bytes(bins))
    final = torch.empty(n, dtype=torch.float32, device=dev)
    record = torch.empty(rec, dtype=torch.uint8, device=dev)
    records = torch.empty(rec * periods.size, dtype=torch.uint8, device=dev)
    depleted = torch.empty(p + 1, dtype=torch.int64, device=dev)
    cf, keep = S.Engine.make_cashflow(p, amount=a.amount, floor=0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out_c = _lib.PortfolioCashflowOutputs()
    out_c.struct_size = C.sizeof(_lib.PortfolioCashflowOutputs)
    out_c.final, out_c.stats, out_c.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def joint_table(K):
        return np.stack([np.roll(table, 97 * k) for k in range(K)], axis=1)

    for mode_name, mode in (("table", S.MODE_TABLE), ("gaussian", S.MODE_GAUSSIAN)):
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

        def held_clock():
            eng.timing(True)
            step_a()
            eng.kernel_ms()
            step_a()
            clock = eng.kernel_clock_ghz()
            eng.timing(False)
            return clock

        def portfolio(K):
            if mode == S.MODE_TABLE:
                return S.Engine.make_portfolio([1.0 / K] * K, a.every)
            corr = np.full((K, K), 0.3) + 0.7 * np.eye(K)
            return S.Engine.make_portfolio([1.0 / K] * K, a.every, means=[0.5] * K, factor=S.cholesky_factor([0.83333] * K, corr))

        def step_c(pf):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(out_c)))
            return step

        def step_k(pf):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow_checkpoints(
                    h, C.byref(sim), C.byref(pf), C.byref(cf), periods.ctypes.data_as(C.c_void_p), periods.size, C.byref(out_c), ptr(records)))
            return step

        res, spread = {}, {}
        steps = [("A_simulate_final_stats", step_a, None, KIND[eng.divide_kind(sim)])]
        for K in (1, 2, 4):
            pf = portfolio(K)
            if mode == S.MODE_TABLE:  # the divide rule reads the joint table of this K
                eng.set_asset_table(joint_table(K))
            divide = KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf))]
            steps.append((f"C{K}_portfolio_cashflow_final_stats_counts", step_c(pf), pf, divide))
            steps.append((f"K{K}_portfolio_cashflow_checkpoints_final_stats_counts_records", step_k(pf), pf, divide))
        clock_before = held_clock()
        for name, fn, pf, divide in steps:
            if pf is not None and mode == S.MODE_TABLE:
                eng.set_asset_table(joint_table(int(pf.n_assets)))
            wall, ev, all_ev = measure(eng, fn, reps)
            res[name] = ev
            spread[name] = (max(all_ev) - min(all_ev)) / ev
            line = {"mode": mode_name, "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps,
                    "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev],
                    "spread": round(spread[name], 4), "ns_per_path": round(ev / n * 1e6, 4), "divide": divide}
            if pf is not None:
                line["rebalance_every"], line["amount"] = a.every, a.amount
            if name[0] == "K":
                line["n_checkpoints"], line["first_period"], line["last_period"] = int(periods.size), int(periods[0]), int(periods[-1])
            emit(line)
        clock_after = held_clock()
        ratios = {f"K{K}/C{K}": round(res[f"K{K}_portfolio_cashflow_checkpoints_final_stats_counts_records"]
                                      / res[f"C{K}_portfolio_cashflow_final_stats_counts"], 4) for K in (1, 2, 4)}
        parent_spread = {f"C{K}": round(spread[f"C{K}_portfolio_cashflow_final_stats_counts"], 4) for K in (1, 2, 4)}
        emit({"mode": mode_name, "build_digest": _lib.build_digest(), "held_clock_ghz_step_A_before": round(clock_before, 4),
              "held_clock_ghz_step_A_after": round(clock_after, 4), "ratios": ratios, "parent_spread": parent_spread})
    del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
