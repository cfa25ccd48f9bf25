"""Stationary-bootstrap plans beside the portfolio cash-flow step of the same K, the block plan at L = 12 and the table-mode
final-value step, in ONE process.

Table mode at n_paths x n_periods (default 1e8 x 360) on the bundled 1127-month table widened to K columns (column k is the
table rotated by 97 k months, as tools/bench_portfolio_cashflow_blocks.py), rebalanced every 12 periods, one constant amount
with floor 0.01; warm-up 1, median of --reps (>= 5) steps; per step the wall time (enqueue to drained stream) and the
HIP-event time between the step's first and last launch.  Outputs are allocated once, outside the timed region.
  A             simulate(final + statistics, 100 buckets): the table-mode plain step, whose clock probe gives the clock held
  C1, C2, C4    simulate_portfolio_cashflow with K = 1, 2, 4 assets, final + statistics + depletion counts: the parent,
                timed TWICE per K (before and after that K's other steps): its own run-to-run spread
  B<K>_L12      simulate_portfolio_cashflow_blocks with the same portfolio and schedule at block length 12
  S<K>_M<m>     simulate_portfolio_cashflow_stationary at a mean run of m = 1, 12 periods (renew_q16 = round(65536 / m)) and
                S<K>_M0: renew_q16 = 0, one run
One JSON line per measurement (with the divide form the launch used), then the clock the chip held under step A
(smmc_engine_kernel_clock), the parent's spread per K ((max - min) / median over all its timed steps) and the ratios over
C<K>: a ratio outside what the count by source explains is a finding for profiles/portfolio_cashflow_stationary/README.md.
Usage:
  python tools/bench_stationary_plan.py [--paths N] [--periods P] [--reps K] [--every R] [--amount A] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import stock_market_monte_carlo_amd as S  # noqa: E402
from bench_cashflow import measure  # noqa: E402
from stock_market_monte_carlo_amd import _lib, stationary  # noqa: E402

KIND = {0: "fast", 1: "exact", 2: "checked"}
ASSETS = (1, 2, 4)
MEANS = (1, 12, 0)  # 0: one run
BLOCK_LEN = 12


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
    final = torch.empty(n, dtype=torch.float32, device=dev)
    record = torch.empty(int(L.smmc_stats_bytes(bins)), dtype=torch.uint8, device=dev)
    depleted = torch.empty(p + 1, dtype=torch.int64, device=dev)
    cf, keep = S.Engine.make_cashflow(p, amount=a.amount, floor=0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out_c = _lib.PortfolioCashflowOutputs()
    out_c.struct_size = C.sizeof(_lib.PortfolioCashflowOutputs)
    out_c.final, out_c.stats, out_c.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    sim = S.Engine.make_sim(n, p, S.MODE_TABLE, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def timed(name, fn, divide, **more):
        wall, ev, all_ev = measure(eng, fn, reps)
        emit(dict({"mode": "table", "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps, "wall_ms": round(wall, 4),
                   "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev], "ns_per_path": round(ev / n * 1e6, 4),
                   "divide": divide}, **more))
        return ev, all_ev

    def step_a():
        eng._enter()
        _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

    timed("A_simulate_final_stats", step_a, KIND[eng.divide_kind(sim)])
    ratios, spread = {}, {}
    blocks = S.Engine.make_blocks(BLOCK_LEN)
    for K in ASSETS:
        eng.set_asset_table(np.stack([np.roll(table, 97 * k) for k in range(K)], axis=1))
        pf = S.Engine.make_portfolio([1.0 / K] * K, a.every)

        def step_c():
            eng._enter()
            _lib.check(L.smmc_engine_simulate_portfolio_cashflow(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(out_c)))

        def step_b():
            eng._enter()
            _lib.check(L.smmc_engine_simulate_portfolio_cashflow_blocks(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(blocks),
                                                                        C.byref(out_c)))

        def step_s(st):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow_stationary(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(st),
                                                                                C.byref(out_c)))
            return step

        divide = KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf))]
        common = dict(rebalance_every=a.every, amount=a.amount, n_assets=K)
        _, first = timed(f"C{K}_portfolio_cashflow_final_stats_counts", step_c, divide, **common)
        ms = {}
        ms[f"B{K}_L{BLOCK_LEN}"], _ = timed(f"B{K}_L{BLOCK_LEN}_portfolio_cashflow_blocks_final_stats_counts", step_b, divide,
                                            block_len=BLOCK_LEN, **common)
        for m in MEANS:
            st = stationary.make_stationary(mean_block_len=m) if m else stationary.make_stationary(renew_q16=0)
            kind = KIND[L.smmc_engine_portfolio_cashflow_stationary_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(st))]
            ms[f"S{K}_M{m}"], _ = timed(f"S{K}_M{m}_portfolio_cashflow_stationary_final_stats_counts", step_s(st), kind,
                                        renew_q16=int(st.renew_q16), **common)
        _, second = timed(f"C{K}_portfolio_cashflow_final_stats_counts_again", step_c, divide, **common)
        parent = first + second
        med = statistics.median(parent)
        spread[f"C{K}"] = round((max(parent) - min(parent)) / med, 4)
        for name, v in ms.items():
            ratios[f"{name}/C{K}"] = round(v / med, 4)
    eng.timing(True)
    step_a()
    eng.kernel_ms()
    step_a()
    clock = eng.kernel_clock_ghz()
    eng.timing(False)
    emit({"mode": "table", "build_digest": _lib.build_digest(), "held_clock_ghz_step_A": round(clock, 4), "parent_spread": spread,
          "ratios": ratios})
    del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
