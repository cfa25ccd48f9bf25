"""Real cash flows beside the portfolio cash-flow calls that bracket them, in ONE process.

Both modes at n_paths x n_periods (default 1e8 x 360), K = 1, 2, 3 invested assets, a constant amount (default 6.0, in
money of period 0 for the real call) with floor 0.01, rebalanced every 12 periods.  Warm-up 1, median of --reps (>= 5)
steps; per step the wall time (enqueue to drained stream) and the HIP-event time between the step's first and last
launch.  Outputs are allocated once, outside the timed region.
  A      simulate(final + statistics, 100 buckets): the plain step, whose clock probe gives the clock held
  C<K>   simulate_portfolio_cashflow with K assets: final + statistics + depletion counts
  R<K>   simulate_real_cashflow with K assets and the inflation series: final + final_real + statistics + depletion counts
  C<K+1> simulate_portfolio_cashflow with K + 1 assets
  X<K>   C<K> with SMMC_FLAG_EXACT_DIV: a constant withdrawal is FAST in the parent's divide rule and EXACT in the real
         call's (the nominal amount varies), so R<K> is bracketed by the parents forced to the same divide
Table mode: column k of the joint table is the bundled table rotated by 97 k months; the inflation column is
0.25 + 0.1 x the column rotated by 97 K.  Gaussian mode: means 0.5 %, standard deviations 0.83333 %, every correlation
0.3; inflation 0.25 % +- 0.4 %.  One JSON line per measurement (with the divide form the launch used), then per mode the
clock the chip held under step A (smmc_engine_kernel_clock) and, per K, R<K> / X<K> and R<K> / X<K+1> (and the same
against C<K>, C<K+1>).

The expectation the feature states: X<K> <= R<K> <= X<K+1> -- the extra series costs a draw but no compounding chain per
weight.  A cell outside that bracket is to be named in profiles/real_cashflow/README.md with the instruction counts of
profiles/real_cashflow/isa.txt that explain it.
Usage:
  python tools/bench_real_cashflow.py [--paths N] [--periods P] [--reps K] [--every R] [--amount A] [--out FILE]
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


def weights(K):
    """0.6 / 0.4, 0.5 / 0.3 / 0.2, ...: the first asset holds the most."""
    return {1: [1.0], 2: [0.6, 0.4], 3: [0.5, 0.3, 0.2], 4: [0.4, 0.3, 0.2, 0.1]}[K]


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
    final = torch.empty(n, dtype=torch.float32, device=dev)
    final_real = torch.empty(n, dtype=torch.float32, device=dev)
    record = torch.empty(rec, dtype=torch.uint8, device=dev)
    depleted = torch.empty(p + 1, dtype=torch.int64, device=dev)
    cf, keep = S.Engine.make_cashflow(p, amount=a.amount, floor=0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out_c = _lib.PortfolioCashflowOutputs()
    out_c.struct_size = C.sizeof(_lib.PortfolioCashflowOutputs)
    out_c.final, out_c.stats, out_c.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    out_r = _lib.RealCashflowOutputs()
    out_r.struct_size = C.sizeof(_lib.RealCashflowOutputs)
    out_r.final, out_r.final_real, out_r.stats, out_r.depleted_at = final.data_ptr(), final_real.data_ptr(), record.data_ptr(), depleted.data_ptr()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def joint_table(K, inflation):
        cols = [np.roll(table, 97 * k) for k in range(K)]
        if inflation:
            cols.append((0.25 + 0.1 * np.roll(table, 97 * K)).astype(np.float32))
        return np.stack(cols, axis=1)

    for mode_name, mode in (("table", S.MODE_TABLE), ("gaussian", S.MODE_GAUSSIAN)):
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
        sim_x = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0, exact_div=True)

        def law(K, inflation):
            if mode == S.MODE_TABLE:
                return {}
            width = K + (1 if inflation else 0)
            corr = np.full((width, width), 0.3) + 0.7 * np.eye(width)
            return dict(means=[0.5] * K + ([0.25] if inflation else []),
                        factor=S.cholesky_factor([0.83333] * K + ([0.4] if inflation else []), corr))

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

        def step_c(pf, which=None):
            which = sim if which is None else which

            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow(h, C.byref(which), C.byref(pf), C.byref(cf), C.byref(out_c)))
            return step

        def step_r(pf):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_real_cashflow(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(out_r)))
            return step

        def line(name, wall, ev, all_ev, divide, **more):
            emit(dict({"mode": mode_name, "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps,
                       "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev],
                       "ns_per_path": round(ev / n * 1e6, 4), "divide": divide}, **more))

        wall, ev, all_ev = measure(eng, step_a, reps)
        line("A_simulate_final_stats", wall, ev, all_ev, KIND[eng.divide_kind(sim)])
        parent, forced, real = {}, {}, {}
        for K in (1, 2, 3, 4):
            if mode == S.MODE_TABLE:
                eng.set_asset_table(joint_table(K, False))
            pf = S.Engine.make_portfolio(weights(K), a.every, **law(K, False))
            wall, ev, all_ev = measure(eng, step_c(pf), reps)
            parent[K] = ev
            line(f"C{K}_portfolio_cashflow_final_stats_counts", wall, ev, all_ev,
                 KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf))], n_assets=K,
                 rebalance_every=a.every, amount=a.amount)
            wall, ev, all_ev = measure(eng, step_c(pf, sim_x), reps)
            forced[K] = ev
            line(f"X{K}_portfolio_cashflow_exact_div", wall, ev, all_ev,
                 KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim_x), C.byref(pf), C.byref(cf))], n_assets=K,
                 rebalance_every=a.every, amount=a.amount)
            if K == 4:
                break
            if mode == S.MODE_TABLE:
                eng.set_asset_table(joint_table(K, True))
            pf = S.Engine.make_real_portfolio(weights(K), a.every, **law(K, True))
            wall, ev, all_ev = measure(eng, step_r(pf), reps)
            real[K] = ev
            line(f"R{K}_real_cashflow_final_real_stats_counts", wall, ev, all_ev,
                 KIND[L.smmc_engine_real_cashflow_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf))], n_assets=K,
                 rebalance_every=a.every, amount=a.amount)
        eng.timing(True)
        step_a()
        eng.kernel_ms()
        step_a()
        clock = eng.kernel_clock_ghz()
        eng.timing(False)
        emit({"mode": mode_name, "build_digest": _lib.build_digest(), "held_clock_ghz_step_A": round(clock, 4),
              "real_over_parent_same_k": {f"K{K}": round(real[K] / parent[K], 4) for K in real},
              "real_over_parent_k_plus_1": {f"K{K}": round(real[K] / parent[K + 1], 4) for K in real},
              "real_over_exact_parent_same_k": {f"K{K}": round(real[K] / forced[K], 4) for K in real},
              "real_over_exact_parent_k_plus_1": {f"K{K}": round(real[K] / forced[K + 1], 4) for K in real},
              "inside_the_bracket_of_exact_parents": {f"K{K}": bool(forced[K] <= real[K] <= forced[K + 1]) for K in real}})
    del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
