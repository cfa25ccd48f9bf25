"""Regime-switching plans beside the Gaussian portfolio cash-flow step of the same K and divide, the one-asset regime step
and the plain Gaussian step, in ONE process.

Gaussian mode at n_paths x n_periods (default 1e8 x 360), equal weights, rebalanced every 12 periods, one constant amount
with floor 0.01; regime 0: means 0.8, deviations 4, correlations 0.1; regime 1: means -1.0, deviations 6, correlations 0.6.
Warm-up 1, median of --reps (>= 5) steps; per step the wall time (enqueue to drained stream) and the HIP-event time between
the step's first and last launch.  Outputs are allocated once, outside the timed region.
  A             simulate(final + statistics, 100 buckets): the plain Gaussian step, whose clock probe gives the clock held
  G             simulate_regimes(final + statistics) at mean durations (40, 8): the one-asset regime step
  C1, C2, C4    simulate_portfolio_cashflow with K = 1, 2, 4 assets under regime 0's law, final + statistics + depletion
                counts: the parent, timed TWICE per K (before and after that K's other steps): its own run-to-run spread
  M<K>_<p>      simulate_portfolio_cashflow_regimes at p = d1_1 (mean durations 1, 1), d40_8, never (regime 0 never left) and
                equal (both regimes hold regime 0's law)
One JSON line per measurement (with the divide form the launch used), then the clock the chip held under step A
(smmc_engine_kernel_clock), the parent's spread per K ((max - min) / median over all its timed steps) and the ratios over
C<K> -- refused where the regime step's divide is not the parent's --: a ratio beyond what the count by source explains, by more than that spread, is a finding for
profiles/portfolio_cashflow_regimes/README.md.
Usage:
  python tools/bench_regime_plan.py [--paths N] [--periods P] [--reps K] [--every R] [--amount A] [--out FILE]
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
from stock_market_monte_carlo_amd import _lib, regimes  # noqa: E402
from stock_market_monte_carlo_amd.engine import cholesky_factor  # noqa: E402

KIND = {0: "fast", 1: "exact", 2: "checked"}
ASSETS = (1, 2, 4)


def law(K, mean, std, rho):
    corr = np.full((K, K), rho) + (1.0 - rho) * np.eye(K)
    return [mean] * K, cholesky_factor([std] * K, corr)


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
    final = torch.empty(n, dtype=torch.float32, device=dev)
    record = torch.empty(int(L.smmc_stats_bytes(bins)), dtype=torch.uint8, device=dev)
    depleted = torch.empty(p + 1, dtype=torch.int64, device=dev)
    cf, keep = S.Engine.make_cashflow(p, amount=a.amount, floor=0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out_c = _lib.PortfolioCashflowOutputs()
    out_c.struct_size = C.sizeof(_lib.PortfolioCashflowOutputs)
    out_c.final, out_c.stats, out_c.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    sim = S.Engine.make_sim(n, p, S.MODE_GAUSSIAN, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0, gauss_mean=0.8, gauss_std=4.0)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def timed(name, fn, divide, **more):
        wall, ev, all_ev = measure(eng, fn, reps)
        emit(dict({"mode": "gaussian", "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps, "wall_ms": round(wall, 4),
                   "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev], "ns_per_path": round(ev / n * 1e6, 4),
                   "divide": divide}, **more))
        return ev, all_ev

    def step_a():
        eng._enter()
        _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

    one = regimes.make_regimes((0.8, -1.0), (4.0, 6.0), mean_durations=(40, 8))

    def step_g():
        eng._enter()
        _lib.check(L.smmc_engine_simulate_regimes(h, C.byref(sim), C.byref(one), ptr(final), None, None, ptr(record)))

    timed("A_simulate_final_stats", step_a, KIND[eng.divide_kind(sim)])
    timed("G_simulate_regimes_final_stats", step_g, KIND[L.smmc_engine_regimes_divide_kind(h, C.byref(sim), C.byref(one))])
    ratios, spread = {}, {}
    for K in ASSETS:
        (m0, f0), (m1, f1) = law(K, 0.8, 4.0, 0.1), law(K, -1.0, 6.0, 0.6)
        parent_pf = S.Engine.make_portfolio([1.0 / K] * K, a.every, means=m0, factor=f0)
        pf = S.Engine.make_portfolio([1.0 / K] * K, a.every)
        settings = {"d1_1": regimes.make_portfolio_regimes((m0, m1), (f0, f1), mean_durations=(1, 1)),
                    "d40_8": regimes.make_portfolio_regimes((m0, m1), (f0, f1), mean_durations=(40, 8)),
                    "never": regimes.make_portfolio_regimes((m0, m1), (f0, f1), leave_q16=(0, 8192), start1_q16=0),
                    "equal": regimes.make_portfolio_regimes((m0, m0), (f0, f0), mean_durations=(40, 8))}

        def step_c():
            eng._enter()
            _lib.check(L.smmc_engine_simulate_portfolio_cashflow(h, C.byref(sim), C.byref(parent_pf), C.byref(cf), C.byref(out_c)))

        def step_m(rg):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow_regimes(h, C.byref(sim), C.byref(pf), C.byref(rg), C.byref(cf),
                                                                             C.byref(out_c)))
            return step

        divide = KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim), C.byref(parent_pf), C.byref(cf))]
        common = dict(rebalance_every=a.every, amount=a.amount, n_assets=K)
        _, first = timed(f"C{K}_portfolio_cashflow_final_stats_counts", step_c, divide, **common)
        ms, kinds = {}, {}
        for name, rg in settings.items():
            kind = KIND[L.smmc_engine_portfolio_cashflow_regimes_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(rg), C.byref(cf))]
            kinds[f"M{K}_{name}"] = kind
            ms[f"M{K}_{name}"], _ = timed(f"M{K}_{name}_portfolio_cashflow_regimes_final_stats_counts", step_m(rg), kind,
                                          leave_q16=list(rg.leave_q16), start1_q16=int(rg.start1_q16), **common)
        _, second = timed(f"C{K}_portfolio_cashflow_final_stats_counts_again", step_c, divide, **common)
        parent = first + second
        med = statistics.median(parent)
        spread[f"C{K}"] = round((max(parent) - min(parent)) / med, 4)
        for name, v in ms.items():  # a ratio only beside the parent of the same divide
            ratios[f"{name}/C{K}"] = round(v / med, 4) if kinds[name] == divide else f"refused: {kinds[name]} divide beside the parent's {divide}"
    eng.timing(True)
    step_a()
    eng.kernel_ms()
    step_a()
    clock = eng.kernel_clock_ghz()
    eng.timing(False)
    emit({"mode": "gaussian", "build_digest": _lib.build_digest(), "held_clock_ghz_step_A": round(clock, 4), "parent_spread": spread,
          "ratios": ratios})
    del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
