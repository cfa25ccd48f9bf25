"""Glide paths beside the portfolio cash-flow step of the same K, and the final-value step, in ONE process.

Both modes at n_paths x n_periods (default 1e8 x 360), K = 2 and 4, rebalanced every 12 periods, one constant amount with
floor 0.01.  Table mode: the bundled table widened to K columns (column k is the table rotated by 97 k months, as
tools/bench_portfolio_cashflow.py); Gaussian mode: means 0.6 and a lower-triangular factor (4.0 on the diagonal, 0.9 under
it).  The targets glide on a straight line (glide_linear) from 90/10 to 40/60 (K = 2) or from 40/30/20/10 to its reverse
(K = 4).  Warm-up 1, median of --reps (>= 5) steps; per step the wall time (enqueue to drained stream) and the HIP-event
time between the step's first and last launch.  Outputs are allocated once, outside the timed region.
  A                    simulate(final + statistics, 100 buckets): the final-value step, whose clock probe gives the clock held
  C<K>                 simulate_portfolio_cashflow at the starting weights, final + statistics + depletion counts: the parent,
                       timed TWICE per mode and K (before and after that K's glide steps): its own run-to-run spread
  G<K>_0 / _30 / _359  simulate_glide with no change, with 30 yearly changes on the rebalance periods (12, 24, .. 360), and
                       with 359 monthly changes (1 .. 359)
One JSON line per measurement (with the divide form the launch used), then per mode the clock the chip held under step A
(smmc_engine_kernel_clock), the parent's spread per K ((max - min) / median over all its timed steps) and the ratios
G<K>_<changes> / C<K>: a ratio above 1 by more than that spread is a finding for profiles/glide/README.md.
Usage:
  python tools/bench_glide.py [--paths N] [--periods P] [--reps K] [--every R] [--amount A] [--out FILE]
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
from stock_market_monte_carlo_amd import _lib  # noqa: E402

KIND = {0: "fast", 1: "exact", 2: "checked"}
ASSETS = (2, 4)
ENDS = {2: ((0.9, 0.1), (0.4, 0.6)), 4: ((0.4, 0.3, 0.2, 0.1), (0.1, 0.2, 0.3, 0.4))}


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
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for mode, name in ((S.MODE_TABLE, "table"), (S.MODE_GAUSSIAN, "gaussian")):
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0, gauss_mean=0.6, gauss_std=4.3)

        def timed(step, fn, divide, **more):
            wall, ev, all_ev = measure(eng, fn, reps)
            emit(dict({"mode": name, "step": step, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps, "wall_ms": round(wall, 4),
                       "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev], "ns_per_path": round(ev / n * 1e6, 4),
                       "divide": divide}, **more))
            return ev, all_ev

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

        timed("A_simulate_final_stats", step_a, KIND[eng.divide_kind(sim)])
        ratios, spread = {}, {}
        for K in ASSETS:
            w_from, w_to = ENDS[K]
            if mode == S.MODE_TABLE:
                eng.set_asset_table(np.stack([np.roll(table, 97 * k) for k in range(K)], axis=1))
                pf = S.Engine.make_portfolio(w_from, a.every)
            else:
                factor = 4.0 * np.eye(K, dtype=np.float32) + 0.9 * np.eye(K, k=-1, dtype=np.float32)
                pf = S.Engine.make_portfolio(w_from, a.every, [0.6] * K, factor)
            glides = {0: [], 30: [c for c in S.glide_linear(w_from, w_to, 0, p, a.every)],
                      359: [c for c in S.glide_linear(w_from, w_to, 0, p - 1, 1)]}

            def step_c():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(out_c)))

            def step_g(gl):
                def step():
                    eng._enter()
                    _lib.check(L.smmc_engine_simulate_glide(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(gl), C.byref(out_c)))
                return step

            divide = KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf))]
            common = dict(rebalance_every=a.every, amount=a.amount, n_assets=K)
            _, first = timed(f"C{K}_portfolio_cashflow_final_stats_counts", step_c, divide, **common)
            glide_ms = {}
            for tag, changes in glides.items():
                gl, keep_gl = S.Engine.make_glide(changes)
                kind = KIND[L.smmc_engine_glide_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(gl))]
                glide_ms[tag], _ = timed(f"G{K}_{tag}_glide_final_stats_counts", step_g(gl), kind, n_changes=len(changes), **common)
                del keep_gl
            _, second = timed(f"C{K}_portfolio_cashflow_final_stats_counts_again", step_c, divide, **common)
            parent = first + second
            med = statistics.median(parent)
            spread[f"C{K}"] = round((max(parent) - min(parent)) / med, 4)
            for tag in glides:
                ratios[f"G{K}_{tag}/C{K}"] = round(glide_ms[tag] / med, 4)
        eng.timing(True)
        step_a()
        eng.kernel_ms()
        step_a()
        clock = eng.kernel_clock_ghz()
        eng.timing(False)
        emit({"mode": name, "build_digest": _lib.build_digest(), "held_clock_ghz_step_A": round(clock, 4), "parent_spread": spread,
              "ratios": ratios})
    del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
