"""Regime-switching Gaussian step beside the plain Gaussian step and the Gaussian portfolio step of one asset, INTERLEAVED
in one process.

n_paths x n_periods (default 1e8 x 360), final values + statistics (100 buckets).  One round is G, P1, every regime
variant, then P1 again; --reps rounds after one warm-up round, so that clock drift falls on all sides alike.  Per step the
HIP-event time between its first and last launch; per variant the median, the spread (max - min) and the clock the chip held
in the kernel (smmc_engine_kernel_clock).
  G         simulate, Gaussian mode (paths_kernel)                          -- the clock is reported under this step
  P1, P1'   simulate_portfolio, one Gaussian asset (portfolio_kernel<1>), timed twice per round: the difference of the two
            medians and their spreads are the yardstick for "the same"
  R1-1      simulate_regimes at mean durations (1, 1): the state flips every period
  R40-8     ... (40, 8)
  Rinf      ... leave_q16 = (0, 0), start 1/2: no path ever changes its regime
  Requal    ... (40, 8) with equal regimes: the values of P1
One JSON line per variant and one with the ratios over P1 and over G (never a ratio of the regime step to itself).  No ratio
is expected in advance: profiles/regimes/isa.txt holds the instruction counts to read them against.  Usage:
  python tools/bench_regimes.py [--paths N] [--periods P] [--reps K] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import stock_market_monte_carlo_amd as S  # noqa: E402
from stock_market_monte_carlo_amd import _lib, regimes  # noqa: E402

MEANS, STDS = (0.9, -1.5), (3.5, 7.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100_000_000)
    ap.add_argument("--periods", type=int, default=360)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    eng.timing(True)
    final = torch.empty(n, dtype=torch.float32, device=dev)
    rec = torch.empty(int(L.smmc_stats_bytes(bins)), dtype=torch.uint8, device=dev)
    sim = S.Engine.make_sim(n, p, S.MODE_GAUSSIAN, 12345, gauss_mean=MEANS[0], gauss_std=STDS[0], n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
    stream = torch.cuda.current_stream(dev)
    outputs = (C.c_void_p(final.data_ptr()), None, None, C.c_void_p(rec.data_ptr()))

    def step_g():
        _lib.check(L.smmc_engine_simulate(h, C.byref(sim), *outputs))

    pf = S.Engine.make_portfolio((1.0,), 0, means=(MEANS[0],), factor=((STDS[0],),))
    po = _lib.PortfolioOutputs()
    po.struct_size, po.final, po.stats = C.sizeof(_lib.PortfolioOutputs), final.data_ptr(), rec.data_ptr()

    def step_p():
        _lib.check(L.smmc_engine_simulate_portfolio(h, C.byref(sim), C.byref(pf), C.byref(po)))

    def step_r(rg):
        def step():
            _lib.check(L.smmc_engine_simulate_regimes(h, C.byref(sim), C.byref(rg), *outputs))
        return step

    cases = [("R1-1", regimes.make_regimes(MEANS, STDS, mean_durations=(1, 1))),
             ("R40-8", regimes.make_regimes(MEANS, STDS, mean_durations=(40, 8))),
             ("Rinf", regimes.make_regimes(MEANS, STDS, leave_q16=(0, 0), start=0.5)),
             ("Requal", regimes.make_regimes((MEANS[0],) * 2, (STDS[0],) * 2, mean_durations=(40, 8)))]
    variants = [("G", step_g, None), ("P1", step_p, None)]
    variants += [(name, step_r(rg), [int(rg.leave_q16[0]), int(rg.leave_q16[1]), int(rg.start1_q16)]) for name, rg in cases]
    variants.append(("P1'", step_p, None))
    times = {name: [] for name, _, _ in variants}
    clocks = {name: [] for name, _, _ in variants}
    for it in range(a.reps + 1):  # round 0 is the warm-up
        for name, fn, _ in variants:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            eng.sync()
            eng._enter()
            t0.record(stream)
            fn()
            t1.record(stream)
            eng.sync()
            if it:
                times[name].append(t0.elapsed_time(t1))
                clocks[name].append(eng.kernel_clock_ghz())
            eng.kernel_ms()  # hands the timing events back
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    med = {}
    for name, _, q in variants:
        t = times[name]
        med[name] = statistics.median(t)
        ck = [c for c in clocks[name] if c]
        emit({"step": name, "leave_q16_start1_q16": q, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": a.reps,
              "event_ms": round(med[name], 4), "spread_ms": round(max(t) - min(t), 4), "event_ms_all": [round(v, 4) for v in t],
              "ps_per_path_period": round(med[name] / n / max(p, 1) * 1e9, 4),
              "held_clock_ghz": round(statistics.median(ck), 4) if ck else None})
    emit({"build_digest": _lib.build_digest(),
          "ratios_over_P1": {k: round(v / med["P1"], 4) for k, v in med.items() if k != "P1"},
          "ratios_over_G": {k: round(v / med["G"], 4) for k, v in med.items() if k != "G"}})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
