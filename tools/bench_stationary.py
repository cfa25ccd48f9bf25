"""Stationary-bootstrap step beside the table-mode final-value step and the block-bootstrap step, INTERLEAVED in one
process.

n_paths x n_periods (default 1e8 x 360 on the bundled 1127 months: configs[2] of bench.py), final values + statistics
(100 buckets).  One round is A, B, then S at every mean run length; --reps rounds after one warm-up round, so that clock
drift falls on all sides alike.  Per step the HIP-event time between its first and last launch; per variant the median,
the spread (max - min) and the clock the chip held in the kernel (smmc_engine_kernel_clock).
  A        simulate, table mode (paths_kernel)               -- the yardstick; the parent commit's instructions
  B12      simulate_blocks at block length 12 (blocks_kernel, the default read form)
  S<m>     simulate_stationary at a mean run of m periods, renew_q16 = round(65536 / m); S0: renew_q16 = 0, one run
One JSON line per variant and one with the ratios over A (never a ratio of the stationary step to itself).  Usage:
  python tools/bench_stationary.py [--paths N] [--periods P] [--means 1,3,12,60] [--reps K] [--out FILE]
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
from stock_market_monte_carlo_amd import _lib, stationary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100_000_000)
    ap.add_argument("--periods", type=int, default=360)
    ap.add_argument("--means", default="1,3,12,60")
    ap.add_argument("--block-len", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    eng.set_table(S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv")))
    eng.timing(True)
    final = torch.empty(n, dtype=torch.float32, device=dev)
    rec = torch.empty(int(L.smmc_stats_bytes(bins)), dtype=torch.uint8, device=dev)
    sim = S.Engine.make_sim(n, p, S.MODE_TABLE, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
    stream = torch.cuda.current_stream(dev)
    outputs = (C.c_void_p(final.data_ptr()), None, None, C.c_void_p(rec.data_ptr()))

    def step_a():
        _lib.check(L.smmc_engine_simulate(h, C.byref(sim), *outputs))

    blocks = S.Engine.make_blocks(a.block_len)

    def step_b():
        _lib.check(L.smmc_engine_simulate_blocks(h, C.byref(sim), C.byref(blocks), *outputs))

    def step_s(st):
        def step():
            _lib.check(L.smmc_engine_simulate_stationary(h, C.byref(sim), C.byref(st), *outputs))
        return step

    variants = [("A", step_a, None), (f"B{a.block_len}", step_b, None)]
    for m in [int(v) for v in a.means.split(",")]:
        st = stationary.make_stationary(mean_block_len=m)
        variants.append((f"S{m}", step_s(st), st.renew_q16))
    variants.append(("S0", step_s(stationary.make_stationary(renew_q16=0)), 0))
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
        emit({"step": name, "renew_q16": q, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": a.reps, "event_ms": round(med[name], 4),
              "spread_ms": round(max(t) - min(t), 4), "event_ms_all": [round(v, 4) for v in t],
              "ps_per_path_period": round(med[name] / n / max(p, 1) * 1e9, 4),
              "held_clock_ghz": round(statistics.median(ck), 4) if ck else None})
    emit({"build_digest": _lib.build_digest(), "ratios_over_A": {k: round(v / med["A"], 4) for k, v in med.items() if k != "A"}})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
