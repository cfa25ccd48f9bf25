"""Guardrail withdrawals beside the portfolio cash-flow step of the same K, in ONE child process.

Both modes at n_paths x n_periods (default 1e8 x 360), K = 1, 2, 4 assets, reviewed and rebalanced every 12 periods: a
starting amount of 4.0 per period, indexed by 2 % a review, cut by 10 % above 0.6 % of the value, raised by 10 % below
0.3 %, clamped to [2, 8], floor 0.01.  Warm-up 1, median of --reps (>= 5) steps; per step the wall time (enqueue to drained
stream) and the HIP-event time between the step's first and last launch.  Outputs are allocated once, outside the timed
region.
  A      simulate(final + statistics, 100 buckets): the plain step, whose clock probe gives the clock held
  X<K>   simulate_portfolio_cashflow with K assets and the constant amount 4.0, forced to SMMC_FLAG_EXACT_DIV: the
         like-for-like parent (guardrails_kernel always takes the IEEE divide)
  C<K>   the same at the divide the host chooses for it (fast, for one constant amount)
  G<K>   simulate_guardrails: final + statistics + depletion counts + the two count arrays (no further per-path output,
         as the parents)
Table mode: column k of the joint table is the bundled table rotated by 97 k months.  Gaussian mode: means 0.5 %, standard
deviations 0.83333 %, every correlation 0.3.  One JSON line per measurement, then per mode the clock the chip held under
step A (smmc_engine_kernel_clock) and per K the ratios G<K> / X<K> and G<K> / C<K>.

The expectation to test: an ordinary period costs the exact-divide parent's, so G<K> / X<K> is near the by-source
instruction ratio ("Guardrails"); what lies above it is written down in profiles/guardrails/README.md.

The measuring runs in a child process (started here, nothing of the GPU is touched before); in it every GPU step runs
under a time limit of its own (--step-limit seconds, an alarm with its default action): a step that overruns ends the
child at once, nothing more is started and this program returns 124.
Usage:
  python tools/bench_guardrails.py [--paths N] [--periods P] [--reps K] [--every R] [--review E] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import signal
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = {0: "fast", 1: "exact", 2: "checked"}


def weights(K):
    """0.6 / 0.4, 0.5 / 0.3 / 0.2, ...: the first asset holds the most."""
    return {1: [1.0], 2: [0.6, 0.4], 3: [0.5, 0.3, 0.2], 4: [0.4, 0.3, 0.2, 0.1]}[K]


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import torch

    import stock_market_monte_carlo_amd as S
    from bench_cashflow import measure
    from stock_market_monte_carlo_amd import _lib

    # SIGALRM keeps its default action: the child ends AT ONCE, also inside a HIP call that never returns (a Python handler
    # would run only after the call)
    def limited(fn, *args):
        signal.alarm(a.step_limit)
        try:
            return fn(*args)
        finally:
            signal.alarm(0)

    reps = max(a.reps, 5)
    n, p, bins = a.paths, a.periods, a.bins
    eng = S.Engine(0)
    L, h, dev = eng._L, eng._h, eng.tdevice
    table = S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv"))
    eng.set_table(table)
    final = torch.empty(n, dtype=torch.float32, device=dev)
    record = torch.empty(int(L.smmc_stats_bytes(bins)), dtype=torch.uint8, device=dev)
    depleted, cuts_at, raises_at = (torch.empty(p + 1, dtype=torch.int64, device=dev) for _ in range(3))
    cf, keep = S.Engine.make_cashflow(p, amount=a.amount, floor=0.01)
    gr = S.Engine.make_guardrails(a.amount, a.review, upper=0.006, lower=0.003, cut=0.9, raise_=1.1, index=1.02, amount_min=0.5 * a.amount,
                                  amount_max=2.0 * a.amount, floor=0.01)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out_c = _lib.PortfolioCashflowOutputs()
    out_c.struct_size = C.sizeof(_lib.PortfolioCashflowOutputs)
    out_c.final, out_c.stats, out_c.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    out_g = _lib.GuardrailsOutputs()
    out_g.struct_size = C.sizeof(_lib.GuardrailsOutputs)
    out_g.final, out_g.stats, out_g.depleted_at = final.data_ptr(), record.data_ptr(), depleted.data_ptr()
    out_g.cuts_at, out_g.raises_at = cuts_at.data_ptr(), raises_at.data_ptr()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for mode_name, mode in (("table", S.MODE_TABLE), ("gaussian", S.MODE_GAUSSIAN)):
        sim = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0)
        sim_x = S.Engine.make_sim(n, p, mode, 12345, n_bins=bins, hist_lo=0.0, hist_hi=20000.0, exact_div=True)

        def law(K):
            if mode == S.MODE_TABLE:
                return {}
            return dict(means=[0.5] * K, factor=S.cholesky_factor([0.83333] * K, np.full((K, K), 0.3) + 0.7 * np.eye(K)))

        def step_a():
            eng._enter()
            _lib.check(L.smmc_engine_simulate(h, C.byref(sim), ptr(final), None, None, ptr(record)))

        def step_c(pf, which):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_portfolio_cashflow(h, C.byref(which), C.byref(pf), C.byref(cf), C.byref(out_c)))
            return step

        def step_g(pf):
            def step():
                eng._enter()
                _lib.check(L.smmc_engine_simulate_guardrails(h, C.byref(sim), C.byref(pf), C.byref(gr), C.byref(out_g)))
            return step

        def line(name, wall, ev, all_ev, divide, **more):
            emit(dict({"mode": mode_name, "step": name, "n_paths": n, "n_periods": p, "n_bins": bins, "reps": reps,
                       "wall_ms": round(wall, 4), "event_ms": round(ev, 4), "event_ms_all": [round(x, 4) for x in all_ev],
                       "ns_per_path": round(ev / n * 1e6, 4), "divide": divide}, **more))

        wall, ev, all_ev = limited(measure, eng, step_a, reps)
        line("A_simulate_final_stats", wall, ev, all_ev, KIND[eng.divide_kind(sim)])
        own, forced, rails, shares = {}, {}, {}, {}
        for K in (1, 2, 4):
            if mode == S.MODE_TABLE:
                eng.set_asset_table(np.stack([np.roll(table, 97 * k) for k in range(K)], axis=1))
            pf = S.Engine.make_portfolio(weights(K), a.every, **law(K))
            more = dict(n_assets=K, rebalance_every=a.every, amount=a.amount)
            wall, ev, all_ev = limited(measure, eng, step_c(pf, sim_x), reps)
            forced[K] = ev
            line(f"X{K}_portfolio_cashflow_exact_div", wall, ev, all_ev,
                 KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim_x), C.byref(pf), C.byref(cf))], **more)
            wall, ev, all_ev = limited(measure, eng, step_c(pf, sim), reps)
            own[K] = ev
            line(f"C{K}_portfolio_cashflow_own_divide", wall, ev, all_ev,
                 KIND[L.smmc_engine_portfolio_cashflow_divide_kind(h, C.byref(sim), C.byref(pf), C.byref(cf))], **more)
            wall, ev, all_ev = limited(measure, eng, step_g(pf), reps)
            rails[K] = ev
            eng.sync()
            shares[K] = dict(depleted=round(1.0 - int(depleted[0].item()) / n, 4), cuts_per_path=round(int(cuts_at.sum().item()) / n, 4),
                             raises_per_path=round(int(raises_at.sum().item()) / n, 4))
            line(f"G{K}_guardrails_final_stats_counts", wall, ev, all_ev, "exact", review_every=a.review, **more, **shares[K])

        def clock():
            eng.timing(True)
            step_a()
            eng.kernel_ms()
            step_a()
            ghz = eng.kernel_clock_ghz()
            eng.timing(False)
            return ghz
        emit({"mode": mode_name, "build_digest": _lib.build_digest(), "held_clock_ghz_step_A": round(limited(clock), 4),
              "guardrails_over_exact_parent": {f"K{K}": round(rails[K] / forced[K], 4) for K in rails},
              "guardrails_over_own_divide_parent": {f"K{K}": round(rails[K] / own[K], 4) for K in rails}})
    del keep
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100_000_000)
    ap.add_argument("--periods", type=int, default=360)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--every", type=int, default=12)
    ap.add_argument("--review", type=int, default=12)
    ap.add_argument("--amount", type=float, default=4.0)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--step-limit", type=int, default=60, help="seconds a measured step (warm-up and repetitions) may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    # this process never touches the GPU: the measuring happens in ONE fresh child, bounded as a whole as well
    whole = 15 * a.step_limit
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=whole).returncode
        if rc == -signal.SIGALRM:
            sys.stderr.write("bench_guardrails: a step passed its time limit; nothing more was started\n")
            return 124
        return rc
    except subprocess.TimeoutExpired:
        sys.stderr.write(f"bench_guardrails: the child passed {whole} s\n")
        return 124


if __name__ == "__main__":
    sys.exit(main())
