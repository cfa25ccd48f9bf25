"""The cash-flow arithmetic of include/smmc.h (smmc_engine_simulate_cashflow) restated in numpy float32, over the
CPU oracle's per-path returns: the reference of tests/test_cashflow_cpu.py and tests/test_cashflow_gpu.py.

Every operation is one binary32 rounding (numpy float32 arithmetic never fuses).  The oracle's returns r reproduce
the engine's multiplier as 100.0f + r, and total * a / 100 exactly, for a in [50, 200]: the bundled table
(-15.1 .. +14.3 %), the tests' 3001-entry table (+-25 %) and the default Gaussian stay inside that."""
import ctypes
import functools

import numpy as np

f32 = np.float32
SEED = 0x5EED0123456789AB
FIRST_PATH = 3
CAPITAL = 1000.0
FLOOR = 0.01


def big_table():
    """3001 entries: above the 2048 up to which a Philox block yields eight draws, so the four-draw form runs."""
    rng = np.random.default_rng(5)
    return rng.normal(0.6, 4.0, 3001).clip(-25.0, 25.0).astype(np.float32)


def returns(oracle, mode, table, n_paths, n_periods, first_path=FIRST_PATH, seed=SEED):
    """[n_paths, n_periods] percent returns of paths first_path .. (counter stream v3)."""
    p = oracle.make_params(mode, n_periods, n_paths, seed, first_path=first_path, initial_capital=CAPITAL, table=table)
    R = np.empty((n_paths, n_periods), dtype=f32)
    # oracle.counter_path_returns row by row, written in place: a launch that walks its chunks twice has 1e5 paths
    fill, ref, row, step = oracle.lib().orc_counter_path_returns, ctypes.byref(p), R.ctypes.data, 4 * n_periods
    for i in range(n_paths):
        fill(ref, first_path + i, row + i * step)
    return R


def simulate(R, amount=0.0, fraction=0.0, floor=0.0, capital=CAPITAL):
    """(final, paid, ruin_period, depleted_at) for the returns R [n, P]; amount / fraction: scalars or [P] arrays."""
    n, P = R.shape
    am = np.broadcast_to(np.asarray(amount, f32), (P,))
    fr = np.broadcast_to(np.asarray(fraction, f32), (P,))
    floor = f32(floor)
    v = np.full(n, capital, f32)
    paid = np.zeros(n, f32)
    ruin = np.zeros(n, np.uint32)
    alive = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for t in range(P):
            a = f32(100.0) + R[:, t]
            g = (v * a) / f32(100.0)            # update_fund
            w = am[t] + g * fr[t]               # the product is rounded, then the sum
            nv = g - w
            ok = nv > floor                     # False for NaN
            dies = alive & ~ok
            pay = np.where(ok, w, np.fmax(g, f32(0.0)))
            paid = np.where(alive, paid + pay, paid).astype(f32)
            ruin[dies] = t + 1
            alive &= ok
            v = np.where(alive, nv, f32(0.0)).astype(f32)
    depleted_at = np.bincount(ruin, minlength=P + 1).astype(np.uint64)
    return v, paid, ruin, depleted_at


@functools.lru_cache(maxsize=None)
def _cached_returns(oracle, mode, table_key, n_paths, n_periods):
    from conftest import load_table
    table = {"none": None, "bundled": load_table(), "big": big_table()}[table_key]
    R = returns(oracle, mode, table, n_paths, n_periods)
    R.setflags(write=False)
    return R


def cached_returns(oracle, mode, table_key, n_paths, n_periods):
    """Computed once per (mode, table, periods) and shared: never modified."""
    return _cached_returns(oracle, mode, table_key, n_paths, n_periods)
