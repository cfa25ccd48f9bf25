"""The excursion arithmetic of include/smmc.h (smmc_engine_simulate_excursions) restated in numpy float32 over the
CPU oracle's trajectories, oracle.counter_mc(params, want_traj=True)["traj"]: the reference of
tests/test_excursions_cpu.py and tests/test_excursions_gpu.py.

Every operation is one binary32 rounding (numpy float32 arithmetic never fuses) and every comparison is false for
NaN.  The trajectories are the oracle engine's own values, so the restatement is exact for any table, which a
restatement over returns would not be."""
import functools

import numpy as np

f32 = np.float32
SEED = 0x5EED0123456789AB
FIRST_PATH = 3
CAPITAL = 1000.0
GAUSS_MEAN, GAUSS_STD = 0.6, 4.3   # the engine's default 0.83 % never takes a path below 800
N_MAX = 2 * 4099 + 1               # 8199
DD_THRESHOLD = 0.2
FIELDS = ("final", "peak", "low", "drawdown", "drawdown_period", "underwater", "first_below", "first_reach")


def levels(n_periods):
    """(lower, target) of the tests for a number of periods."""
    return (950.0, 1050.0) if n_periods <= 7 else (800.0, 2000.0)


def trajectories(oracle, mode, table, n_paths, n_periods, first_path=FIRST_PATH, seed=SEED):
    """[n_paths, n_periods + 1] values of paths first_path .. (counter stream v3); column 0 is the capital."""
    p = oracle.make_params(mode, n_periods, n_paths, seed, first_path=first_path, initial_capital=CAPITAL, table=table,
                           gauss_mean=GAUSS_MEAN, gauss_std=GAUSS_STD)
    return oracle.counter_mc(p, want_final=False, want_traj=True)["traj"]


def excursions(traj, lower, target):
    """dict of the eight per-path outputs plus first_below_at / first_reach_at for the trajectories traj [n, P + 1]."""
    traj = np.asarray(traj, dtype=f32)
    n, P = traj.shape[0], traj.shape[1] - 1
    lower, target = f32(lower), f32(target)
    v0 = traj[:, 0].copy()
    peak, low, dd_peak, dd_low = v0.copy(), v0.copy(), v0.copy(), v0.copy()
    dd_period = np.zeros(n, np.uint32)
    run = np.zeros(n, np.uint32)
    longest = np.zeros(n, np.uint32)
    first_below = np.zeros(n, np.uint32)
    first_reach = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        for t in range(1, P + 1):
            v = traj[:, t]
            peak = np.where(v > peak, v, peak)
            low = np.where(v < low, v, low)
            deeper = (v * dd_peak) < (dd_low * peak)   # float32 products, each rounded; strict; the updated peak
            dd_peak = np.where(deeper, peak, dd_peak)
            dd_low = np.where(deeper, v, dd_low)
            dd_period = np.where(deeper, np.uint32(t), dd_period)
            run = np.where(v < peak, run + np.uint32(1), np.uint32(0))
            longest = np.maximum(longest, run)
            first_below = np.where((first_below == 0) & (v < lower), np.uint32(t), first_below)
            first_reach = np.where((first_reach == 0) & (v >= target), np.uint32(t), first_reach)
        drawdown = (dd_peak - dd_low) / dd_peak       # two roundings, once per path
    assert peak.dtype == f32 and drawdown.dtype == f32 and dd_period.dtype == np.uint32
    return {"final": traj[:, P].copy(), "peak": peak, "low": low, "drawdown": drawdown, "drawdown_period": dd_period,
            "underwater": longest, "first_below": first_below, "first_reach": first_reach,
            "first_below_at": np.bincount(first_below, minlength=P + 1).astype(np.uint64),
            "first_reach_at": np.bincount(first_reach, minlength=P + 1).astype(np.uint64)}


def big_table():
    from cashflow_reference import big_table as bt
    return bt()


@functools.lru_cache(maxsize=None)
def _cached_trajectories(oracle, mode, table_key, n_paths, n_periods):
    from conftest import load_table
    table = {"none": None, "bundled": load_table(), "big": big_table()}[table_key]
    T = trajectories(oracle, mode, table, n_paths, n_periods)
    T.setflags(write=False)
    return T


def cached_trajectories(oracle, mode, table_key, n_periods, n_paths=N_MAX):
    """Computed once per (mode, table, periods) and shared: never modified."""
    return _cached_trajectories(oracle, mode, table_key, n_paths, n_periods)


@functools.lru_cache(maxsize=None)
def cached_excursions(oracle, mode, table_key, n_periods):
    """The restatement on N_MAX paths at levels(n_periods); computed once, shared, read-only."""
    out = excursions(cached_trajectories(oracle, mode, table_key, n_periods), *levels(n_periods))
    for a in out.values():
        a.setflags(write=False)
    return out
