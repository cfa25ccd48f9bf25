"""The cash-flow arithmetic of include/smmc.h (smmc_engine_simulate_cashflow) restated in numpy float32, over the
CPU oracle's per-path returns: the reference of tests/test_cashflow_cpu.py and tests/test_cashflow_gpu.py.

Every operation is one binary32 rounding (numpy float32 arithmetic never fuses).  The oracle's returns r reproduce
the engine's multiplier as 100.0f + r, and total * a / 100 exactly, for a in [50, 200]: the bundled table
(-15.1 .. +14.3 %), the tests' 3001-entry table (+-25 %) and the default Gaussian stay inside that.  Inputs outside
it (tests/feature_matrix.py's wide Gaussian laws and wild tables) take the oracle's multipliers themselves:
multipliers() and simulate_multipliers(); simulate(R, ...) is simulate_multipliers(100.0f + R, ...), and
tests/test_feature_matrix_cpu.py compares the two routes bit for bit on the inputs above."""
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


def multipliers(oracle, mode, table, n_paths, n_periods, first_path=FIRST_PATH, seed=SEED, gauss_mean=0.5, gauss_std=0.83333):
    """[n_paths, n_periods] multipliers a of paths first_path .. (counter stream v3) as the oracle's path loop forms them
    (oracle.multipliers_of_words of the Philox blocks (b, id lo, id hi, mode)): 100.0f + entry in table mode, the drawn
    multiplier itself in Gaussian mode -- exact for any law and any table, which 100.0f + (a - 100.0f) is not."""
    p = oracle.make_params(mode, n_periods, n_paths, seed, first_path=first_path, table=table, gauss_mean=gauss_mean,
                           gauss_std=gauss_std)
    D = int(oracle.lib().orc_draws_per_block(p.mode, p.table_len))
    nb = -(-n_periods // D)
    if nb == 0 or n_paths == 0:
        return np.empty((n_paths, n_periods), dtype=f32)
    ids = np.uint64(first_path) + np.arange(n_paths, dtype=np.uint64)
    ctr = np.empty((n_paths, nb, 4), dtype=np.uint32)
    ctr[:, :, 0] = np.arange(nb, dtype=np.uint32)[None, :]
    ctr[:, :, 1] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[:, :, 2] = (ids >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[:, :, 3] = np.uint32(mode)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    words = oracle.philox4x32_10_bulk(ctr.reshape(-1, 4), key)
    return np.ascontiguousarray(oracle.multipliers_of_words(p, words).reshape(n_paths, nb * D)[:, :n_periods])


def simulate(R, amount=0.0, fraction=0.0, floor=0.0, capital=CAPITAL):
    """(final, paid, ruin_period, depleted_at) for the returns R [n, P]; amount / fraction: scalars or [P] arrays."""
    return simulate_multipliers(f32(100.0) + np.asarray(R, dtype=f32), amount, fraction, floor, capital)


def simulate_multipliers(A, amount=0.0, fraction=0.0, floor=0.0, capital=CAPITAL):
    """simulate() for the multipliers A [n, P] themselves (multipliers() above)."""
    A = np.asarray(A, dtype=f32)
    n, P = A.shape
    am = np.broadcast_to(np.asarray(amount, f32), (P,))
    fr = np.broadcast_to(np.asarray(fraction, f32), (P,))
    floor = f32(floor)
    v = np.full(n, capital, f32)
    paid = np.zeros(n, f32)
    ruin = np.zeros(n, np.uint32)
    alive = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for t in range(P):
            a = A[:, t]
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
