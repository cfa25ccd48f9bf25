"""The stationary-bootstrap plan of include/smmc.h (smmc_engine_simulate_portfolio_cashflow_stationary) restated as a
composition of two restatements that exist: the rows are tests/stationary_reference.py's indices over a table of n_rows,

    i = indices_bulk(oracle, a column of n_rows entries, seed, first_path, n, P, q)
    a[:, t, :] = (100.0f + table)[i[:, t]]                                   t = 0 .. P - 1

and the recurrence is tests/portfolio_cashflow_reference.py's simulate() on those multipliers.  Nothing of the contract is
written a second time here.  The reference of tests/test_portfolio_cashflow_stationary_cpu.py and
tests/test_portfolio_cashflow_stationary_gpu.py; seed, first path (the ids cross 2^32), capital, histogram, tables, weights
and the four schedule forms are the block plan's (tests/portfolio_cashflow_blocks_reference.py).

The schedules start from the block plan's at L = 1 -- sized on independent rows, which is q = 65536 -- and are resized by
that module's procedure (the factor on what a schedule takes out that depletes half the buy-and-hold paths, by bisection)
where the stationary paths of a (table, K, weights, q) leave the band: tests/test_portfolio_cashflow_stationary_cpu.py
asserts that each depletes between 10 % and 90 % of the paths at the longest P.  The table of ONE row is exempt, as there:
all its paths are the same path."""
import functools

import numpy as np

import portfolio_cashflow_blocks_reference as B
import portfolio_cashflow_reference as pcref
import stationary_reference as sref

f32 = np.float32
SEED, FIRST_PATH, CAPITAL = B.SEED, B.FIRST_PATH, B.CAPITAL
BINS, LO, HI, BELOW = B.BINS, B.LO, B.HI, B.BELOW
WEIGHTS, WEIGHTS_WITH_ZERO, FLOOR = B.WEIGHTS, B.WEIGHTS_WITH_ZERO, B.FLOOR
N = B.N                       # 549: whole chunks, a ragged one, inactive lanes
LONGEST = 41
PERIODS = [1, 7, 8, 9, 16, LONGEST]
RENEW = [0, 1, 5461, 21845, 32768, 65535, sref.ONE]   # one run, nearly one, mean runs of 12, 3, 2, nearly and exactly independent rows
REBALANCE = [0, 1, 5, 12]
SCHEDULES = B.SCHEDULES
TABLES = B.TABLES             # 37 x K = 1 .. 4 (dense), 2500 x 2 (four-draw), 5 x 2 (fewer rows than a segment), 1 x 1
FOUR_DRAW_ONCE = [(2500, 1), (2500, 3), (2500, 4)]    # the four-draw table with the other K: one case each
ZERO_WEIGHT = B.ZERO_WEIGHT   # run once more with WEIGHTS_WITH_ZERO
asset_table = B.asset_table
cut = pcref.cut


def rows(oracle, T, n, P, q, seed=SEED, first_path=FIRST_PATH):
    """[n, P] row of every period: stationary_reference.indices_bulk over a table of T entries (their values play no part)."""
    return sref.indices_bulk(oracle, np.zeros(T, f32), seed, first_path, n, P, q)


def multipliers_of(oracle, table, n, P, q, seed=SEED, first_path=FIRST_PATH):
    """[n, P, K] multipliers of any table [T, K], seed and first path."""
    table = np.asarray(table, dtype=f32)
    return (f32(100.0) + table)[rows(oracle, table.shape[0], n, P, q, seed, first_path)]


@functools.lru_cache(maxsize=None)
def _multipliers(oracle, T, K, q):
    a = multipliers_of(oracle, asset_table(T, K), N, LONGEST, q)
    a.setflags(write=False)
    return a


def multipliers(oracle, T, K, q, P=LONGEST):
    """The module's N paths over P <= LONGEST periods: computed once per (T, K, q) and shared, never modified.  A run of
    fewer periods is a slice: the row of period t does not depend on P."""
    return _multipliers(oracle, int(T), int(K), int(q))[:, :P]


def _depleted(oracle, T, K, weights, q, kw, R):
    return float((pcref.simulate(multipliers(oracle, T, K, q), weights, R, **kw)["ruin_period"] > 0).mean())


@functools.lru_cache(maxsize=None)
def _schedules(oracle, T, K, weights, q):
    out = {}
    for name, kw in B.schedules(oracle, T, K, weights, 1).items():
        if T > 1 and not all(0.10 <= _depleted(oracle, T, K, weights, q, kw, R) <= 0.90 for R in REBALANCE):
            lo, hi = 0.0, 8.0  # the block plan's resizing, on these paths; a condition on the inputs, found on the reference alone
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if _depleted(oracle, T, K, weights, q, B._resized(kw, mid), 0) < 0.5 else (lo, mid)
            kw = B._resized(kw, hi)
        for v in kw.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[name] = kw
    return out


def schedules(oracle, T, K, weights, q):
    """name -> keyword arguments of simulate / simulate_portfolio_cashflow_stationary; arrays hold LONGEST entries, a run
    of P periods takes the first P (cut)."""
    return _schedules(oracle, int(T), int(K), tuple(float(x) for x in weights), int(q))


def fast_schedules(oracle, T, K, weights, q):
    """Two requests the parent's divide rule proves safe for the reciprocal-multiply form, one per schedule form of the
    kernel: a constant withdrawal with a floor above 0, and arrays of contributions only (which deplete nothing)."""
    level = schedules(oracle, T, K, weights, q)["amount"]["amount"]
    return {"constant": dict(amount=level, floor=FLOOR),
            "contributions": dict(amounts=np.linspace(-30.0, -1.0, LONGEST).astype(f32))}


@functools.lru_cache(maxsize=None)
def _reference(oracle, T, K, weights, R, name, P, q):
    out = pcref.simulate(multipliers(oracle, T, K, q, P), weights, R, **cut(schedules(oracle, T, K, weights, q)[name], P))
    for x in out.values():
        x.setflags(write=False)
    return out


def reference(oracle, T, K, weights, R, name, P, q):
    """simulate() of the named schedule on the module's paths: computed once per request and shared, never modified."""
    return _reference(oracle, int(T), int(K), tuple(float(x) for x in weights), int(R), str(name), int(P), int(q))


def device_cases(T):
    """The sparse, covering product run on the device for a table: every (q, P) pair with every R, the schedule cycling so
    that every (q, schedule), (P, schedule) and (R, schedule) pair occurs."""
    i = 0
    for q in RENEW:
        for P in PERIODS:
            for r, R in enumerate(REBALANCE):
                yield q, P, R, SCHEDULES[(i + r) % len(SCHEDULES)]
            i += 1
