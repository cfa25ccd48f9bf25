"""The block-bootstrap plan of include/smmc.h (smmc_engine_simulate_portfolio_cashflow_blocks) restated as a composition of
two restatements that exist: the rows are tests/portfolio_reference.py's table stream read as block starts,

    s = row_indices(oracle, n_rows, seed, first_path, n, ceil(P / L))
    a[:, t, :] = (100.0f + table)[(s[:, t // L] + t % L) % n_rows]          t = 0 .. P - 1

and the recurrence is tests/portfolio_cashflow_reference.py's simulate() on those multipliers.  The reference of
tests/test_portfolio_cashflow_blocks_cpu.py and tests/test_portfolio_cashflow_blocks_gpu.py; seed, first path (the ids
cross 2^32), capital and histogram are the parent's.

The schedules are sized by the parent's procedure (portfolio_cashflow_reference._scale and schedules) applied to the
BLOCK paths' own median growth, per (table, K, weights, L), and resized where that misses (_schedules):
tests/test_portfolio_cashflow_blocks_cpu.py asserts that each depletes between 10 % and 90 % of the paths at the longest P.
The table of ONE row is exempt and says why: all its paths are the same path, so any schedule depletes none or all of them."""
import functools

import numpy as np

import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

f32 = np.float32
SEED, FIRST_PATH, CAPITAL = pcref.SEED, pcref.FIRST_PATH, pcref.CAPITAL
BINS, LO, HI, BELOW = pcref.BINS, pcref.LO, pcref.HI, pcref.BELOW
WEIGHTS, WEIGHTS_WITH_ZERO = pcref.WEIGHTS, pcref.WEIGHTS_WITH_ZERO
FLOOR = pcref.FLOOR
N = 64 * 4 * 2 + 37           # whole chunks, a ragged one, inactive lanes
LONGEST = 41
PERIODS = [1, 7, 8, 9, LONGEST]
BLOCK_LENS = [1, 3, 8, 9, 12, 40, 64]   # tails of 1 (9) and 4 (12), L > T = 37 (40, 64), L > P (64)
REBALANCE = [0, 1, 5, 12]
SCHEDULES = pcref.SCHEDULES
# what runs on the device: (rows, assets).  37 rows: eight starts per Philox block; 2500: four; 5: fewer rows than a
# segment; 1: the staged extension is seven copies of the only row
TABLES = [(37, 1), (37, 2), (37, 3), (37, 4), (2500, 2), (5, 2), (1, 1)]
ZERO_WEIGHT = (37, 3)         # run once more with WEIGHTS_WITH_ZERO
# L = 12 with R = 12 (every rebalance on a block's boundary) and L = 5 with R = 12 (inside a block, and on one at t = 60 > P)
REBALANCE_EDGES = [(12, 12), (5, 12)]


def asset_table(T, K):
    return pref.asset_table(T, K)


def starts(oracle, T, n, n_blocks, seed=SEED, first_path=FIRST_PATH):
    """[n, n_blocks] rows at which the blocks begin: the parent's rows over n_blocks periods."""
    return pref.row_indices(oracle, T, seed, first_path, n, n_blocks)


def rows(oracle, T, n, P, L, seed=SEED, first_path=FIRST_PATH):
    """[n, P] row of every period."""
    s = starts(oracle, T, n, -(-P // L), seed, first_path)
    t = np.arange(P, dtype=np.int64)
    return (s[:, t // L] + (t % L)[None, :]) % T


def multipliers_of(oracle, table, n, P, L, seed=SEED, first_path=FIRST_PATH):
    """[n, P, K] multipliers of any table [T, K], seed and first path."""
    table = np.asarray(table, dtype=f32)
    return (f32(100.0) + table)[rows(oracle, table.shape[0], n, P, L, seed, first_path)]


@functools.lru_cache(maxsize=None)
def _multipliers(oracle, T, K, L):
    a = multipliers_of(oracle, asset_table(T, K), N, LONGEST, L)
    a.setflags(write=False)
    return a


def multipliers(oracle, T, K, L, P=LONGEST):
    """The module's N paths over P <= LONGEST periods: computed once per (T, K, L) and shared, never modified.  A run of
    fewer periods is a slice: block b's start does not depend on P."""
    return _multipliers(oracle, int(T), int(K), int(L))[:, :P]


@functools.lru_cache(maxsize=None)
def _scale(oracle, T, K, weights, L):
    """portfolio_cashflow_reference._scale on the block paths: the level amount that exhausts the median path at the end of
    the longest run, and the median final value with 3 % taken out every period."""
    a = multipliers(oracle, T, K, L)
    m = float(np.median(pcref.simulate(a, weights, 0)["final"])) / CAPITAL
    r = m ** (1.0 / LONGEST) - 1.0
    level = CAPITAL * m * r / (m - 1.0)
    return float(f32(level)), float(np.median(pcref.simulate(a, weights, 0, fraction=0.03)["final"]))


def _base_schedules(oracle, T, K, weights, L):
    """portfolio_cashflow_reference.schedules with the block paths' scale."""
    P = LONGEST
    level, median_after_3_percent = _scale(oracle, T, K, weights, L)
    ramp = np.concatenate([np.full(10, -20.0), np.linspace(1.1, 2.0, P - 10) * level]).astype(f32)
    frac = np.concatenate([np.zeros(10), np.full(P - 10, 0.004)]).astype(f32)
    return {
        "amount": dict(amount=level),
        "fraction": dict(fraction=0.03, floor=float(f32(median_after_3_percent))),
        "varying": dict(amounts=ramp, fractions=frac),
        "floor": dict(amount=float(f32(0.95 * level)), fraction=0.001, floor=FLOOR),
    }


def _resized(kw, f):
    """The schedule with what it takes out scaled by f: the withdrawals, or (a schedule of fractions alone) the floor."""
    kw = dict(kw)
    if "amounts" in kw:
        kw["amounts"] = np.where(kw["amounts"] > 0, kw["amounts"] * f32(f), kw["amounts"]).astype(f32)
    elif "amount" in kw:
        kw["amount"] = float(f32(kw["amount"] * f))
    else:
        kw["floor"] = float(f32(kw["floor"] * f))
    return kw


def _depleted(oracle, T, K, weights, L, kw, R):
    return float((pcref.simulate(multipliers(oracle, T, K, L), weights, R, **kw)["ruin_period"] > 0).mean())


@functools.lru_cache(maxsize=None)
def _schedules(oracle, T, K, weights, L):
    """A schedule that the parent's sizing leaves outside 10 % .. 90 % of the paths depleted at the longest P for some R
    (long blocks on a short table: every path reads nearly the whole table, the paths differ little, and a ramp sized for
    independent rows takes all of them) is resized here: the factor on what it takes out that depletes half the
    buy-and-hold paths, by bisection.  A condition on the inputs, found on this reference alone."""
    out = {}
    for name, kw in _base_schedules(oracle, T, K, weights, L).items():
        if T > 1 and not all(0.10 <= _depleted(oracle, T, K, weights, L, kw, R) <= 0.90 for R in REBALANCE):
            # the bisection looks at R = 0 alone; that the other R of REBALANCE then lie in the band too is not guaranteed by
            # construction: tests/test_portfolio_cashflow_blocks_cpu.py asserts it for every (table, K, L, schedule, R)
            lo, hi = 0.0, 8.0
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                if _depleted(oracle, T, K, weights, L, _resized(kw, mid), 0) < 0.5:
                    lo = mid
                else:
                    hi = mid
            kw = _resized(kw, hi)
        for v in kw.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[name] = kw
    return out


def schedules(oracle, T, K, weights, L):
    """name -> keyword arguments of simulate / Engine.simulate_portfolio_cashflow_blocks; arrays hold LONGEST entries, a run
    of P periods takes the first P (cut)."""
    return _schedules(oracle, int(T), int(K), tuple(float(x) for x in weights), int(L))


def fast_schedules(oracle, T, K, weights, L):
    """Two requests the parent's divide rule proves safe for the reciprocal-multiply form, one per schedule form of the
    kernel: a constant withdrawal with a floor above 0, and arrays of contributions only (which deplete nothing)."""
    level = schedules(oracle, T, K, weights, L)["amount"]["amount"]
    return {"constant": dict(amount=level, floor=FLOOR),
            "contributions": dict(amounts=np.linspace(-30.0, -1.0, LONGEST).astype(f32))}


cut = pcref.cut


@functools.lru_cache(maxsize=None)
def _reference(oracle, T, K, weights, R, name, P, L):
    out = pcref.simulate(multipliers(oracle, T, K, L, P), weights, R, **cut(schedules(oracle, T, K, weights, L)[name], P))
    for x in out.values():
        x.setflags(write=False)
    return out


def reference(oracle, T, K, weights, R, name, P, L):
    """simulate() of the named schedule on the module's paths: computed once per request and shared, never modified."""
    return _reference(oracle, int(T), int(K), tuple(float(x) for x in weights), int(R), str(name), int(P), int(L))


def device_cases(T):
    """The sparse, covering product run on the device for a table: every (L, P) pair with every R, the schedule cycling so
    that every (L, schedule), (P, schedule) and (R, schedule) pair occurs; then the two named rebalance edges."""
    i = 0
    for L in BLOCK_LENS:
        for P in PERIODS:
            for r, R in enumerate(REBALANCE):
                yield L, P, R, SCHEDULES[(i + r) % len(SCHEDULES)]
            i += 1
    for L, R in REBALANCE_EDGES:
        for name in SCHEDULES:
            yield L, LONGEST, R, name
