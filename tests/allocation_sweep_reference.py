"""The allocation-sweep contract of include/smmc.h (smmc_engine_simulate_allocation_sweep) restated: scenario s of a
sweep is tests/portfolio_cashflow_reference.py's simulate(a, weights[s], R[s], amount[s], fraction[s], floor[s]) on the
multipliers of tests/portfolio_reference.py.  This module states no arithmetic of its own; what it adds are the scenario
sets that run on the device (tests/test_allocation_sweep_gpu.py), sized here and checked on the restatement alone in
tests/test_allocation_sweep_cpu.py.

A scenario is the tuple (weights, rebalance_every, amount, fraction, floor).  The amounts are multiples of `level`, the
constant amount that exhausts the MEDIAN path of the case's own zero-flow run exactly at its end (the sizing of
portfolio_cashflow_reference.schedules, from the case's capital and growth, for the case's own P): amount 0 depletes no
path, amount = level about half of them."""
import functools

import numpy as np

import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

f32 = np.float32
SEED, FIRST_PATH, CAPITAL = pref.SEED, pref.FIRST_PATH, pref.CAPITAL
BINS, LO, HI, BELOW = pref.BINS, pref.LO, pref.HI, pref.BELOW
FLOOR = pcref.FLOOR
gauss_setup, factor_of, asset_table = pref.gauss_setup, pref.factor_of, pref.asset_table
N_MAX = 2 * 4099 + 1
PATHS = [1, 255, 4099, N_MAX]  # one path; a partial wave; a ragged last chunk; more than one walk
SHAPES = ["t37", "t2500", "gauss"]

# eight allocations per K; K = 1 has one: its scenarios differ in R, amount and floor only
WEIGHT_SETS = {
    1: [(1.0,)] * 8,
    2: [(0.6, 0.4), (1.0, 0.0), (0.8, 0.2), (0.4, 0.6), (0.2, 0.8), (0.0, 1.0), (0.5, 0.5), (0.7, 0.3)],
    3: [(0.5, 0.3, 0.2), (1.0, 0.0, 0.0), (0.2, 0.3, 0.5), (0.4, 0.4, 0.2), (0.1, 0.1, 0.8), (0.5, 0.0, 0.5), (0.3, 0.3, 0.4),
        (0.6, 0.2, 0.2)],
    4: [(0.4, 0.3, 0.2, 0.1), (1.0, 0.0, 0.0, 0.0), (0.1, 0.2, 0.3, 0.4), (0.25, 0.25, 0.25, 0.25), (0.7, 0.1, 0.1, 0.1),
        (0.25, 0.5, 0.0, 0.25), (0.1, 0.1, 0.1, 0.7), (0.3, 0.2, 0.3, 0.2)],
}
REBALANCE = (12, 0, 1, 5, 12, 0, 5, 1)
MULTIPLES = (0.0, 1.0, 0.6, 1.3, 0.85, 2.5, 1.1, 0.3)  # of `level`; scenario 0 takes nothing out, scenario 1 the level


def multipliers(oracle, shape, K, n, P):
    """[n, P, K] multipliers of the module's paths (portfolio_reference.multipliers: cached per request, read-only)."""
    return pref.multipliers(oracle, shape, K, n, P)


def simulate(a, scenarios):
    """One dict of portfolio_cashflow_reference.simulate per scenario."""
    return [pcref.simulate(a, w, R, amount=am, fraction=fr, floor=fl) for w, R, am, fr, fl in scenarios]


@functools.lru_cache(maxsize=None)
def level(oracle, shape, K, P, n=2000):
    """The constant amount that exhausts the median path of scenario 0's allocation at the end of P periods: with the
    median growth m = (1 + r)^P of the zero-flow run a level withdrawal A leaves capital m - A ((1 + r)^P - 1) / r."""
    a = draws(oracle, shape, K, P)[:n]
    m = float(np.median(pcref.simulate(a, WEIGHT_SETS[K][0], 0)["final"])) / CAPITAL
    if abs(m - 1.0) < 1e-6:
        return float(f32(CAPITAL / P))
    r = m ** (1.0 / P) - 1.0
    return float(f32(CAPITAL * m * r / (m - 1.0)))


def draws(oracle, shape, K, P):
    """The module's N_MAX paths for P periods: P <= 9 slices a 9-period draw, P <= 360 the 360-period one (the draws do not
    depend on P); the 1000-period cases run 255 paths."""
    if P <= 360:
        return multipliers(oracle, shape, K, N_MAX, 9 if P <= 9 else 360)[:, :P]
    return multipliers(oracle, shape, K, 255, P)


def uniform_set(oracle, shape, K, P, S):
    """S scenarios that differ in weights, R and amount (fraction 0, floor FLOOR): the first S of the eight; a single
    scenario is scenario 1, the level amount."""
    lv = level(oracle, shape, K, P)
    eight = [(WEIGHT_SETS[K][i], REBALANCE[i], float(f32(MULTIPLES[i] * lv)), 0.0, FLOOR) for i in range(8)]
    return eight[1:2] if S == 1 else eight[:S]


def mixed_set(oracle, shape, K, P):
    """Eight scenarios that differ in weights, in R (0, 1, 5, 12), in amount and fraction, and in floor; scenario 5's
    allocation has a weight of exactly 0 (K >= 2)."""
    lv, W = level(oracle, shape, K, P), WEIGHT_SETS[K]
    return [(W[0], 12, lv, 0.0, FLOOR),                         # the level amount
            (W[1], 0, 0.0, 0.0, 0.0),                           # nothing out, floor 0: depletes no path
            (W[2], 1, float(f32(0.5 * lv)), 0.002, FLOOR),      # amount and fraction
            (W[3], 5, 0.0, 0.004, FLOOR),                       # fraction only
            (W[4], 12, lv, 0.0, 300.0),                         # scenario 0's flow, another allocation and floor
            (W[5], 5, float(f32(1.2 * lv)), 0.0, FLOOR),        # the zero weight
            (W[6], 0, float(f32(-0.2 * lv)), 0.0, FLOOR),       # a contribution, buy and hold
            (W[7], 12, lv, 0.0, FLOOR)]                         # scenario 0's schedule on other weights


MIXED_CASES = [("t37", 3), ("t2500", 2), ("gauss", 4)]
# (shape, K, P, S, n): every shape meets P in {7, 360} with S in {1, 3, 4, 5, 8}; K and n walk round
PARITY_CASES = [(shape, 1 + (i + 2 * j + k) % 4, P, S, PATHS[(i + j + 3 * k) % 4])
                for i, shape in enumerate(SHAPES) for j, P in enumerate((7, 360)) for k, S in enumerate((1, 3, 4, 5, 8))]
LONG_CASES = [("t37", 3, 1000, 5, 255), ("gauss", 2, 1000, 5, 255)]  # without d_stats 5 x 1001 counters fit


def device_sets(oracle):
    """Every (tag, shape, K, P, scenarios) that tests/test_allocation_sweep_gpu.py runs with more than one scenario,
    for the checks of tests/test_allocation_sweep_cpu.py."""
    for shape, K, P, S, n in PARITY_CASES + LONG_CASES:
        if S > 1:
            yield ("uniform", shape, K, P, S), shape, K, P, uniform_set(oracle, shape, K, P, S)
    for shape, K in MIXED_CASES:
        yield ("mixed", shape, K), shape, K, 360, mixed_set(oracle, shape, K, 360)


@functools.lru_cache(maxsize=None)
def _reference(oracle, shape, K, P, scenario):
    out = pcref.simulate(draws(oracle, shape, K, P), *scenario[:2], amount=scenario[2], fraction=scenario[3], floor=scenario[4])
    for x in out.values():
        x.setflags(write=False)
    return out


def reference(oracle, shape, K, P, scenario):
    """The restatement of one scenario on the module's paths (N_MAX of them, 255 for P > 360): computed once per request,
    shared, never modified.  The first n paths of it are a run of n paths."""
    w, R, am, fr, fl = scenario
    return _reference(oracle, str(shape), int(K), int(P), (tuple(float(x) for x in w), int(R), float(am), float(fr), float(fl)))


def cut(out, n):
    """The first n paths of a reference: final, paid, ruin_period [n], holdings [K, n], depleted_at recounted."""
    ruin = out["ruin_period"][:n]
    return {"final": out["final"][:n], "paid": out["paid"][:n], "ruin_period": ruin, "holdings": out["holdings"][:, :n],
            "depleted_at": np.bincount(ruin, minlength=out["depleted_at"].size).astype(np.uint64)}
