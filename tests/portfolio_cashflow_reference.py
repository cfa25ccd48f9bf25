"""The portfolio cash-flow contract of include/smmc.h (smmc_engine_simulate_portfolio_cashflow) restated with numpy float32
over the multipliers of tests/portfolio_reference.py (same seed, FIRST_PATH = 2^32 - 100, tables and Gaussian setups):
the reference of tests/test_portfolio_cashflow_cpu.py and tests/test_portfolio_cashflow_gpu.py.

Every operation is one numpy binary32 operation (numpy never fuses); the value is the left-to-right binary32 sum of the
holdings; a depleted path is kept where it is by a mask (np.where on `alive`), never by the arithmetic."""
import functools

import numpy as np

import portfolio_reference as pref

f32 = np.float32
SEED, FIRST_PATH, CAPITAL = pref.SEED, pref.FIRST_PATH, pref.CAPITAL
BINS, LO, HI, BELOW = pref.BINS, pref.LO, pref.HI, pref.BELOW
WEIGHTS, WEIGHTS_WITH_ZERO = pref.WEIGHTS, pref.WEIGHTS_WITH_ZERO
multipliers, asset_table, gauss_setup, factor_of = pref.multipliers, pref.asset_table, pref.gauss_setup, pref.factor_of
FLOOR = 0.01
# what runs on the device (tests/test_portfolio_cashflow_gpu.py); tests/test_portfolio_cashflow_cpu.py checks the schedules
SHAPES = [("t37", 1), ("t37", 2), ("t37", 3), ("t37", 4), ("t2500", 2), ("gauss", 1), ("gauss", 2), ("gauss", 3), ("gauss", 4)]
REBALANCE = [0, 1, 5, 12]
SCHEDULES = ["amount", "fraction", "varying", "floor"]
ZERO_WEIGHT = ("t37", 3)  # run once more with WEIGHTS_WITH_ZERO


def simulate(a, weights, rebalance_every, amount=0.0, fraction=0.0, floor=0.0, amounts=None, fractions=None, capital=CAPITAL,
             columns=False):
    """a [n, P, K] multipliers -> dict of final [n], holdings [K, n], paid [n], ruin_period [n] (uint32), depleted_at
    [P + 1] (uint64); amounts / fractions: [P] arrays that take the place of the scalars, as in smmc_cashflow.
    columns=True adds values [n, P + 1]: v after every period (column 0: the sum of the initial holdings) and
    live_negative [n]: whether a path held a negative holding while live."""
    a = np.asarray(a, dtype=f32)
    n, P, K = a.shape
    w_k = np.asarray(weights, dtype=f32)
    assert w_k.size == K
    R = int(rebalance_every)
    am = np.broadcast_to(np.asarray(amount if amounts is None else amounts, f32), (P,))
    fr = np.broadcast_to(np.asarray(fraction if fractions is None else fractions, f32), (P,))
    floor = f32(floor)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        h = [np.full(n, f32(capital) * w_k[k], dtype=f32) for k in range(K)]
        v = pref.value(h)
        paid = np.zeros(n, f32)
        ruin = np.zeros(n, np.uint32)
        alive = np.ones(n, bool)
        values = np.empty((n, P + 1), f32)
        values[:, 0] = v
        negative = np.zeros(n, bool)
        for t in range(1, P + 1):
            hc = [(h[k] * a[:, t - 1, k]) / f32(100.0) for k in range(K)]
            g = pref.value(hc)
            w = am[t - 1] + g * fr[t - 1]            # the product is rounded, then the sum
            vn = g - w
            ok = alive & (vn > floor)                # False for NaN
            dies = alive & ~ok
            if R and t % R == 0 and t != P:
                hn = [vn * w_k[k] for k in range(K)]
            else:
                hn = [hc[k] - w * w_k[k] for k in range(K)]
            paid = np.where(ok, paid + w, np.where(dies, paid + np.fmax(g, zero), paid)).astype(f32)
            h = [np.where(ok, hn[k], np.where(dies, zero, h[k])).astype(f32) for k in range(K)]
            v = np.where(ok, vn, np.where(dies, zero, v)).astype(f32)
            ruin[dies] = t
            alive = ok
            values[:, t] = v
            for k in range(K):
                negative |= alive & (h[k] < 0)
    assert all(x.dtype == f32 for x in h) and v.dtype == f32 and paid.dtype == f32
    out = {"final": v, "holdings": np.stack(h), "paid": paid, "ruin_period": ruin,
           "depleted_at": np.bincount(ruin, minlength=P + 1).astype(np.uint64)}
    if columns:
        out["values"], out["live_negative"] = values, negative
    return out


def longest(shape):
    return 38 if shape == "gauss" else 41


def periods(shape):
    """Block boundaries (a Philox block yields eight table rows or four normals) and the partial block."""
    return [1, 7, 8, 9, longest(shape)]


def n_paths(shape):
    """64 kW 2 + 37 with kW = 4 (table) or 8 (Gaussian) waves per workgroup: whole chunks, a ragged one, inactive lanes."""
    return 64 * (8 if shape == "gauss" else 4) * 2 + 37


@functools.lru_cache(maxsize=None)
def _scale(oracle, shape, K, weights):
    """(the constant amount that exhausts the MEDIAN path of the longest run exactly at its end, the median final value
    of that run with 3 % taken out every period): what the schedules below are sized by.  From the zero-flow run: with
    the median growth m = (1 + r)^P a level withdrawal A leaves capital m - A ((1 + r)^P - 1) / r."""
    P = longest(shape)
    a = multipliers(oracle, shape, K, n_paths(shape), P)
    m = float(np.median(simulate(a, weights, 0)["final"])) / CAPITAL
    r = m ** (1.0 / P) - 1.0
    level = CAPITAL * m * r / (m - 1.0)
    return float(f32(level)), float(np.median(simulate(a, weights, 0, fraction=0.03)["final"]))


def schedules(oracle, shape, K, weights):
    """name -> (keyword arguments of simulate / Engine.simulate_portfolio_cashflow) of the schedules run on the device,
    sized for the longest P of the shape and for the portfolio's own median growth, so that each depletes a good part
    of the paths but not all: tests/test_portfolio_cashflow_cpu.py asserts between 10 % and 90 % at the longest P, on
    this reference alone.  The arrays hold longest(shape) entries; a run of P periods takes the first P."""
    P = longest(shape)
    level, median_after_3_percent = _scale(oracle, str(shape), int(K), tuple(float(x) for x in weights))
    ramp = np.concatenate([np.full(10, -20.0), np.linspace(1.1, 2.0, P - 10) * level]).astype(f32)  # contributions, then withdrawals
    frac = np.concatenate([np.zeros(10), np.full(P - 10, 0.004)]).astype(f32)
    return {
        "amount": dict(amount=level),
        "fraction": dict(fraction=0.03, floor=float(f32(median_after_3_percent))),
        "varying": dict(amounts=ramp, fractions=frac),
        "floor": dict(amount=float(f32(0.95 * level)), fraction=0.001, floor=FLOOR),
    }


def cut(schedule, P):
    """The schedule's keyword arguments for a run of P periods."""
    return {k: (np.ascontiguousarray(v[:P]) if isinstance(v, np.ndarray) else v) for k, v in schedule.items()}


@functools.lru_cache(maxsize=None)
def _reference(oracle, shape, K, weights, R, name, P):
    a = multipliers(oracle, shape, K, n_paths(shape), longest(shape))
    out = simulate(a[:, :P], weights, R, **cut(schedules(oracle, shape, K, weights)[name], P))
    for x in out.values():
        x.setflags(write=False)
    return out


def reference(oracle, shape, K, weights, R, name, P):
    """simulate() of the named schedule on the module's paths: computed once per request and shared, never modified."""
    return _reference(oracle, str(shape), int(K), tuple(float(x) for x in weights), int(R), str(name), int(P))
