"""The real cash-flow contract of include/smmc.h (smmc_engine_simulate_real_cashflow) restated with numpy float32 over the
multipliers of tests/portfolio_reference.py at width K + 1 (same seed, FIRST_PATH = 2^32 - 100 and capital): the
reference of tests/test_real_cashflow_cpu.py and tests/test_real_cashflow_gpu.py.

The joint law has K + 1 series, the last one inflation in percent per period.  Table mode: asset_table(T, K + 1) with its
last column c replaced by 0.25 + 0.1 c -- monthly inflation around 0.25 %, sometimes negative, correlated with the
assets.  Gaussian mode: gauss_setup(K + 1) with the last series' mean and standard deviation set to 0.25 and 0.4.

Every operation is one numpy binary32 operation (numpy never fuses); the value is the left-to-right binary32 sum of the K
holdings; a depleted path is kept where it is by a mask, never by the arithmetic; the index compounds on every path."""
import functools

import numpy as np

import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

f32 = np.float32
SEED, FIRST_PATH, CAPITAL = pref.SEED, pref.FIRST_PATH, pref.CAPITAL
BINS, LO, HI, BELOW = pref.BINS, pref.LO, pref.HI, pref.BELOW
WEIGHTS = pref.WEIGHTS
FLOOR = pcref.FLOOR
INFLATION_MEAN, INFLATION_STD = 0.25, 0.4
# what runs on the device (tests/test_real_cashflow_gpu.py); tests/test_real_cashflow_cpu.py checks the schedules
SHAPES = [("t37", 1), ("t37", 2), ("t37", 3), ("t2500", 2), ("gauss", 1), ("gauss", 2), ("gauss", 3)]
REBALANCE = pcref.REBALANCE
SCHEDULES = pcref.SCHEDULES
longest, periods, n_paths, cut = pcref.longest, pcref.periods, pcref.n_paths, pcref.cut


@functools.lru_cache(maxsize=None)
def _joint_table(T, K):
    t = pref.asset_table(T, K + 1).copy()
    t[:, K] = f32(0.25) + f32(0.1) * t[:, K]
    t.setflags(write=False)
    return t


def joint_table(T, K):
    """[T, K + 1] returns in percent: K assets and the inflation column; computed once, shared, read-only."""
    return _joint_table(int(T), int(K))


def gauss_law(K):
    """(means [K + 1], factor [K + 1, K + 1]) of the Gaussian cases: K assets and inflation, every pairwise entry non-zero."""
    means, stds, corr = pref.gauss_setup(K + 1)
    means, stds = list(means), list(stds)
    means[K], stds[K] = INFLATION_MEAN, INFLATION_STD
    return [float(m) for m in means], pref.factor_of(stds, corr)


@functools.lru_cache(maxsize=None)
def _multipliers(oracle, shape, K, n, P):
    if shape == "gauss":
        means, factor = gauss_law(K)
        a = pref.gauss_multipliers(oracle, means, factor, SEED, FIRST_PATH, n, P)
    else:
        a = pref.table_multipliers(oracle, joint_table(int(shape[1:]), K), SEED, FIRST_PATH, n, P)
    a.setflags(write=False)
    return a


def multipliers(oracle, shape, K, n, P):
    """[n, P, K + 1] multipliers of shape 'gauss' or 't<rows>' at the module's seed and first path: computed once per
    request and shared, never modified."""
    return _multipliers(oracle, str(shape), int(K), int(n), int(P))


def simulate(a, weights, rebalance_every, amount=0.0, fraction=0.0, floor=0.0, amounts=None, fractions=None, capital=CAPITAL,
             columns=False):
    """a [n, P, K + 1] multipliers, weights [K] -> dict of final, final_real, index [n], holdings [K, n], paid [n],
    ruin_period [n] (uint32), depleted_at [P + 1] (uint64); amount / amounts and floor in money of period 0.
    columns=True adds values and indices [n, P + 1]: v and I after every period (column 0: the start)."""
    a = np.asarray(a, dtype=f32)
    n, P, K1 = a.shape
    K = K1 - 1
    w_k = np.asarray(weights, dtype=f32)
    assert w_k.size == K >= 1
    R = int(rebalance_every)
    am = np.broadcast_to(np.asarray(amount if amounts is None else amounts, f32), (P,))
    fr = np.broadcast_to(np.asarray(fraction if fractions is None else fractions, f32), (P,))
    floor = f32(floor)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        h = [np.full(n, f32(capital) * w_k[k], dtype=f32) for k in range(K)]
        index = np.ones(n, f32)
        v = pref.value(h)
        paid = np.zeros(n, f32)
        ruin = np.zeros(n, np.uint32)
        alive = np.ones(n, bool)
        values, indices = np.empty((n, P + 1), f32), np.empty((n, P + 1), f32)
        values[:, 0], indices[:, 0] = v, index
        for t in range(1, P + 1):
            hc = [(h[k] * a[:, t - 1, k]) / f32(100.0) for k in range(K)]
            index = (index * a[:, t - 1, K]) / f32(100.0)      # on every path, depleted or not
            g = pref.value(hc)
            w = am[t - 1] * index + g * fr[t - 1]               # both products are rounded, then the sum
            vn = g - w
            ok = alive & (vn > floor * index)                   # False for NaN
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
            values[:, t], indices[:, t] = v, index
        final_real = v / index                                  # one division per path, after the loop
    assert all(x.dtype == f32 for x in h) and v.dtype == f32 and paid.dtype == f32 and index.dtype == f32 and final_real.dtype == f32
    out = {"final": v, "final_real": final_real, "index": index, "holdings": np.stack(h), "paid": paid, "ruin_period": ruin,
           "depleted_at": np.bincount(ruin, minlength=P + 1).astype(np.uint64)}
    if columns:
        out["values"], out["indices"] = values, indices
    return out


@functools.lru_cache(maxsize=None)
def _scale(oracle, shape, K, weights):
    """(the constant REAL amount that exhausts the median path of the longest run exactly at its end, the median real
    final value of that run with 3 % taken out every period): what the schedules below are sized by, as
    portfolio_cashflow_reference._scale, from the zero-flow run's growth in money of period 0."""
    P = longest(shape)
    a = multipliers(oracle, shape, K, n_paths(shape), P)
    m = float(np.median(simulate(a, weights, 0)["final_real"])) / CAPITAL
    r = m ** (1.0 / P) - 1.0
    level = CAPITAL * m * r / (m - 1.0) if abs(m - 1.0) > 1e-9 else CAPITAL / P
    return float(f32(level)), float(np.median(simulate(a, weights, 0, fraction=0.03)["final_real"]))


def schedules(oracle, shape, K, weights):
    """name -> (keyword arguments of simulate / Engine.simulate_real_cashflow) of the schedules run on the device: the
    parent's four, amounts and floors in money of period 0, sized for the longest P of the shape so that each depletes
    a good part of the paths but not all (tests/test_real_cashflow_cpu.py asserts between 10 % and 90 %, on this
    reference alone).  The arrays hold longest(shape) entries; a run of P periods takes the first P."""
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
