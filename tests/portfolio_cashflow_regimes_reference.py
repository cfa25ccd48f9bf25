"""The regime-switching plan of include/smmc.h (smmc_engine_simulate_portfolio_cashflow_regimes) restated as a composition
of restatements that exist:

    s = regimes_reference.states(...)                                      [n, P] the regime of every period
    z = portfolio_reference.standard_normals(...)                          [n, P, K]
    a = where(s, mix(z, means[1], factor[1]), mix(z, means[0], factor[0]))  the SELECT: all that is new here

and the recurrence is tests/portfolio_cashflow_reference.py's simulate() on those multipliers.  Nothing of the two parent
contracts is written a second time.  The reference of tests/test_portfolio_cashflow_regimes_cpu.py and
tests/test_portfolio_cashflow_regimes_gpu.py.

The schedules are sized per (K, probabilities) on this reference alone: the constant amount that depletes half the
buy-and-hold paths at the longest P, found by bisection; tests/test_portfolio_cashflow_regimes_cpu.py asserts that each
schedule depletes between 10 % and 90 % of the paths at the longest P for every R that runs on the device."""
import functools

import numpy as np

import portfolio_cashflow_reference as pcref
import portfolio_reference as pref
import regimes_reference as rref

f32 = np.float32
SEED, CAPITAL = pref.SEED, pref.CAPITAL
FIRST_PATH = (1 << 32) + 0x1234567       # above 2^32: the high word of every id is not 0
BINS, LO, HI, BELOW = pref.BINS, pref.LO, pref.HI, pref.BELOW
WEIGHTS, FLOOR = pref.WEIGHTS, pcref.FLOOR
GROUP = 512                              # wave_walk_group_paths(SMMC_MODE_GAUSSIAN): 8 waves of 64
N = 2 * GROUP + 65                       # two workgroups' worth and a partial last wave
LONGEST = 37
# every remainder against the 4-draw block and the 8-period field block (6 and 10 for the remainders 2 and 6, which the
# other eleven leave out)
PERIODS = [1, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 17, LONGEST]
REBALANCE = [0, 1, 4, 12, "P"]           # "P": rebalance_every = n_periods, which never rebalances
ONE = rref.ONE
# (leave_q16, start1_q16): a flip at every period; mean sojourns of 40 and 8 periods; regime 0 and regime 1 never left;
# regime 0 left at once and regime 1 never; the three starts
PROBS = [((ONE, ONE), 16384), ((1638, 8192), 16384), ((1638, 8192), 0), ((21845, 32768), ONE), ((0, 32768), 0), ((32768, 0), ONE),
         ((ONE, 0), 0)]
SCHEDULES = ["amount", "fraction", "varying", "floor"]
FAST_SCHEDULES = ["fast_constant", "fast_contributions"]   # what the divide rule proves safe for the reciprocal form
cut = pcref.cut


def laws(K):
    """(means [2][K], factors [2][K, K]): regime 0 is portfolio_reference.gauss_setup's; regime 1 has lower means, larger
    deviations and every correlation's sign turned, so that a select taken from the wrong regime -- of the shift, of the
    deviation or of an off-diagonal entry -- changes the bits."""
    m0, s0, c0 = pref.gauss_setup(K)
    m1 = [-1.2, -0.4, 0.3, -2.0][:K]
    s1 = [7.0, 2.5, 4.0, 6.5][:K]
    c1 = 2.0 * np.eye(K) - c0
    return (tuple(m0), tuple(m1)), (pref.factor_of(s0, c0), pref.factor_of(s1, c1))


def states(oracle, n, P, prob, seed=SEED, first_path=FIRST_PATH):
    leave, start1 = prob
    return rref.states(oracle, seed, first_path, n, P, leave, start1)


def multipliers_of(oracle, means, factors, n, P, prob, seed=SEED, first_path=FIRST_PATH):
    """[n, P, K] multipliers of any laws, probabilities, seed and first path."""
    K = len(means[0])
    z = pref.standard_normals(oracle, K, seed, first_path, n, P)
    s = states(oracle, n, P, prob, seed, first_path)
    return np.where((s != 0)[:, :, None], pref.mix(z, means[1], factors[1]), pref.mix(z, means[0], factors[0]))


@functools.lru_cache(maxsize=None)
def _multipliers(oracle, K, prob):
    means, factors = laws(K)
    a = multipliers_of(oracle, means, factors, N, LONGEST, prob)
    a.setflags(write=False)
    return a


def multipliers(oracle, K, prob, P=LONGEST):
    """The module's N paths over P <= LONGEST periods: computed once per (K, prob) and shared, never modified.  A run of
    fewer periods is a slice: neither the normals nor the states of period t depend on P."""
    return _multipliers(oracle, int(K), (tuple(prob[0]), int(prob[1])))[:, :P]


def rebalance(R, P):
    return int(P) if R == "P" else int(R)


def _depleted(oracle, K, prob, kw, R):
    return float((pcref.simulate(multipliers(oracle, K, prob), WEIGHTS[K], R, **kw)["ruin_period"] > 0).mean())


@functools.lru_cache(maxsize=None)
def _schedules(oracle, K, prob):
    lo, hi = 0.0, CAPITAL  # the constant amount that depletes half the buy-and-hold paths: a condition on the inputs
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _depleted(oracle, K, prob, dict(amount=mid), 0) < 0.5 else (lo, mid)
    level = float(f32(hi))
    P = LONGEST
    after = float(np.median(pcref.simulate(multipliers(oracle, K, prob), WEIGHTS[K], 0, fraction=0.03)["final"]))
    ramp = np.concatenate([np.full(10, -20.0), np.linspace(1.1, 2.0, P - 10) * level]).astype(f32)  # contributions, then withdrawals
    frac = np.concatenate([np.zeros(10), np.full(P - 10, 0.004)]).astype(f32)
    contributions = np.linspace(-30.0, -1.0, P).astype(f32)
    for v in (ramp, frac, contributions):
        v.setflags(write=False)
    return {"amount": dict(amount=level),
            "fraction": dict(fraction=0.03, floor=float(f32(after))),
            "varying": dict(amounts=ramp, fractions=frac),
            "floor": dict(amount=float(f32(0.95 * level)), fraction=0.001, floor=FLOOR),
            "fast_constant": dict(amount=level, floor=FLOOR),
            "fast_contributions": dict(amounts=contributions)}


def schedules(oracle, K, prob):
    """name -> keyword arguments of simulate / simulate_portfolio_cashflow_regimes; arrays hold LONGEST entries, a run of P
    periods takes the first P (cut)."""
    return _schedules(oracle, int(K), (tuple(prob[0]), int(prob[1])))


@functools.lru_cache(maxsize=None)
def _reference(oracle, K, prob, R, name, P):
    out = pcref.simulate(multipliers(oracle, K, prob, P), WEIGHTS[K], R, **cut(schedules(oracle, K, prob)[name], P))
    for x in out.values():
        x.setflags(write=False)
    return out


def reference(oracle, K, prob, R, name, P):
    """simulate() of the named schedule on the module's paths: computed once per request and shared, never modified."""
    return _reference(oracle, int(K), (tuple(prob[0]), int(prob[1])), rebalance(R, P), str(name), int(P))


def device_cases(K):
    """The sparse, covering product run on the device for K assets: every (probabilities, P) pair, with R, the schedule
    and the forced IEEE divide cycling so that every (P, R), (schedule, forced) and (probabilities, schedule) pair occurs
    over the four K.  Yields (prob, P, R, schedule name, forced)."""
    names = SCHEDULES + FAST_SCHEDULES
    i = K
    for a, prob in enumerate(PROBS):
        for b, P in enumerate(PERIODS):
            name = names[i % len(names)]
            yield prob, P, REBALANCE[(a + b + K) % len(REBALANCE)], name, (i // len(names)) % 2 == 1
            i += 1
