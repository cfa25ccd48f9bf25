"""Regime-switching Gaussian paths (smmc_engine_simulate_regimes, include/smmc.h): a hidden state per path, 0 or 1, that
persists from period to period and leaves regime r with probability leave_q16[r] / 65536 at every period; each regime has
a mean and a deviation of its own (Hamilton's two regimes).  The Gaussian counterpart of what runs of consecutive months
do for the table.

Functions of an Engine, not methods: they go through the engine's binding helpers exactly as simulate_stationary does and
return what it returns.  means=(m0, m1) and stds=(s0, s1) in percent per period; exactly one of mean_durations=(d0, d1),
the mean sojourn in each regime in periods, and leave_q16=(l0, l1) says how long a regime lasts.  start: the probability
that period 0 is in regime 1 (None: the chain's stationary share), or start1_q16 in units of 2^-16.  sim.gauss_mean and
sim.gauss_std are not read."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .engine import PortfolioCashflowResult, SimResult, Stats, _BLOCKS_ROWS, _PFCF_ROWS, _buffers, _records_as_bytes, cholesky_factor

REGIME_Q16_ONE = _lib.REGIME_Q16_ONE


def _leave_q16_of(duration):
    """leave_q16 for a mean sojourn of `duration` periods: round(65536 / duration), refused as renew_q16_of refuses."""
    d = float(duration)
    if not d >= 1.0:
        raise ValueError("a mean duration must be at least 1 period (got %r)" % (duration,))
    q = int(round(REGIME_Q16_ONE / d))
    if q == 0:
        raise ValueError("mean duration %r is beyond the resolution 2^-16 of the probability: pass leave_q16 with a 0 for a regime "
                         "that is never left" % (duration,))
    return q


def _q16(value, name):
    q = int(value)
    if q != value or not 0 <= q <= REGIME_Q16_ONE:
        raise ValueError("%s must be an integer in [0, 65536] (got %r)" % (name, value))
    return q


def _one_of_each(mean_durations, leave_q16, start, start1_q16):
    if (mean_durations is None) == (leave_q16 is None):
        raise ValueError("give exactly one of mean_durations and leave_q16")
    if start is not None and start1_q16 is not None:
        raise ValueError("give at most one of start and start1_q16")


def _probabilities(mean_durations, leave_q16, start, start1_q16):
    """(leave_q16[2], start1_q16) of a request's probability arguments."""
    _one_of_each(mean_durations, leave_q16, start, start1_q16)
    if leave_q16 is None:
        if len(mean_durations) != 2:
            raise ValueError("mean_durations holds two numbers")
        leave = [_leave_q16_of(d) for d in mean_durations]
    else:
        if len(leave_q16) != 2:
            raise ValueError("leave_q16 holds two numbers")
        leave = [_q16(q, "leave_q16") for q in leave_q16]
    if start1_q16 is not None:
        s1 = _q16(start1_q16, "start1_q16")
    elif start is not None:
        p = float(start)
        if not 0.0 <= p <= 1.0:
            raise ValueError("start is a probability (got %r)" % (start,))
        s1 = int(round(p * REGIME_Q16_ONE))
    else:
        if leave[0] + leave[1] == 0:
            raise ValueError("neither regime is ever left, the chain has no stationary share: give start or start1_q16")
        s1 = int(round(REGIME_Q16_ONE * leave[0] / (leave[0] + leave[1])))
    return leave, s1


def make_regimes(means, stds, mean_durations=None, leave_q16=None, start=None, start1_q16=None):
    """The smmc_regimes of a request."""
    _one_of_each(mean_durations, leave_q16, start, start1_q16)  # the order of the refusals: these two, the numbers, the probabilities
    m, s = [float(x) for x in means], [float(x) for x in stds]
    if len(m) != 2 or len(s) != 2:
        raise ValueError("means and stds hold two numbers, regime 0's and regime 1's")
    if not all(math.isfinite(x) for x in m + s) or min(s) < 0.0:
        raise ValueError("means and stds must be finite, stds >= 0 (got %r, %r)" % (means, stds))
    leave, s1 = _probabilities(mean_durations, leave_q16, start, start1_q16)
    rg = _lib.Regimes()
    rg.struct_size = C.sizeof(_lib.Regimes)
    rg.mean[0], rg.mean[1] = m
    rg.std[0], rg.std[1] = s
    rg.leave_q16[0], rg.leave_q16[1] = leave
    rg.start1_q16 = s1
    return rg


def simulate_regimes(eng, sim, means, stds, mean_durations=None, leave_q16=None, start=None, start1_q16=None, want_final=True,
                     want_chunk_stats=False, want_stats=False, out=None):
    """Engine.simulate() under the two-regime law (Gaussian mode, counter stream v3; include/smmc.h states the draw).  Equal
    regimes are simulate_portfolio with one asset, bit for bit.  Returns the same SimResult of device tensors."""
    raw = simulate_regimes_raw(eng, sim, means, stds, mean_durations, leave_q16, start, start1_q16, want_final, want_chunk_stats,
                               want_stats, out)
    res = SimResult()
    res.final, res.chunk_mean, res.chunk_var, res.stats_raw = raw["final"], raw["chunk_mean"], raw["chunk_var"], raw["stats_raw"]
    return res


def simulate_regimes_raw(eng, sim, means, stds, mean_durations=None, leave_q16=None, start=None, start1_q16=None, want_final=True,
                         want_chunk_stats=False, want_stats=False, out=None):
    """Enqueues the call and returns its device tensors without waiting: a dict with final, chunk_mean, chunk_var (float32)
    and stats_raw (uint8, the packed record); None for what was not asked for."""
    rg = make_regimes(means, stds, mean_durations, leave_q16, start, start1_q16)
    res, ptrs = eng._outputs(_BLOCKS_ROWS, None, sim, (want_final, want_chunk_stats, want_chunk_stats, want_stats), host=False,
                             given={"final": out})
    eng._check_out(res["final"], sim)
    eng._run(eng._L.smmc_engine_simulate_regimes, C.byref(sim), C.byref(rg), *ptrs, device=_buffers(_BLOCKS_ROWS, res))
    return res


def simulate_regimes_to_host(eng, sim, means, stds, mean_durations=None, leave_q16=None, start=None, start1_q16=None, out=None,
                             want_stats=False, want_chunk_stats=False, progress=None):
    """Engine.simulate_to_host() with these draws: (final, stats, (means, vars)) in host memory."""
    n = int(sim.n_paths)
    rg = make_regimes(means, stds, mean_durations, leave_q16, start, start1_q16)
    host = out if out is not None else np.empty(n, dtype=np.float32)
    assert host.dtype == np.float32 and host.size >= n and host.flags.c_contiguous
    rec = _lib.Stats()
    hist = np.zeros(max(int(sim.n_bins), 1), dtype=np.uint64)
    nc = (n + _lib.CHUNK - 1) // _lib.CHUNK
    cm = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
    cv = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    # synchronous: returns with both of its streams drained
    eng._run(eng._L.smmc_engine_simulate_regimes_to_host, C.byref(sim), C.byref(rg), vp(host), vp(cm), vp(cv),
             C.byref(progress) if progress is not None else None, C.byref(rec) if want_stats else None, vp(hist) if want_stats else None)
    stats = None
    if want_stats:
        stats = Stats(rec.count, rec.below, rec.underflow, rec.overflow, rec.sum, rec.sumsq, rec.min, rec.max, hist[: int(sim.n_bins)])
    return host, stats, (cm, cv)


def regimes_divide_kind(eng, sim, means, stds, mean_durations=None, leave_q16=None, start=None, start1_q16=None):
    """DIV_FAST / DIV_EXACT / DIV_CHECKED: the divide simulate_regimes uses for this request (results never depend on it)."""
    rg = make_regimes(means, stds, mean_durations, leave_q16, start, start1_q16)
    return eng._kind(eng._L.smmc_engine_regimes_divide_kind(eng._h, C.byref(sim), C.byref(rg)))


# ---- regime-switching plans (smmc_engine_simulate_portfolio_cashflow_regimes) ----------------------------------------

def make_portfolio_regimes(means, factors=None, mean_durations=None, leave_q16=None, start=None, start1_q16=None, stds=None, corrs=None):
    """The smmc_portfolio_regimes of a request: means[r][k] in percent per period and, per regime, either the
    lower-triangular factor L_r (factors[r], K x K) or stds[r] with corrs[r] (through cholesky_factor).  The probability
    arguments are make_regimes'."""
    if (factors is None) == (stds is None and corrs is None):
        raise ValueError("give either factors, or stds with corrs")
    if factors is None and (stds is None or corrs is None):
        raise ValueError("stds and corrs come together")
    m = np.asarray(means, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != 2 or not 1 <= m.shape[1] <= _lib.MAX_ASSETS:
        raise ValueError("means holds two rows, regime 0's and regime 1's, of 1 .. %d assets" % _lib.MAX_ASSETS)
    K = m.shape[1]
    if factors is None:
        if len(stds) != 2 or len(corrs) != 2:
            raise ValueError("stds and corrs hold two entries, regime 0's and regime 1's")
        factors = [cholesky_factor(stds[r], corrs[r]) for r in range(2)]
    if len(factors) != 2:
        raise ValueError("factors holds two matrices, regime 0's and regime 1's")
    L = [np.asarray(f, dtype=np.float32) for f in factors]
    if any(f.shape != (K, K) for f in L):
        raise ValueError("a factor is K x K for the K = %d assets of means" % K)
    if not np.isfinite(m).all() or not all(np.isfinite(f).all() for f in L):
        raise ValueError("means and factors must be finite")
    if any(np.triu(f, 1).any() or (np.diag(f) < 0).any() for f in L):
        raise ValueError("a factor is lower triangular with a diagonal >= 0")
    leave, s1 = _probabilities(mean_durations, leave_q16, start, start1_q16)
    rg = _lib.PortfolioRegimes()
    rg.struct_size = C.sizeof(_lib.PortfolioRegimes)
    rg.leave_q16[0], rg.leave_q16[1] = leave
    rg.start1_q16 = s1
    for r in range(2):
        for k in range(K):
            rg.means[r][k] = float(m[r, k])
            for j in range(k + 1):
                rg.factor[r][k * _lib.MAX_ASSETS + j] = float(L[r][k, j])
    return rg


def simulate_portfolio_cashflow_regimes(eng, sim, weights, means, factors=None, mean_durations=None, leave_q16=None, start=None,
                                        start1_q16=None, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                        fractions=None, stds=None, corrs=None, want_final=True, want_holdings=False, want_paid=False,
                                        want_ruin_period=False, want_stats=False, want_depleted_at=True):
    """Engine.simulate_portfolio_cashflow in Gaussian mode under simulate_regimes' hidden state: a month's multipliers are
    those of the regime the path is in (counter stream v3; include/smmc.h states the composition).  Equal regimes, or a
    regime never left, are simulate_portfolio_cashflow bit for bit.  Returns the same PortfolioCashflowResult, so survival()
    works as there."""
    raw = simulate_portfolio_cashflow_regimes_raw(eng, sim, weights, means, factors, mean_durations, leave_q16, start, start1_q16,
                                                  rebalance_every, amount, fraction, floor, amounts, fractions, stds, corrs, want_final,
                                                  want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at)
    res = PortfolioCashflowResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                                  n_assets=raw["n_assets"], holdings=raw["holdings"])
    return eng._read_back(res, sim, raw, _PFCF_ROWS)


def simulate_portfolio_cashflow_regimes_raw(eng, sim, weights, means, factors=None, mean_durations=None, leave_q16=None, start=None,
                                            start1_q16=None, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                            fractions=None, stds=None, corrs=None, want_final=True, want_holdings=False,
                                            want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=True):
    """Enqueues the call and returns its device tensors without waiting: simulate_portfolio_cashflow_raw's dict."""
    pf = eng.make_portfolio(weights, rebalance_every)
    rg = make_portfolio_regimes(means, factors, mean_durations, leave_q16, start, start1_q16, stds, corrs)
    cf, keep = eng.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
    res, o = eng._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                               host=False)
    eng._run(eng._L.smmc_engine_simulate_portfolio_cashflow_regimes, C.byref(sim), C.byref(pf), C.byref(rg), C.byref(cf), C.byref(o),
             device=_buffers(_PFCF_ROWS, res))
    del keep
    return res


def simulate_portfolio_cashflow_regimes_to_host(eng, sim, weights, means, factors=None, mean_durations=None, leave_q16=None, start=None,
                                                start1_q16=None, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                                fractions=None, stds=None, corrs=None, want_final=True, want_holdings=False,
                                                want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=True):
    """The same through smmc_engine_simulate_portfolio_cashflow_regimes_to_host: a dict of numpy arrays (stats_raw: bytes)."""
    pf = eng.make_portfolio(weights, rebalance_every)
    rg = make_portfolio_regimes(means, factors, mean_durations, leave_q16, start, start1_q16, stds, corrs)
    cf, keep = eng.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
    res, o = eng._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                               host=True)
    eng._run(eng._L.smmc_engine_simulate_portfolio_cashflow_regimes_to_host, C.byref(sim), C.byref(pf), C.byref(rg), C.byref(cf), C.byref(o))
    del keep
    return _records_as_bytes(_PFCF_ROWS, res)


def portfolio_cashflow_regimes_divide_kind(eng, sim, weights, means, factors=None, mean_durations=None, leave_q16=None, start=None,
                                           start1_q16=None, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                           fractions=None, stds=None, corrs=None):
    """_lib.DIV_FAST or DIV_EXACT: the divide simulate_portfolio_cashflow_regimes uses for this request (results never depend on
    it): portfolio_cashflow_divide_kind's rule on the union of the two regimes' bounds."""
    pf = eng.make_portfolio(weights, rebalance_every)
    rg = make_portfolio_regimes(means, factors, mean_durations, leave_q16, start, start1_q16, stds, corrs)
    cf, keep = eng.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)  # keep lives until the return
    return eng._kind(eng._L.smmc_engine_portfolio_cashflow_regimes_divide_kind(eng._h, C.byref(sim), C.byref(pf), C.byref(rg), C.byref(cf)))
