"""The stationary bootstrap (smmc_engine_simulate_stationary, include/smmc.h): table paths that start a new run of
consecutive months with probability p = renew_q16 / 65536 at every period, so that run lengths are geometric with mean
1 / p and no period of a path is a fixed block boundary.

Functions of an Engine, not methods: they go through the engine's binding helpers exactly as Engine.simulate_blocks does
and return what it returns.  Exactly one of mean_block_len and renew_q16 says how long the runs are.

The same draw under a plan (smmc_engine_simulate_portfolio_cashflow_stationary): simulate_portfolio_cashflow_stationary and
its _raw, _to_host and divide_kind forms, which go through the helpers exactly as Engine.simulate_portfolio_cashflow_blocks
does."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import PortfolioCashflowResult, SimResult, Stats, _BLOCKS_ROWS, _PFCF_ROWS, _buffers, _records_as_bytes

RENEW_Q16_ONE = _lib.RENEW_Q16_ONE


def renew_q16_of(mean_block_len):
    """renew_q16 for runs of the given mean length: round(65536 / mean).  A mean below 1 is no run length; one so long
    that the quotient rounds to 0 would silently mean "never renew" and is refused too (renew_q16=0 asks for that)."""
    mean = float(mean_block_len)
    if not mean >= 1.0:
        raise ValueError("mean_block_len must be at least 1 (got %r)" % (mean_block_len,))
    q = int(round(RENEW_Q16_ONE / mean))
    if q == 0:
        raise ValueError("mean_block_len %r is beyond the resolution 2^-16 of the renewal probability: pass renew_q16=0 for one run" %
                         (mean_block_len,))
    return q


def make_stationary(mean_block_len=None, renew_q16=None):
    """The smmc_stationary of a request."""
    if (mean_block_len is None) == (renew_q16 is None):
        raise ValueError("give exactly one of mean_block_len and renew_q16")
    q = renew_q16_of(mean_block_len) if renew_q16 is None else int(renew_q16)
    if not 0 <= q <= RENEW_Q16_ONE:
        raise ValueError("renew_q16 must lie in [0, 65536] (got %r)" % (renew_q16,))
    st = _lib.Stationary()
    st.struct_size, st.renew_q16 = C.sizeof(_lib.Stationary), q
    return st


def simulate_stationary(eng, sim, mean_block_len=None, renew_q16=None, want_final=True, want_chunk_stats=False, want_stats=False,
                        out=None):
    """Engine.simulate() with the stationary bootstrap (table mode, counter stream v3; include/smmc.h states the draw).
    renew_q16 = 65536 is simulate() bit for bit, renew_q16 = 0 simulate_blocks() with one block.  Returns the same
    SimResult of device tensors."""
    raw = simulate_stationary_raw(eng, sim, mean_block_len, renew_q16, want_final, want_chunk_stats, want_stats, out)
    res = SimResult()
    res.final, res.chunk_mean, res.chunk_var, res.stats_raw = raw["final"], raw["chunk_mean"], raw["chunk_var"], raw["stats_raw"]
    return res


def simulate_stationary_raw(eng, sim, mean_block_len=None, renew_q16=None, want_final=True, want_chunk_stats=False, want_stats=False,
                            out=None):
    """Enqueues the call and returns its device tensors without waiting: a dict with final, chunk_mean, chunk_var (float32)
    and stats_raw (uint8, the packed record); None for what was not asked for."""
    st = make_stationary(mean_block_len, renew_q16)
    res, ptrs = eng._outputs(_BLOCKS_ROWS, None, sim, (want_final, want_chunk_stats, want_chunk_stats, want_stats), host=False,
                             given={"final": out})
    eng._check_out(res["final"], sim)
    eng._run(eng._L.smmc_engine_simulate_stationary, C.byref(sim), C.byref(st), *ptrs, device=_buffers(_BLOCKS_ROWS, res))
    return res


def simulate_stationary_to_host(eng, sim, mean_block_len=None, renew_q16=None, out=None, want_stats=False, want_chunk_stats=False,
                                progress=None):
    """Engine.simulate_to_host() with these draws: (final, stats, (means, vars)) in host memory."""
    n = int(sim.n_paths)
    st = make_stationary(mean_block_len, renew_q16)
    host = out if out is not None else np.empty(n, dtype=np.float32)
    assert host.dtype == np.float32 and host.size >= n and host.flags.c_contiguous
    rec = _lib.Stats()
    hist = np.zeros(max(int(sim.n_bins), 1), dtype=np.uint64)
    nc = (n + _lib.CHUNK - 1) // _lib.CHUNK
    cm = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
    cv = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    # synchronous: returns with both of its streams drained
    eng._run(eng._L.smmc_engine_simulate_stationary_to_host, C.byref(sim), C.byref(st), vp(host), vp(cm), vp(cv),
             C.byref(progress) if progress is not None else None, C.byref(rec) if want_stats else None, vp(hist) if want_stats else None)
    stats = None
    if want_stats:
        stats = Stats(rec.count, rec.below, rec.underflow, rec.overflow, rec.sum, rec.sumsq, rec.min, rec.max, hist[: int(sim.n_bins)])
    return host, stats, (cm, cv)


def stationary_divide_kind(eng, sim, mean_block_len=None, renew_q16=None):
    """DIV_FAST / DIV_EXACT / DIV_CHECKED: the divide simulate_stationary uses for this request (results never depend on it)."""
    st = make_stationary(mean_block_len, renew_q16)
    return eng._kind(eng._L.smmc_engine_stationary_divide_kind(eng._h, C.byref(sim), C.byref(st)))


def simulate_portfolio_cashflow_stationary(eng, sim, weights, mean_block_len=None, renew_q16=None, rebalance_every=0, amount=0.0,
                                           fraction=0.0, floor=0.0, amounts=None, fractions=None, want_final=True, want_holdings=False,
                                           want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=True):
    """Engine.simulate_portfolio_cashflow on rows of set_asset_table's table chosen by the stationary bootstrap (table mode,
    counter stream v3; include/smmc.h states the row rule): a path starts a new run where the portfolio's table stream would
    have drawn a single row, with probability renew_q16 / 65536 at every period.  renew_q16 = 65536 is
    simulate_portfolio_cashflow bit for bit, renew_q16 = 0 simulate_portfolio_cashflow_blocks with one block.  Returns the
    same PortfolioCashflowResult, so survival() works as there."""
    raw = simulate_portfolio_cashflow_stationary_raw(eng, sim, weights, mean_block_len, renew_q16, rebalance_every, amount, fraction,
                                                     floor, amounts, fractions, want_final, want_holdings, want_paid, want_ruin_period,
                                                     want_stats, want_depleted_at)
    res = PortfolioCashflowResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                                  n_assets=raw["n_assets"], holdings=raw["holdings"])
    return eng._read_back(res, sim, raw, _PFCF_ROWS)


def simulate_portfolio_cashflow_stationary_raw(eng, sim, weights, mean_block_len=None, renew_q16=None, rebalance_every=0, amount=0.0,
                                               fraction=0.0, floor=0.0, amounts=None, fractions=None, want_final=True,
                                               want_holdings=False, want_paid=False, want_ruin_period=False, want_stats=False,
                                               want_depleted_at=True):
    """Enqueues the call and returns its device tensors without waiting: simulate_portfolio_cashflow_raw's dict."""
    pf = eng.make_portfolio(weights, rebalance_every)
    st = make_stationary(mean_block_len, renew_q16)
    cf, keep = eng.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
    res, o = eng._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                               host=False)
    eng._run(eng._L.smmc_engine_simulate_portfolio_cashflow_stationary, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(st), C.byref(o),
             device=_buffers(_PFCF_ROWS, res))
    del keep
    return res


def simulate_portfolio_cashflow_stationary_to_host(eng, sim, weights, mean_block_len=None, renew_q16=None, rebalance_every=0,
                                                   amount=0.0, fraction=0.0, floor=0.0, amounts=None, fractions=None, want_final=True,
                                                   want_holdings=False, want_paid=False, want_ruin_period=False, want_stats=False,
                                                   want_depleted_at=True):
    """The same through smmc_engine_simulate_portfolio_cashflow_stationary_to_host: a dict of numpy arrays (stats_raw: bytes)."""
    pf = eng.make_portfolio(weights, rebalance_every)
    st = make_stationary(mean_block_len, renew_q16)
    cf, keep = eng.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
    res, o = eng._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                               host=True)
    eng._run(eng._L.smmc_engine_simulate_portfolio_cashflow_stationary_to_host, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(st),
             C.byref(o))
    del keep
    return _records_as_bytes(_PFCF_ROWS, res)


def portfolio_cashflow_stationary_divide_kind(eng, sim, weights, mean_block_len=None, renew_q16=None, rebalance_every=0, amount=0.0,
                                              fraction=0.0, floor=0.0, amounts=None, fractions=None):
    """_lib.DIV_FAST or DIV_EXACT: what portfolio_cashflow_divide_kind says of the same plan (results never depend on it)."""
    pf = eng.make_portfolio(weights, rebalance_every)
    st = make_stationary(mean_block_len, renew_q16)
    cf, keep = eng.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)  # keep lives until the return
    return eng._kind(eng._L.smmc_engine_portfolio_cashflow_stationary_divide_kind(eng._h, C.byref(sim), C.byref(pf), C.byref(cf),
                                                                                  C.byref(st)))
