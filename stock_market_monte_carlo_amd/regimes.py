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
from .engine import SimResult, Stats, _BLOCKS_ROWS, _buffers

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


def make_regimes(means, stds, mean_durations=None, leave_q16=None, start=None, start1_q16=None):
    """The smmc_regimes of a request."""
    if (mean_durations is None) == (leave_q16 is None):
        raise ValueError("give exactly one of mean_durations and leave_q16")
    if start is not None and start1_q16 is not None:
        raise ValueError("give at most one of start and start1_q16")
    m, s = [float(x) for x in means], [float(x) for x in stds]
    if len(m) != 2 or len(s) != 2:
        raise ValueError("means and stds hold two numbers, regime 0's and regime 1's")
    if not all(math.isfinite(x) for x in m + s) or min(s) < 0.0:
        raise ValueError("means and stds must be finite, stds >= 0 (got %r, %r)" % (means, stds))
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
