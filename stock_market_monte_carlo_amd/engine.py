"""Host-side mirror of the reference's Monte-Carlo API on top of the C ABI.

Function names, argument meaning and error behaviour follow
include/stock_market_monte_carlo/simulations.h of the reference (cited per function);
the work happens in libsmmc_hip.so on the MI355X.  PyTorch only provides device
memory and the stream.
"""
import collections
import ctypes as C
import dataclasses
import os

import numpy as np

from . import _lib
from ._lib import MODE_GAUSSIAN, MODE_TABLE, SmmcError

DEFAULT_TABLE_CSV = "data/SP500_monthly_returns.csv"  # examples/benchmark_mc_cpu_v2.cpp:25


@dataclasses.dataclass
class Stats:
    """Host copy of a packed statistics record (smmc_stats + bucket counts)."""
    count: int
    below: int
    underflow: int
    overflow: int
    sum: float
    sumsq: float
    min: float
    max: float
    hist: np.ndarray
    hist_lo: float = None  # the bucket range, where the producer knows it (simulate_checkpoints; fan() reads it)
    hist_hi: float = None

    @property
    def mean(self):
        return self.sum / self.count if self.count else float("nan")

    @property
    def std(self):
        """Population standard deviation (examples/benchmark_mc_gpu.cpp:19-27)."""
        if not self.count:
            return float("nan")
        m = self.mean
        return max(self.sumsq / self.count - m * m, 0.0) ** 0.5


def stats_from_bytes(raw):
    """raw: bytes/uint8 array holding one packed record."""
    buf = np.frombuffer(bytes(raw), dtype=np.uint8)
    hdr = _lib.Stats.from_buffer_copy(buf[: C.sizeof(_lib.Stats)].tobytes())
    hist = np.frombuffer(buf[C.sizeof(_lib.Stats):].tobytes(), dtype=np.uint64)[: hdr.n_bins].copy()
    return Stats(hdr.count, hdr.below, hdr.underflow, hdr.overflow, hdr.sum, hdr.sumsq, hdr.min, hdr.max, hist)


def merge_stats_bytes(records):
    """Merges packed records (same n_bins) in the given order; returns bytes."""
    L = _lib.lib()
    acc = bytearray(records[0])
    dst = (C.c_char * len(acc)).from_buffer(acc)
    for r in records[1:]:
        src = (C.c_char * len(r)).from_buffer_copy(bytes(r))
        _lib.check(L.smmc_stats_merge(dst, src))
    return bytes(acc)


Fan = collections.namedtuple("Fan", "values clipped")


def fan(stats_list, quantiles, hist_lo=None, hist_hi=None):
    """Quantiles over time from checkpoint records: Fan(values, clipped), both [len(stats_list), len(quantiles)].
    values[k, j] is quantile quantiles[j] (0 .. 1) of record k, interpolated linearly inside the bucket in which the
    cumulative count -- underflow first, then the buckets -- reaches q * count: right to within one bucket width.
    A quantile that falls into the underflow or overflow mass cannot be located: it is returned as hist_lo or
    hist_hi and clipped[k, j] says so (-1 below the range, +1 above it, 0 inside).  NaN for an empty record.
    The bucket range is taken from the records (Engine.simulate_checkpoints fills it) unless given.
    The band a caller draws around the plotted lines (examples/visualize_returns_cpu_v2.cpp:397-411 of the
    reference draws two fixed levels there)."""
    qs = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    if qs.size and (qs.min() < 0.0 or qs.max() > 1.0):
        raise ValueError("quantiles must lie in [0, 1]")
    values = np.full((len(stats_list), qs.size), np.nan)
    clipped = np.zeros((len(stats_list), qs.size), dtype=np.int8)
    for k, st in enumerate(stats_list):
        lo = st.hist_lo if hist_lo is None else hist_lo
        hi = st.hist_hi if hist_hi is None else hist_hi
        n_bins = len(st.hist)
        if lo is None or hi is None or not n_bins:
            raise ValueError("fan() needs records with a histogram and its range")
        if not st.count:
            continue
        hist = np.asarray(st.hist, dtype=np.float64)
        edges = float(st.underflow) + np.concatenate(([0.0], np.cumsum(hist)))  # cumulative count at the bucket edges
        width = (float(hi) - float(lo)) / n_bins
        filled = np.flatnonzero(hist)
        for j, q in enumerate(qs):
            target = q * st.count
            if target < edges[0] or (filled.size == 0 and st.underflow):
                values[k, j], clipped[k, j] = lo, -1
            elif target > edges[-1] or filled.size == 0:
                values[k, j], clipped[k, j] = hi, 1
            else:
                b = min(int(np.searchsorted(edges[1:], target, side="left")), n_bins - 1)  # first bucket that closes at >= target
                b = int(filled[min(np.searchsorted(filled, b), filled.size - 1)])        # ... that holds anything
                inside = min(max((target - edges[b]) / hist[b], 0.0), 1.0)
                values[k, j] = lo + (b + inside) * width
    return Fan(values, clipped)


@dataclasses.dataclass
class SimResult:
    final: object = None        # torch.float32 [n_paths] on the engine's device, or None
    chunk_mean: object = None   # torch.float32 [ceil(n/256)] or None
    chunk_var: object = None
    stats_raw: object = None    # torch.uint8 [smmc_stats_bytes(n_bins)] on device, or None


@dataclasses.dataclass
class CashflowResult:
    """What Engine.simulate_cashflow returns: the outputs that were asked for, None for the others."""
    n_paths: int
    n_periods: int
    final: object = None         # torch.float32 [n_paths] on the engine's device: 0 for a depleted path
    paid: object = None          # torch.float32 [n_paths]: the total paid out to each path
    ruin_period: object = None   # torch.int32 [n_paths] holding uint32 values: period of depletion, 0 = never
    stats: Stats = None          # record of the final values
    depleted_at: np.ndarray = None  # uint64 [n_periods + 1]: [0] never depleted, [t] depleted at period t

    def survival(self):
        """Share of paths still alive after each period: [0] = 1, [t] = 1 - (paths depleted at periods 1 .. t) / n;
        length n_periods + 1."""
        if self.depleted_at is None:
            raise ValueError("survival() needs depleted_at (want_depleted_at=True)")
        d = np.asarray(self.depleted_at, dtype=np.float64)
        n = d.sum()
        if n == 0:
            return np.full(d.size, np.nan)
        gone = np.cumsum(d)
        gone -= d[0]  # [0] counts the paths that were never depleted
        return 1.0 - gone / n


@dataclasses.dataclass
class SweepResult:
    """What Engine.simulate_cashflow_sweep returns: S scenarios on the same paths, scenario-major; None for what was
    not asked for."""
    n_paths: int
    n_periods: int
    amounts: np.ndarray             # float32 [S]: the scenarios as they were run
    fractions: np.ndarray
    floors: np.ndarray
    final: object = None            # torch.float32 [S, n_paths] on the engine's device: 0 for a depleted path
    paid: object = None             # torch.float32 [S, n_paths]
    ruin_period: object = None      # torch.int32 [S, n_paths] holding uint32 values: period of depletion, 0 = never
    stats: list = None              # S records of the final values
    depleted_at: np.ndarray = None  # uint64 [S, n_periods + 1]: [s, 0] never depleted, [s, t] depleted at period t

    def _counts(self, what):
        if self.depleted_at is None:
            raise ValueError(f"{what}() needs depleted_at (want_depleted_at=True)")
        d = np.asarray(self.depleted_at, dtype=np.float64)
        if d.ndim != 2:
            raise ValueError("depleted_at must have shape [scenarios, n_periods + 1]")
        return d

    def survival(self):
        """[S, n_periods + 1]: row s is CashflowResult.survival() of scenario s."""
        d = self._counts("survival")
        return np.stack([CashflowResult(self.n_paths, self.n_periods, depleted_at=row).survival() for row in d]) if d.size else d

    def depleted_share(self):
        """[S]: the share of paths depleted at any period."""
        d = self._counts("depleted_share")
        n = d.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, (n - d[:, 0]) / n, np.nan)

    def highest_surviving(self, confidence):
        """The index of the scenario with the largest amount whose share of paths alive after the last period is at
        least `confidence` (0 .. 1); None if no scenario of the swept grid reaches it (ties: the first such scenario)."""
        alive = self.survival()[:, -1]
        best = None
        for s in np.flatnonzero(alive >= float(confidence)):
            if best is None or self.amounts[s] > self.amounts[best]:
                best = int(s)
        return best


@dataclasses.dataclass
class AllocationSweepResult(SweepResult):
    """What Engine.simulate_allocation_sweep returns: SweepResult's outputs (survival() and depleted_share() included) of
    S portfolio strategies on the same jointly drawn paths, and the final holdings."""
    weights: np.ndarray = None          # float32 [S, K]: the strategies as they were run
    rebalance_every: np.ndarray = None  # uint32 [S]
    n_assets: int = 0
    holdings: object = None             # torch.float32 [S, K, n_paths]: the final holdings (no rebalance at P)

    def surviving(self, confidence):
        """The indices of the scenarios whose share of paths alive after the last period is at least `confidence` (0 .. 1)."""
        return [int(s) for s in np.flatnonzero(self.survival()[:, -1] >= float(confidence))]


def _by_period(counts, what):
    """Cumulative share of paths whose first passage lies at or before each period, from a [n_periods + 1] count
    array ([0]: never, [t]: first at period t)."""
    if counts is None:
        raise ValueError(f"{what}() needs its count array (want_first_{'below' if what == 'ever_below' else 'reach'}_at=True)")
    d = np.asarray(counts, dtype=np.float64)
    n = d.sum()
    if n == 0:
        return np.full(d.size, np.nan)
    hit = np.cumsum(d)
    hit -= d[0]  # [0] counts the paths that never got there
    return hit / n


@dataclasses.dataclass
class ExcursionResult:
    """What Engine.simulate_excursions returns: the outputs that were asked for, None for the others."""
    n_paths: int
    n_periods: int
    final: object = None            # torch.float32 [n_paths] on the engine's device
    peak: object = None             # torch.float32 [n_paths]: the largest value of the path, v_0 included
    low: object = None              # torch.float32 [n_paths]: the smallest
    drawdown: object = None         # torch.float32 [n_paths]: the deepest relative drawdown, (peak - trough) / peak
    drawdown_period: object = None  # torch.int32 [n_paths] holding uint32 values: period of that trough, 0 = none
    underwater: object = None       # torch.int32 [n_paths]: the longest run of periods below the running peak
    first_below: object = None      # torch.int32 [n_paths]: first period with value < lower, 0 = never
    first_reach: object = None      # torch.int32 [n_paths]: first period with value >= target, 0 = never
    stats: Stats = None             # record of the final values
    drawdown_stats: Stats = None    # record of the drawdowns: buckets over [0, 1), below = drawdown < drawdown_threshold
    first_below_at: np.ndarray = None  # uint64 [n_periods + 1]: [0] never below, [t] first below at period t
    first_reach_at: np.ndarray = None  # uint64 [n_periods + 1]: the same for the target

    def ever_below(self):
        """Share of paths that have been below `lower` by each period: [0] = 0, non-decreasing, n_periods + 1 entries."""
        return _by_period(self.first_below_at, "ever_below")

    def reached_by(self):
        """Share of paths that have reached `target` by each period; n_periods + 1 entries."""
        return _by_period(self.first_reach_at, "reached_by")


@dataclasses.dataclass
class PortfolioResult:
    """What Engine.simulate_portfolio returns: the outputs that were asked for, None for the others."""
    n_paths: int
    n_assets: int
    final: object = None     # torch.float32 [n_paths] on the engine's device: V_P
    holdings: object = None  # torch.float32 [n_assets, n_paths]: the final holdings, before any rebalance at P
    stats: Stats = None      # record of the final values


@dataclasses.dataclass
class PortfolioCashflowResult(CashflowResult):
    """What Engine.simulate_portfolio_cashflow returns: CashflowResult's outputs (survival() included) of the portfolio's
    value, and the final holdings."""
    n_assets: int = 0
    holdings: object = None  # torch.float32 [n_assets, n_paths]: the final holdings (no rebalance at P), 0 for a depleted path


@dataclasses.dataclass
class PortfolioCashflowCheckpointsResult(PortfolioCashflowResult):
    """What Engine.simulate_portfolio_cashflow_checkpoints returns: PortfolioCashflowResult's outputs and the record of
    the paths' values after each chosen period (0 for a path depleted by then)."""
    periods: np.ndarray = None  # uint32 [n_checkpoints]
    checkpoints: list = None    # [Stats per checkpoint], hist_lo / hist_hi filled

    def fan(self, quantiles):
        """The fan chart: fan(self.checkpoints, quantiles) -- [n_checkpoints, len(quantiles)] values."""
        return fan(self.checkpoints, quantiles)

    def depleted_by(self):
        """Share of paths depleted at or before each checkpoint's period: float64 [n_checkpoints]."""
        if self.depleted_at is None:
            raise ValueError("depleted_by() needs depleted_at (want_depleted_at=True)")
        d = np.asarray(self.depleted_at, dtype=np.float64)
        n = d.sum()
        if n == 0:
            return np.full(len(self.periods), np.nan)
        gone = np.cumsum(d) - d[0]  # [0] counts the paths that were never depleted
        return gone[np.asarray(self.periods, dtype=np.int64)] / n


@dataclasses.dataclass
class RealCashflowResult(PortfolioCashflowResult):
    """What Engine.simulate_real_cashflow returns: PortfolioCashflowResult's nominal outputs (survival() included), the
    final values in money of period 0 and the price index they were divided by; stats is the record of final_real."""
    final_real: object = None  # torch.float32 [n_paths]: final / index
    index: object = None       # torch.float32 [n_paths]: the price index after the last period (1.0 at the start)


@dataclasses.dataclass
class GuardrailsResult(PortfolioCashflowResult):
    """What Engine.simulate_guardrails returns: PortfolioCashflowResult's outputs (survival() included), the amounts in
    force per path and the counts of cuts and raises, per path and per review."""
    amount_last: object = None    # torch.float32 [n_paths]: the amount in force after the last review
    amount_lowest: object = None  # torch.float32 [n_paths]: the lowest amount ever in force
    cuts: object = None           # torch.int32 [n_paths] holding uint32 values: the path's cuts
    raises: object = None         # torch.int32 [n_paths] holding uint32 values: the path's raises
    cuts_at: np.ndarray = None    # uint64 [n_periods + 1]: [t] paths cut at the review after period t; [0] stays 0
    raises_at: np.ndarray = None  # uint64 [n_periods + 1], likewise

    def ever_cut(self):
        """Share of paths with at least one cut."""
        if self.cuts is None:
            raise ValueError("ever_cut() needs cuts (want_cuts=True)")
        if self.n_paths == 0:
            return float("nan")
        return float((self.cuts > 0).sum().item()) / self.n_paths

    def cut_by(self):
        """Cuts made by period t per path, cumulative, length n_periods + 1: cumsum(cuts_at) / n_paths.  Where no path is
        cut more than once (cuts.max() <= 1) this is the share of paths first cut by period t; cuts_at counts EVERY cut,
        and the contract has no per-path period of the first one, so with repeated cuts it is an upper bound of that
        share (ever_cut() is its exact last value)."""
        if self.cuts_at is None:
            raise ValueError("cut_by() needs cuts_at (want_cuts_at=True)")
        if self.n_paths == 0:
            return np.full(len(self.cuts_at), np.nan)
        return np.cumsum(np.asarray(self.cuts_at, dtype=np.float64)) / self.n_paths


def glide_linear(w_from, w_to, first, last, every=1):
    """The `changes` list of Engine.simulate_glide for a straight-line glide: the targets are `w_from` at period `first`,
    `w_to` at period `last` and move between them in steps of `every` periods -- rows at first, first + every, ... below
    `last`, and one at `last`.  The two end rows are the inputs as float32, unchanged; the rows between are interpolated
    in double, cast to float32 and renormalised so that each sums to 1 well within the library's 1e-6.  With first == 0
    the first row is left out: before the first change the call's own `weights` hold, so pass w_from there."""
    a, b = np.asarray(w_from, dtype=np.float32).ravel(), np.asarray(w_to, dtype=np.float32).ravel()
    first, last, every = int(first), int(last), int(every)
    if a.size != b.size or a.size == 0:
        raise ValueError("w_from and w_to must have the same number of weights")
    if not (0 <= first < last) or every < 1:
        raise ValueError("glide_linear needs 0 <= first < last and every >= 1")
    out = []
    for t in range(first, last, every):
        if t == first:
            row = a.copy()
        else:
            mix = (a.astype(np.float64) * (last - t) + b.astype(np.float64) * (t - first)) / (last - first)
            row = (mix / mix.sum()).astype(np.float32)
            row = (row.astype(np.float64) / row.astype(np.float64).sum()).astype(np.float32)
        if t >= 1:
            out.append((t, row))
    out.append((last, b.copy()))
    return out


def cholesky_factor(stds, corr):
    """The lower-triangular factor L (float32 [K, K], percent) of diag(stds) corr diag(stds), for
    Engine.simulate_portfolio(factor=...): numpy's float64 Cholesky, cast once.  Raises ValueError for a matrix that
    is not symmetric positive definite."""
    sd = np.asarray(stds, dtype=np.float64)
    c = np.asarray(corr, dtype=np.float64)
    if sd.ndim != 1 or c.shape != (sd.size, sd.size):
        raise ValueError("stds must have K entries and corr K x K")
    if not (np.isfinite(sd).all() and np.isfinite(c).all() and (sd > 0).all() and np.allclose(c, c.T)):
        raise ValueError("stds must be positive and corr symmetric and finite")
    try:
        return np.linalg.cholesky(sd[:, None] * c * sd[None, :]).astype(np.float32)
    except np.linalg.LinAlgError as err:
        raise ValueError("the covariance matrix is not positive definite") from err


# ---------------------------------------------------------------------------
# The outputs of the feature entries, stated once: Engine._outputs allocates from these tables and fills the outputs
# structure, Engine._read_back decodes what a simulate_X reads back.  A new feature adds its rows and its short entries.
# ---------------------------------------------------------------------------

# An output kind: torch dtype (by name) on the device, numpy dtype on the host, device elements per host element.
_Kind = collections.namedtuple("_Kind", "torch numpy unit")
_FLOAT = _Kind("float32", np.float32, 1)  # per-path float
_UINT = _Kind("int32", np.uint32, 1)      # per-path uint32: int32 holding the uint32 values on the device
_RECORD = _Kind("uint8", np.uint64, 8)    # packed record(s): smmc_stats_bytes(n_bins) bytes on the device; uint64 on the host, handed back as bytes
_COUNTS = _Kind("int64", np.uint64, 1)    # count array: int64 holding the uint64 counts on the device

# What a shape is a function of: paths, periods, assets, the sweeps' leading scenario dimension -- () or (S,) --, bytes of a record.
_Dims = collections.namedtuple("_Dims", "n p K S rec")

# field of an outputs structure (or C parameter of the entries that take loose pointers) -> (kind, shape without S)
_OUTPUT = {"holdings": (_FLOAT, lambda d: (d.K, d.n)),
           "chunk_mean": (_FLOAT, lambda d: ((d.n + _lib.CHUNK - 1) // _lib.CHUNK,)),
           "chunk_var": (_FLOAT, lambda d: ((d.n + _lib.CHUNK - 1) // _lib.CHUNK,))}
_OUTPUT.update({f: (_FLOAT, lambda d: (d.n,)) for f in ("final", "final_real", "index", "paid", "amount_last", "amount_lowest", "peak", "low",
                                                       "drawdown")})
_OUTPUT.update({f: (_UINT, lambda d: (d.n,)) for f in ("ruin_period", "cuts", "raises", "drawdown_period", "underwater", "first_below",
                                                      "first_reach")})
_OUTPUT.update({f: (_RECORD, lambda d: (d.rec,)) for f in ("stats", "drawdown_stats")})
_OUTPUT.update({f: (_COUNTS, lambda d: (d.p + 1,)) for f in ("depleted_at", "cuts_at", "raises_at", "first_below_at", "first_reach_at")})


def _rows(fields, stats_key="stats_raw"):
    """The output table of a structure or a parameter list: rows (field, result key, kind, shape), in the C order."""
    return tuple((f, stats_key if f == "stats" else f) + _OUTPUT[f] for f in fields)


def _pointer_fields(struct):
    return tuple(name for name, _ in struct._fields_ if name not in ("struct_size", "reserved"))


_CASHFLOW_ROWS = _rows(("final", "paid", "ruin_period", "stats", "depleted_at"))  # loose pointers: cashflow, cashflow_sweep
_BLOCKS_ROWS = _rows(("final", "chunk_mean", "chunk_var", "stats"))               # loose pointers: blocks
_PORTFOLIO_ROWS = _rows(_pointer_fields(_lib.PortfolioOutputs))
_PFCF_ROWS = _rows(_pointer_fields(_lib.PortfolioCashflowOutputs))                # and smmc_allocation_sweep_outputs
_REAL_ROWS = _rows(_pointer_fields(_lib.RealCashflowOutputs))
_GUARDRAILS_ROWS = _rows(_lib.GUARDRAILS_OUTPUTS)
_EXCURSION_ROWS = _rows(_lib.EXCURSION_OUTPUTS, stats_key="stats")


def _buffers(rows, res):
    return [res[key] for _, key, _, _ in rows]


def _records_as_bytes(rows, res):
    """The host flavour's last step, after the C call: a record is handed back as bytes."""
    for _, key, kind, _ in rows:
        if kind is _RECORD and res[key] is not None:
            res[key] = res[key].tobytes()
    return res


class Engine:
    """One engine per (process, device): table, workspace and stream stay resident."""

    def __init__(self, device=0, stream="torch"):
        import torch
        self._torch = torch
        self._L = _lib.lib()
        if not torch.cuda.is_available():
            raise SmmcError("no MI355X visible to this process; the engine has no CPU fallback")
        self.device = int(device)
        self.tdevice = torch.device("cuda", self.device)
        # "torch": launch on torch's current stream of that device (handle 0 = the default
        # stream), so tensors produced here are ordered with the caller's torch work;
        # "new": an engine-owned non-blocking stream; or a raw hipStream_t handle.
        if stream == "torch":
            sp = int(torch.cuda.current_stream(self.tdevice).cuda_stream)
        elif stream == "new":
            sp = -1  # SMMC_STREAM_NEW
        else:
            sp = int(stream)
        self.own_stream = sp == -1
        self.follow_torch = stream == "torch"
        h = C.c_void_p()
        _lib.check(self._L.smmc_engine_create(self.device, C.c_void_p(sp), C.byref(h)))
        self._h = h
        self.table_len = 0

    # -- stream discipline ---------------------------------------------------
    def _enter(self):
        """Before enqueuing: launches go to the caller's CURRENT torch stream (a "torch" engine
        re-binds on every call: the caller may be inside `with torch.cuda.stream(s)` now), or the
        engine's own stream first waits for it (its outputs were just allocated there)."""
        self._uniform_hi_from_env()
        cur = int(self._torch.cuda.current_stream(self.tdevice).cuda_stream)
        if self.follow_torch:
            _lib.check(self._L.smmc_engine_set_stream(self._h, C.c_void_p(cur)))
        elif self.own_stream:
            _lib.check(self._L.smmc_engine_wait_stream(self._h, C.c_void_p(cur)))
        return cur

    def _uniform_hi_from_env(self):
        """SMMC_UNIFORM_HI (0 | 1, default 1), read before every call: the library itself has the switch as a call
        (smmc_set_uniform_hi), this wrapper maps the variable onto it so that a whole run -- bench.py, a profile of
        the generic kernel -- is switched from outside.  Anything but "0" leaves the default."""
        _lib.check(self._L.smmc_set_uniform_hi(0 if os.environ.get("SMMC_UNIFORM_HI", "1").strip() == "0" else 1))

    def _leave(self, cur, *tensors):
        """After enqueuing on an engine-owned stream: torch's current stream waits for the engine's
        work, so whatever torch does next with the outputs there -- read, free, reuse the block --
        is ordered after the kernels that wrote them (no record_stream: the caching allocator would
        poll events on a stream the engine may already have destroyed)."""
        if self.own_stream:
            _lib.check(self._L.smmc_engine_release_to_stream(self._h, C.c_void_p(cur)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.smmc_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------
    def set_table(self, returns_percent):
        t = np.ascontiguousarray(returns_percent, dtype=np.float32)
        self._enter()  # never act on a stream bound by an earlier call: the caller may have destroyed it since
        _lib.check(self._L.smmc_engine_set_table(self._h, t.ctypes.data_as(C.c_void_p), t.size))
        self.table_len = int(t.size)

    def geometry(self):
        g, b, cu = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _lib.check(self._L.smmc_engine_geometry(self._h, C.byref(g), C.byref(b), C.byref(cu)))
        return g.value, b.value, cu.value

    def timing(self, enable=True):
        _lib.check(self._L.smmc_engine_timing(self._h, 1 if enable else 0))

    def kernel_ms(self):
        """(summed main-kernel milliseconds, launches) since the last call; synchronises."""
        ms, n = C.c_double(), C.c_uint32()
        self._enter()
        _lib.check(self._L.smmc_engine_kernel_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_clock_ghz(self):
        """The shader clock the chip held, averaged over the workgroups of the path-kernel launches timed since the
        last call (0.0 if none was sampled); synchronises."""
        ghz = C.c_double()
        self._enter()
        _lib.check(self._L.smmc_engine_kernel_clock(self._h, C.byref(ghz)))
        return ghz.value

    def selftest(self, bits_lo, bits_hi):
        """Mismatches of the device's divide-by-100 shortcut vs the IEEE divide on [lo, hi)."""
        a = C.c_uint64()
        _lib.check(self._L.smmc_engine_selftest(self._h, bits_lo, bits_hi, C.byref(a)))
        return a.value

    def selftest_draws(self, sim, words, form=0):
        """The multipliers the device draws from GIVEN words in sim's mode and stream (smmc_engine_selftest_draws):
        words is (n, 4) uint32, one item per row in the place of a Philox block's output; returns float32
        (n, draws), draws = 8 for a table of up to 2048 entries, else 4.  form 0 draws one item at a time, form 1
        two together as the kernels that interleave two blocks do.  Waits for the result."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if w.ndim != 2 or w.shape[1] != 4:
            raise ValueError("words must have shape (n, 4)")
        n, draws = int(w.shape[0]), C.c_uint32()
        self._enter()
        # the count first (n = 0 touches no buffer), then the call itself into an array of that width
        _lib.check(self._L.smmc_engine_selftest_draws(self._h, C.byref(sim), None, 0, int(form), None, C.byref(draws)))
        out = np.empty((n, draws.value), dtype=np.float32)
        if n:
            _lib.check(self._L.smmc_engine_selftest_draws(self._h, C.byref(sim), w.ctypes.data_as(C.c_void_p), n, int(form),
                                                          out.ctypes.data_as(C.c_void_p), C.byref(draws)))
        return out

    def sync(self):
        """Waits for everything the engine has enqueued.  A "torch" engine first re-binds to the caller's
        current stream (work enqueued on the stream of an earlier call stays ordered before it; a stream
        handed to the engine must outlive its pending work, not the engine)."""
        self._enter()
        _lib.check(self._L.smmc_engine_sync(self._h))

    # -- simulation ----------------------------------------------------------
    @staticmethod
    def make_sim(n_paths, n_periods, mode, seed, first_path=0, initial_capital=1000.0, gauss_mean=0.5,
                 gauss_std=0.83333, n_bins=0, hist_lo=0.0, hist_hi=1.0, below_threshold=None,
                 exact_div=False, stream=3):
        s = _lib.Sim()
        s.struct_size = C.sizeof(_lib.Sim)
        s.mode = mode
        s.seed = seed & 0xFFFFFFFFFFFFFFFF
        s.first_path = first_path
        s.n_paths = n_paths
        s.n_periods = n_periods
        s.initial_capital = initial_capital
        s.gauss_mean = gauss_mean
        s.gauss_std = gauss_std
        s.n_bins = n_bins
        s.hist_lo = hist_lo
        s.hist_hi = hist_hi
        s.below_threshold = initial_capital if below_threshold is None else below_threshold
        if stream not in (2, 3, "ref"):
            raise ValueError("stream must be 3 or 2 (the counter stream: Philox counter layout in both modes and "
                             "the Gaussian draw) or 'ref' (the reference CPU engine's per-path mt19937 stream)")
        s.flags = ((_lib.FLAG_EXACT_DIV if exact_div else 0) | (_lib.FLAG_STREAM_V2 if stream == 2 else 0)
                   | (_lib.FLAG_STREAM_REF if stream == "ref" else 0))
        return s

    def simulate(self, sim, want_final=True, want_chunk_stats=False, want_stats=False, out=None):
        """Enqueues one simulation on the engine stream; returns device tensors."""
        torch = self._torch
        n = int(sim.n_paths)
        res = SimResult()
        if want_final:
            res.final = out if out is not None else torch.empty(n, dtype=torch.float32, device=self.tdevice)
            assert res.final.numel() >= n and res.final.dtype == torch.float32 and res.final.is_contiguous()
        if want_chunk_stats:
            nc = (n + _lib.CHUNK - 1) // _lib.CHUNK
            res.chunk_mean = torch.empty(nc, dtype=torch.float32, device=self.tdevice)
            res.chunk_var = torch.empty(nc, dtype=torch.float32, device=self.tdevice)
        if want_stats:
            res.stats_raw = torch.empty(int(self._L.smmc_stats_bytes(sim.n_bins)), dtype=torch.uint8,
                                        device=self.tdevice)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
        cur = self._enter()
        _lib.check(self._L.smmc_engine_simulate(self._h, C.byref(sim), ptr(res.final), ptr(res.chunk_mean),
                                                ptr(res.chunk_var), ptr(res.stats_raw)))
        self._leave(cur, res.final, res.chunk_mean, res.chunk_var, res.stats_raw)
        return res

    def simulate_checkpoints(self, sim, periods, want_final=False):
        """The value distribution at chosen periods: ([Stats per checkpoint], final values or None).
        periods: strictly increasing integers in 1 .. n_periods (any integer sequence), at most
        _lib.MAX_CHECKPOINTS of them; record k describes the paths' values after periods[k] compounding steps --
        column periods[k] of simulate_keepdata's trajectories -- with sim's threshold and bucket range
        (smmc_engine_simulate_checkpoints, include/smmc.h).  Waits for the records; the final values stay on
        the device."""
        torch = self._torch
        per = np.ascontiguousarray([int(p) for p in periods], dtype=np.int64)
        if per.size and (per.min() < 0 or per.max() > 0xFFFFFFFF):
            raise ValueError("periods must be non-negative 32-bit integers")
        per = per.astype(np.uint32)
        n, rec = int(sim.n_paths), int(self._L.smmc_stats_bytes(sim.n_bins))
        final = torch.empty(n, dtype=torch.float32, device=self.tdevice) if want_final else None
        raw = torch.empty(max(per.size, 1) * rec, dtype=torch.uint8, device=self.tdevice)
        cur = self._enter()
        _lib.check(self._L.smmc_engine_simulate_checkpoints(
            self._h, C.byref(sim), per.ctypes.data_as(C.c_void_p), per.size,
            C.c_void_p(final.data_ptr()) if final is not None and n else None, C.c_void_p(raw.data_ptr())))
        self._leave(cur, final, raw)
        self.sync()
        host = raw.cpu().numpy().tobytes()
        out = []
        for k in range(per.size):
            st = stats_from_bytes(host[k * rec:(k + 1) * rec])
            st.hist_lo, st.hist_hi = float(sim.hist_lo), float(sim.hist_hi)
            out.append(st)
        return out, final

    def simulate_checkpoints_raw(self, sim, periods, want_final=False, to_host=False):
        """The packed records as bytes (n_checkpoints x smmc_stats_bytes(n_bins)) and the final values (numpy, or
        None): through the device entry, or through smmc_engine_simulate_checkpoints_to_host."""
        per = np.ascontiguousarray(periods, dtype=np.uint32)
        n, rec = int(sim.n_paths), int(self._L.smmc_stats_bytes(sim.n_bins))
        if to_host:
            buf = np.zeros(max(per.size, 1) * rec, dtype=np.uint8)
            final = np.empty(n, dtype=np.float32) if want_final else None
            self._enter()
            _lib.check(self._L.smmc_engine_simulate_checkpoints_to_host(
                self._h, C.byref(sim), per.ctypes.data_as(C.c_void_p), per.size,
                final.ctypes.data_as(C.c_void_p) if final is not None else None, buf.ctypes.data_as(C.c_void_p)))
            return buf[: per.size * rec].tobytes(), final
        torch = self._torch
        final = torch.empty(n, dtype=torch.float32, device=self.tdevice) if want_final else None
        raw = torch.empty(max(per.size, 1) * rec, dtype=torch.uint8, device=self.tdevice)
        cur = self._enter()
        _lib.check(self._L.smmc_engine_simulate_checkpoints(
            self._h, C.byref(sim), per.ctypes.data_as(C.c_void_p), per.size,
            C.c_void_p(final.data_ptr()) if final is not None and n else None, C.c_void_p(raw.data_ptr())))
        self._leave(cur, final, raw)
        self.sync()
        return raw.cpu().numpy()[: per.size * rec].tobytes(), (final.cpu().numpy() if final is not None else None)

    # -- the binding layer of the feature entries (the tables above) ---------------------------------------------------
    def _new(self, kind, shape, host):
        """One output buffer: zeroed numpy on the host, uninitialised torch on the engine's device; `shape` counts device
        elements."""
        if host:
            return np.zeros(shape[:-1] + (shape[-1] // kind.unit,), dtype=kind.numpy)
        return self._torch.empty(shape, dtype=getattr(self._torch, kind.torch), device=self.tdevice)

    def _outputs(self, rows, struct, sim, wants, host, K=0, S=None, head=None, given=None, host_null_empty=False):
        """Allocates what `wants` (one flag per row) asks for: (result dict -- `head`, then the rows' keys, None for what is
        not wanted --, `struct` filled with the addresses, or for struct None the list of pointer arguments).  `given` maps
        a key to a caller's buffer to use in place of a new one (None: none).  A device output without elements is passed
        as a null pointer; a host one only with host_null_empty."""
        d = _Dims(int(sim.n_paths), int(sim.n_periods), int(K), () if S is None else (int(S),), int(self._L.smmc_stats_bytes(sim.n_bins)))
        assert len(wants) == len(rows)
        res, addresses = dict(head or {}), []
        for (field, key, kind, shape), want in zip(rows, wants):
            buf = (given or {}).get(key) if want else None
            if want and buf is None:
                buf = self._new(kind, d.S + shape(d), host)
            res[key] = buf
            if buf is None:
                addresses.append(None)
            elif host:
                addresses.append(buf.ctypes.data if buf.size or not host_null_empty else None)
            else:
                addresses.append(buf.data_ptr() if buf.numel() else None)
        if struct is None:
            return res, [None if a is None else C.c_void_p(a) for a in addresses]
        o = struct()
        o.struct_size = C.sizeof(struct)
        for (field, _, _, _), a in zip(rows, addresses):
            setattr(o, field, a)
        return res, o

    def _run(self, entry, *args, device=None):
        """The stream discipline around the one C call of an entry; `device`: the tensors it writes (a _to_host entry has
        none, the call has drained its streams when it returns)."""
        cur = self._enter()
        _lib.check(entry(self._h, *args))
        if device is not None:
            self._leave(cur, *device)

    def _read_back(self, res, sim, raw, rows, n_records=None, also=(), ranges=None):
        """Finishes a simulate_X: the rows' records and count arrays that `raw` holds go to the host and into `res`, under
        the field's name -- a record as Stats (n_records given: a list of so many) with sim's bucket range, or the one
        `ranges` names for the field; a count array as a uint64 copy.  `also`: further (attribute, key, kind, n_records).
        Waits for the engine only if there is something to read."""
        items = [(field, key, kind, n_records) for field, key, kind, _ in rows if kind in (_RECORD, _COUNTS)] + list(also)
        items = [item for item in items if raw[item[1]] is not None]
        if items:
            self.sync()
        rec = int(self._L.smmc_stats_bytes(sim.n_bins))
        for attr, key, kind, count in items:
            if kind is _COUNTS:
                setattr(res, attr, raw[key].cpu().numpy().view(np.uint64).copy())
                continue
            host, out = raw[key].cpu().numpy().tobytes(), []
            for k in range(1 if count is None else count):
                st = stats_from_bytes(host[k * rec:(k + 1) * rec])
                st.hist_lo, st.hist_hi = (ranges or {}).get(attr, (float(sim.hist_lo), float(sim.hist_hi)))
                out.append(st)
            setattr(res, attr, out[0] if count is None else out)
        return res

    @staticmethod
    def _kind(rc):
        """The tail of a *_divide_kind call: a negative return is the library's error."""
        if rc < 0:
            _lib.check(rc)
        return rc

    # -- cash flows: withdrawal and contribution schedules (smmc_engine_simulate_cashflow) ------------
    @staticmethod
    def make_cashflow(n_periods, amount=0.0, fraction=0.0, amounts=None, fractions=None, floor=0.0):
        """(smmc_cashflow, the arrays it points to): keep the second alive until the call has returned."""
        keep = []
        cf = _lib.Cashflow()
        cf.struct_size = C.sizeof(_lib.Cashflow)
        cf.amount, cf.fraction, cf.floor = float(amount), float(fraction), float(floor)
        for name, arr in (("amounts", amounts), ("fractions", fractions)):
            if arr is None:
                continue
            a = np.ascontiguousarray(arr, dtype=np.float32)
            if a.ndim != 1 or a.size != int(n_periods):
                raise ValueError(f"{name} must hold n_periods = {int(n_periods)} entries")
            keep.append(a)
            setattr(cf, name, a.ctypes.data)
        return cf, keep

    def simulate_cashflow(self, sim, amount=0.0, fraction=0.0, amounts=None, fractions=None, floor=0.0,
                          want_final=True, want_paid=False, want_ruin_period=False, want_stats=False,
                          want_depleted_at=True):
        """One simulation in which, after every period's return, amount + fraction * value is taken out of every
        path (negative amounts are contributions): a fixed amount, some percentage, or per-period arrays of
        n_periods entries (amounts, fractions).  A path whose value would not stay above `floor` is depleted: it pays
        out what is left and stays at 0.  Returns a CashflowResult; per-path outputs stay on the device,
        stats and depleted_at are read back (that waits).  include/smmc.h states the arithmetic."""
        raw = self.simulate_cashflow_raw(sim, amount, fraction, amounts, fractions, floor, want_final, want_paid,
                                         want_ruin_period, want_stats, want_depleted_at)
        res = CashflowResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"])
        return self._read_back(res, sim, raw, _CASHFLOW_ROWS)

    def simulate_cashflow_raw(self, sim, amount=0.0, fraction=0.0, amounts=None, fractions=None, floor=0.0,
                              want_final=True, want_paid=False, want_ruin_period=False, want_stats=False,
                              want_depleted_at=True):
        """Enqueues the call and returns its device tensors without waiting: a dict with final, paid (float32),
        ruin_period (int32 holding uint32 values), stats_raw (uint8, the packed record) and depleted_at (int64
        holding uint64 counts, n_periods + 1); None for what was not asked for."""
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        out, ptrs = self._outputs(_CASHFLOW_ROWS, None, sim, (want_final, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                  host=False)
        self._run(self._L.smmc_engine_simulate_cashflow, C.byref(sim), C.byref(cf), *ptrs, device=_buffers(_CASHFLOW_ROWS, out))
        del keep
        return out

    def simulate_cashflow_to_host(self, sim, amount=0.0, fraction=0.0, amounts=None, fractions=None, floor=0.0,
                                  want_final=True, want_paid=False, want_ruin_period=False, want_stats=False,
                                  want_depleted_at=True):
        """The same through smmc_engine_simulate_cashflow_to_host: a dict of numpy arrays (stats_raw: bytes)."""
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        out, ptrs = self._outputs(_CASHFLOW_ROWS, None, sim, (want_final, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                  host=True)
        self._run(self._L.smmc_engine_simulate_cashflow_to_host, C.byref(sim), C.byref(cf), *ptrs)
        del keep
        return _records_as_bytes(_CASHFLOW_ROWS, out)

    def cashflow_divide_kind(self, sim, amount=0.0, fraction=0.0, amounts=None, fractions=None, floor=0.0):
        """_lib.DIV_FAST or DIV_EXACT: the divide simulate_cashflow uses for this request (results never depend on it)."""
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)  # keep lives until the return
        return self._kind(self._L.smmc_engine_cashflow_divide_kind(self._h, C.byref(sim), C.byref(cf)))

    # -- cash-flow sweeps: up to MAX_SWEEP constant schedules on the same paths (smmc_engine_simulate_cashflow_sweep) ----
    @staticmethod
    def make_sweep(amounts, fractions=0.0, floors=0.0):
        """(array of smmc_cashflow, amounts, fractions, floors as float32 [S]): scalars broadcast over the scenarios."""
        try:
            am, fr, fl = np.broadcast_arrays(np.atleast_1d(np.asarray(amounts, dtype=np.float32)),
                                             np.asarray(fractions, dtype=np.float32), np.asarray(floors, dtype=np.float32))
        except ValueError:
            raise ValueError("amounts, fractions and floors must be scalars or sequences of one length") from None
        if am.ndim != 1:
            raise ValueError("amounts, fractions and floors must be scalars or one-dimensional")
        cfs = (_lib.Cashflow * max(am.size, 1))()
        for s in range(am.size):
            cfs[s].struct_size = C.sizeof(_lib.Cashflow)
            cfs[s].amount, cfs[s].fraction, cfs[s].floor = float(am[s]), float(fr[s]), float(fl[s])
        return cfs, am.copy(), fr.copy(), fl.copy()

    def simulate_cashflow_sweep(self, sim, amounts, fractions=0.0, floors=0.0, want_final=False, want_paid=False,
                                want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """Up to MAX_SWEEP constant cash-flow schedules on the SAME paths in one launch: scenario s takes amounts[s] +
        fractions[s] * value out after every period and is depleted at floors[s], exactly as simulate_cashflow with
        those three (scalars broadcast).  Returns a SweepResult; per-path outputs ([S, n_paths]) stay on the device,
        stats and depleted_at are read back (that waits).  include/smmc.h states the contract."""
        raw = self.simulate_cashflow_sweep_raw(sim, amounts, fractions, floors, want_final, want_paid, want_ruin_period,
                                               want_stats, want_depleted_at)
        _, am, fr, fl = self.make_sweep(amounts, fractions, floors)
        res = SweepResult(int(sim.n_paths), int(sim.n_periods), am, fr, fl, raw["final"], raw["paid"], raw["ruin_period"])
        return self._read_back(res, sim, raw, _CASHFLOW_ROWS, n_records=am.size)

    def simulate_cashflow_sweep_raw(self, sim, amounts, fractions=0.0, floors=0.0, want_final=False, want_paid=False,
                                    want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """Enqueues the sweep and returns its device tensors without waiting: a dict with final, paid (float32
        [S, n_paths]), ruin_period (int32 holding uint32 values), stats_raw (uint8 [S, smmc_stats_bytes(n_bins)]) and
        depleted_at (int64 holding uint64 counts, [S, n_periods + 1]); None for what was not asked for."""
        cfs, am, _, _ = self.make_sweep(amounts, fractions, floors)
        S = int(am.size)
        out, ptrs = self._outputs(_CASHFLOW_ROWS, None, sim, (want_final, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                  host=False, S=S)
        self._run(self._L.smmc_engine_simulate_cashflow_sweep, C.byref(sim), cfs, S, *ptrs, device=_buffers(_CASHFLOW_ROWS, out))
        return out

    def simulate_cashflow_sweep_to_host(self, sim, amounts, fractions=0.0, floors=0.0, want_final=False, want_paid=False,
                                        want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """The same through smmc_engine_simulate_cashflow_sweep_to_host: a dict of numpy arrays, scenario-major
        (stats_raw: the S packed records as bytes)."""
        cfs, am, _, _ = self.make_sweep(amounts, fractions, floors)
        S = int(am.size)
        out, ptrs = self._outputs(_CASHFLOW_ROWS, None, sim, (want_final, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                  host=True, S=S)
        self._run(self._L.smmc_engine_simulate_cashflow_sweep_to_host, C.byref(sim), cfs, S, *ptrs)
        return _records_as_bytes(_CASHFLOW_ROWS, out)

    def cashflow_sweep_divide_kind(self, sim, amounts, fractions=0.0, floors=0.0):
        """_lib.DIV_FAST or DIV_EXACT: the divide simulate_cashflow_sweep uses for this request: FAST only if every
        scenario's own rule says so (results never depend on it)."""
        cfs, am, _, _ = self.make_sweep(amounts, fractions, floors)
        return self._kind(self._L.smmc_engine_cashflow_sweep_divide_kind(self._h, C.byref(sim), cfs, int(am.size)))

    # -- excursions: drawdown, running extremes, first passage of levels (smmc_engine_simulate_excursions) --------
    _EXCURSION_WANTS = dict(final=True, peak=False, low=False, drawdown=False, drawdown_period=False, underwater=False,
                            first_below=False, first_reach=False, stats=False, drawdown_stats=True, first_below_at=True,
                            first_reach_at=True)

    @staticmethod
    def make_excursions(lower, target, drawdown_threshold=0.2):
        x = _lib.Excursions()
        x.struct_size = C.sizeof(_lib.Excursions)
        x.lower, x.target, x.drawdown_threshold = float(lower), float(target), float(drawdown_threshold)
        return x

    def _excursion_wants(self, wants):
        """The want_<name> arguments over the defaults: one flag per row of _EXCURSION_ROWS."""
        full = dict(self._EXCURSION_WANTS)
        for key, val in wants.items():
            if not key.startswith("want_") or key[5:] not in full:
                raise TypeError(f"unknown argument {key!r}")
            full[key[5:]] = bool(val)
        return [full[field] for field in _lib.EXCURSION_OUTPUTS]

    def simulate_excursions(self, sim, lower, target, drawdown_threshold=0.2, **wants):
        """One simulation reduced ALONG every path: running peak and low, the deepest relative drawdown and its
        period, the longest run of periods under water, the first period below `lower` and the first at or above
        `target`.  want_<name>=True / False selects the outputs (names: the fields of ExcursionResult; by default
        final, drawdown_stats and the two count arrays).  Per-path outputs stay on the device; the records and count
        arrays are read back (that waits).  include/smmc.h states the arithmetic."""
        self._excursion_wants(wants)
        raw = self.simulate_excursions_raw(sim, lower, target, drawdown_threshold, **wants)
        res = ExcursionResult(int(sim.n_paths), int(sim.n_periods),
                              **{k: raw[k] for k in _lib.EXCURSION_OUTPUTS[:8]})
        return self._read_back(res, sim, raw, _EXCURSION_ROWS, ranges={"drawdown_stats": (0.0, 1.0)})

    def simulate_excursions_raw(self, sim, lower, target, drawdown_threshold=0.2, **wants):
        """Enqueues the call and returns its device tensors without waiting: a dict keyed by the fields of
        smmc_excursion_outputs -- float32 / int32 (holding uint32 values) [n_paths], uint8 packed records, int64
        (holding uint64 counts) [n_periods + 1]; None for what was not asked for."""
        out, o = self._outputs(_EXCURSION_ROWS, _lib.ExcursionOutputs, sim, self._excursion_wants(wants), host=False)
        x = self.make_excursions(lower, target, drawdown_threshold)
        self._run(self._L.smmc_engine_simulate_excursions, C.byref(sim), C.byref(x), C.byref(o), device=_buffers(_EXCURSION_ROWS, out))
        return out

    def simulate_excursions_to_host(self, sim, lower, target, drawdown_threshold=0.2, **wants):
        """The same through smmc_engine_simulate_excursions_to_host: a dict of numpy arrays (the records: bytes)."""
        out, o = self._outputs(_EXCURSION_ROWS, _lib.ExcursionOutputs, sim, self._excursion_wants(wants), host=True,
                               host_null_empty=True)  # this family alone passes a host array without elements as a null pointer
        x = self.make_excursions(lower, target, drawdown_threshold)
        self._run(self._L.smmc_engine_simulate_excursions_to_host, C.byref(sim), C.byref(x), C.byref(o))
        return _records_as_bytes(_EXCURSION_ROWS, out)

    # -- block bootstrap: table paths drawn in runs of consecutive months (smmc_engine_simulate_blocks) ----------
    @staticmethod
    def make_blocks(block_len, kind=_lib.BLOCKS_CIRCULAR):
        b = _lib.Blocks()
        b.struct_size, b.block_len, b.kind, b.reserved = C.sizeof(_lib.Blocks), int(block_len), kind, 0
        return b

    def simulate_blocks(self, sim, block_len, want_final=True, want_chunk_stats=False, want_stats=False, out=None):
        """simulate() with the circular block bootstrap: a path is built from runs of block_len consecutive entries
        of the returns table, each run starting where the table stream would have drawn a single month (table mode,
        counter stream v3; include/smmc.h states the draw).  block_len = 1 is simulate() bit for bit.  Returns the
        same SimResult of device tensors."""
        raw = self.simulate_blocks_raw(sim, block_len, want_final, want_chunk_stats, want_stats, out)
        res = SimResult()
        res.final, res.chunk_mean, res.chunk_var, res.stats_raw = (raw["final"], raw["chunk_mean"], raw["chunk_var"],
                                                                   raw["stats_raw"])
        return res

    def _check_out(self, final, sim):
        """A caller's `out` must hold the final values as the kernel writes them."""
        if final is not None:
            assert final.numel() >= int(sim.n_paths) and final.dtype == self._torch.float32 and final.is_contiguous()

    def simulate_blocks_raw(self, sim, block_len, want_final=True, want_chunk_stats=False, want_stats=False, out=None):
        """Enqueues the call and returns its device tensors without waiting: a dict with final, chunk_mean, chunk_var
        (float32) and stats_raw (uint8, the packed record); None for what was not asked for."""
        blocks = self.make_blocks(block_len)
        res, ptrs = self._outputs(_BLOCKS_ROWS, None, sim, (want_final, want_chunk_stats, want_chunk_stats, want_stats), host=False,
                                  given={"final": out})
        self._check_out(res["final"], sim)
        self._run(self._L.smmc_engine_simulate_blocks, C.byref(sim), C.byref(blocks), *ptrs, device=_buffers(_BLOCKS_ROWS, res))
        return res

    def simulate_blocks_to_host(self, sim, block_len, out=None, want_stats=False, want_chunk_stats=False, progress=None):
        """simulate_to_host() with block draws: (final, stats, (means, vars)) in host memory."""
        n = int(sim.n_paths)
        blocks = self.make_blocks(block_len)
        host = out if out is not None else np.empty(n, dtype=np.float32)
        assert host.dtype == np.float32 and host.size >= n and host.flags.c_contiguous
        st = _lib.Stats()
        hist = np.zeros(max(int(sim.n_bins), 1), dtype=np.uint64)
        nc = (n + _lib.CHUNK - 1) // _lib.CHUNK
        cm = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
        cv = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        self._enter()  # synchronous: returns with both of its streams drained
        _lib.check(self._L.smmc_engine_simulate_blocks_to_host(
            self._h, C.byref(sim), C.byref(blocks), vp(host), vp(cm), vp(cv),
            C.byref(progress) if progress is not None else None, C.byref(st) if want_stats else None,
            vp(hist) if want_stats else None))
        stats = None
        if want_stats:
            stats = Stats(st.count, st.below, st.underflow, st.overflow, st.sum, st.sumsq, st.min, st.max,
                          hist[: int(sim.n_bins)])
        return host, stats, (cm, cv)

    def blocks_divide_kind(self, sim, block_len):
        """DIV_FAST / DIV_EXACT / DIV_CHECKED: the divide simulate_blocks uses for this request (results never depend
        on it)."""
        blocks = self.make_blocks(block_len)
        return self._kind(self._L.smmc_engine_blocks_divide_kind(self._h, C.byref(sim), C.byref(blocks)))

    # -- portfolios: jointly drawn assets, weights, periodic rebalancing (smmc_engine_simulate_portfolio) -----
    def set_asset_table(self, returns_percent):
        """The joint table of table-mode portfolios: returns[T, K] in percent, one row per month, one column per asset."""
        t = np.ascontiguousarray(returns_percent, dtype=np.float32)
        if t.ndim != 2:
            raise ValueError("the asset table has shape (rows, assets)")
        self._enter()
        _lib.check(self._L.smmc_engine_set_asset_table(self._h, t.ctypes.data_as(C.c_void_p), t.shape[0], t.shape[1]))

    @staticmethod
    def make_portfolio(weights, rebalance_every=0, means=None, factor=None):
        """smmc_portfolio of K = len(weights) assets; means [K] and factor [K, K] (lower triangular) in Gaussian mode."""
        w = np.asarray(weights, dtype=np.float32).ravel()
        K = int(w.size)
        if not 1 <= K <= _lib.MAX_ASSETS:
            raise ValueError(f"1 .. {_lib.MAX_ASSETS} assets")
        pf = _lib.Portfolio()
        pf.struct_size = C.sizeof(_lib.Portfolio)
        pf.n_assets, pf.rebalance_every = K, int(rebalance_every)
        for k in range(K):
            pf.weights[k] = float(w[k])
        if means is not None:
            m = np.asarray(means, dtype=np.float32).ravel()
            if m.size != K:
                raise ValueError("means must hold one entry per asset")
            for k in range(K):
                pf.means[k] = float(m[k])
        if factor is not None:
            f = np.asarray(factor, dtype=np.float32)
            if f.shape != (K, K):
                raise ValueError("factor must be K x K")
            for k in range(K):
                for j in range(K):
                    pf.factor[k * _lib.MAX_ASSETS + j] = float(f[k, j])
        return pf

    def simulate_portfolio(self, sim, weights, rebalance_every=0, means=None, factor=None, want_final=True,
                           want_holdings=False, want_stats=False, out=None):
        """One simulation of a portfolio of K = len(weights) assets drawn jointly -- table mode: the rows of
        set_asset_table; Gaussian mode: normals with the given means and Cholesky factor (cholesky_factor) -- held with
        `weights` and rebalanced to them every `rebalance_every` periods (0: never).  Returns a PortfolioResult; final
        and holdings stay on the device, stats is read back (that waits).  include/smmc.h states the arithmetic."""
        raw = self.simulate_portfolio_raw(sim, weights, rebalance_every, means, factor, want_final, want_holdings,
                                          want_stats, out)
        res = PortfolioResult(int(sim.n_paths), raw["n_assets"], raw["final"], raw["holdings"])
        return self._read_back(res, sim, raw, _PORTFOLIO_ROWS)

    def simulate_portfolio_raw(self, sim, weights, rebalance_every=0, means=None, factor=None, want_final=True,
                               want_holdings=False, want_stats=False, out=None):
        """Enqueues the call and returns its device tensors without waiting: a dict with final, holdings (float32) and
        stats_raw (uint8, the packed record); None for what was not asked for."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        K = int(pf.n_assets)
        res, o = self._outputs(_PORTFOLIO_ROWS, _lib.PortfolioOutputs, sim, (want_final, want_holdings, want_stats), host=False, K=K,
                               head={"n_assets": K}, given={"final": out})
        self._check_out(res["final"], sim)
        self._run(self._L.smmc_engine_simulate_portfolio, C.byref(sim), C.byref(pf), C.byref(o), device=_buffers(_PORTFOLIO_ROWS, res))
        return res

    def simulate_portfolio_to_host(self, sim, weights, rebalance_every=0, means=None, factor=None, want_final=True,
                                   want_holdings=False, want_stats=False):
        """The same through smmc_engine_simulate_portfolio_to_host: a dict of numpy arrays (stats_raw: bytes)."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        K = int(pf.n_assets)
        res, o = self._outputs(_PORTFOLIO_ROWS, _lib.PortfolioOutputs, sim, (want_final, want_holdings, want_stats), host=True, K=K,
                               head={"n_assets": K})
        self._run(self._L.smmc_engine_simulate_portfolio_to_host, C.byref(sim), C.byref(pf), C.byref(o))
        return _records_as_bytes(_PORTFOLIO_ROWS, res)

    def portfolio_divide_kind(self, sim, weights, rebalance_every=0, means=None, factor=None):
        """_lib.DIV_FAST or DIV_EXACT: the divide simulate_portfolio uses for this request (results never depend on it)."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        return self._kind(self._L.smmc_engine_portfolio_divide_kind(self._h, C.byref(sim), C.byref(pf)))

    # -- portfolio cash flows: a schedule on a rebalanced portfolio (smmc_engine_simulate_portfolio_cashflow) -----
    def _pfcf_outputs(self, sim, K, wants, host, S=None, struct=_lib.PortfolioCashflowOutputs, head=None):
        """smmc_portfolio_cashflow_outputs (or the sweep's structure of the same fields) for the entries that fill it:
        (result dict beginning with n_assets and `head`, the structure)."""
        return self._outputs(_PFCF_ROWS, struct, sim, wants, host, K=K, S=S, head=dict({"n_assets": int(K)}, **(head or {})))

    def simulate_portfolio_cashflow(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                    fractions=None, means=None, factor=None, want_final=True, want_holdings=False,
                                    want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """simulate_portfolio's portfolio with simulate_cashflow's schedule taken out of its value after every period: the
        flow settles at the target weights, a rebalance sets the holdings to the weights' shares of what is left, and a
        path whose value would not stay above `floor` is depleted.  Returns a PortfolioCashflowResult; per-path outputs
        stay on the device, stats and depleted_at are read back (that waits).  include/smmc.h states the arithmetic."""
        raw = self.simulate_portfolio_cashflow_raw(sim, weights, rebalance_every, amount, fraction, floor, amounts, fractions,
                                                   means, factor, want_final, want_holdings, want_paid, want_ruin_period,
                                                   want_stats, want_depleted_at)
        res = PortfolioCashflowResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                                      n_assets=raw["n_assets"], holdings=raw["holdings"])
        return self._read_back(res, sim, raw, _PFCF_ROWS)

    def simulate_portfolio_cashflow_raw(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0,
                                        amounts=None, fractions=None, means=None, factor=None, want_final=True,
                                        want_holdings=False, want_paid=False, want_ruin_period=False, want_stats=False,
                                        want_depleted_at=True):
        """Enqueues the call and returns its device tensors without waiting: a dict with final, holdings, paid (float32),
        ruin_period (int32 holding uint32 values), stats_raw (uint8, the packed record) and depleted_at (int64 holding
        uint64 counts, n_periods + 1); None for what was not asked for."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=False)
        self._run(self._L.smmc_engine_simulate_portfolio_cashflow, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(o),
                  device=_buffers(_PFCF_ROWS, res))
        del keep
        return res

    def simulate_portfolio_cashflow_to_host(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0,
                                            amounts=None, fractions=None, means=None, factor=None, want_final=True,
                                            want_holdings=False, want_paid=False, want_ruin_period=False, want_stats=False,
                                            want_depleted_at=True):
        """The same through smmc_engine_simulate_portfolio_cashflow_to_host: a dict of numpy arrays (stats_raw: bytes)."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=True)
        self._run(self._L.smmc_engine_simulate_portfolio_cashflow_to_host, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(o))
        del keep
        return _records_as_bytes(_PFCF_ROWS, res)

    def portfolio_cashflow_divide_kind(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                       fractions=None, means=None, factor=None):
        """_lib.DIV_FAST or DIV_EXACT: the divide simulate_portfolio_cashflow uses for this request (results never depend on it)."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)  # keep lives until the return
        return self._kind(self._L.smmc_engine_portfolio_cashflow_divide_kind(self._h, C.byref(sim), C.byref(pf), C.byref(cf)))

    # -- glide paths: target weights that change along a plan (smmc_engine_simulate_glide) ---------------------------
    @staticmethod
    def make_glide(changes):
        """smmc_glide from a list of (after, weights); returns (structure, what must stay alive while it is used).  The
        library checks the periods and the rows."""
        changes = list(changes or ())
        after = np.ascontiguousarray([int(a) for a, _ in changes], dtype=np.uint32)
        rows = np.zeros((len(changes), _lib.MAX_ASSETS), dtype=np.float32)
        for c, (_, w) in enumerate(changes):
            w = np.asarray(w, dtype=np.float32).ravel()
            if w.size > _lib.MAX_ASSETS:
                raise ValueError("a row of a glide path has at most %d weights" % _lib.MAX_ASSETS)
            rows[c, :w.size] = w
        gl = _lib.Glide()
        gl.struct_size = C.sizeof(_lib.Glide)
        gl.n_changes = len(changes)
        if changes:
            gl.after = after.ctypes.data_as(C.POINTER(C.c_uint32))
            gl.weights = rows.ctypes.data_as(C.POINTER(C.c_float))
        return gl, (after, rows)

    def simulate_glide(self, sim, weights, changes, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                       fractions=None, means=None, factor=None, want_final=True, want_holdings=False, want_paid=False,
                       want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """simulate_portfolio_cashflow with target weights that change along the plan: `changes` is a list of
        (after, weights), strictly increasing in `after` >= 1; every trade at the end of period t -- a rebalance or the
        settlement of the flow -- uses the row of the last change with after <= t, `weights` before the first.  A change
        does not trade by itself: put it on a rebalance period to reallocate right there.  glide_linear() makes the list of
        a straight-line glide.  Returns a PortfolioCashflowResult, so survival() works as there; include/smmc.h states
        the arithmetic."""
        raw = self.simulate_glide_raw(sim, weights, changes, rebalance_every, amount, fraction, floor, amounts, fractions, means,
                                      factor, want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at)
        res = PortfolioCashflowResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                                      n_assets=raw["n_assets"], holdings=raw["holdings"])
        return self._read_back(res, sim, raw, _PFCF_ROWS)

    def simulate_glide_raw(self, sim, weights, changes, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                           fractions=None, means=None, factor=None, want_final=True, want_holdings=False, want_paid=False,
                           want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """Enqueues the call and returns its device tensors without waiting: simulate_portfolio_cashflow_raw's dict."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        gl, keep_gl = self.make_glide(changes)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=False)
        self._run(self._L.smmc_engine_simulate_glide, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(gl), C.byref(o),
                  device=_buffers(_PFCF_ROWS, res))
        del keep, keep_gl
        return res

    def simulate_glide_to_host(self, sim, weights, changes, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                               fractions=None, means=None, factor=None, want_final=True, want_holdings=False, want_paid=False,
                               want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """The same through smmc_engine_simulate_glide_to_host: a dict of numpy arrays (stats_raw: bytes)."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        gl, keep_gl = self.make_glide(changes)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=True)
        self._run(self._L.smmc_engine_simulate_glide_to_host, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(gl), C.byref(o))
        del keep, keep_gl
        return _records_as_bytes(_PFCF_ROWS, res)

    def glide_divide_kind(self, sim, weights, changes, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                          fractions=None, means=None, factor=None):
        """_lib.DIV_FAST or DIV_EXACT: the divide simulate_glide uses for this request (results never depend on it)."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        gl, keep_gl = self.make_glide(changes)  # keep_gl and keep live until the return
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        return self._kind(self._L.smmc_engine_glide_divide_kind(self._h, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(gl)))

    # -- block-bootstrap plans: portfolio cash flows on runs of consecutive months (smmc_engine_simulate_portfolio_cashflow_blocks) --
    def simulate_portfolio_cashflow_blocks(self, sim, weights, block_len, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0,
                                           amounts=None, fractions=None, want_final=True, want_holdings=False, want_paid=False,
                                           want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """simulate_portfolio_cashflow on paths built from runs of block_len consecutive rows of set_asset_table's table, each
        run starting where the portfolio's table stream would have drawn a single row (table mode, counter stream v3): the
        circular block bootstrap, which keeps what lies between neighbouring months.  block_len = 1 is
        simulate_portfolio_cashflow bit for bit.  Returns the same PortfolioCashflowResult, so survival() works as there."""
        raw = self.simulate_portfolio_cashflow_blocks_raw(sim, weights, block_len, rebalance_every, amount, fraction, floor, amounts,
                                                          fractions, want_final, want_holdings, want_paid, want_ruin_period,
                                                          want_stats, want_depleted_at)
        res = PortfolioCashflowResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                                      n_assets=raw["n_assets"], holdings=raw["holdings"])
        return self._read_back(res, sim, raw, _PFCF_ROWS)

    def simulate_portfolio_cashflow_blocks_raw(self, sim, weights, block_len, rebalance_every=0, amount=0.0, fraction=0.0,
                                               floor=0.0, amounts=None, fractions=None, want_final=True, want_holdings=False,
                                               want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """Enqueues the call and returns its device tensors without waiting: simulate_portfolio_cashflow_raw's dict."""
        pf = self.make_portfolio(weights, rebalance_every)
        blocks = self.make_blocks(block_len)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=False)
        self._run(self._L.smmc_engine_simulate_portfolio_cashflow_blocks, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(blocks),
                  C.byref(o), device=_buffers(_PFCF_ROWS, res))
        del keep
        return res

    def simulate_portfolio_cashflow_blocks_to_host(self, sim, weights, block_len, rebalance_every=0, amount=0.0, fraction=0.0,
                                                   floor=0.0, amounts=None, fractions=None, want_final=True, want_holdings=False,
                                                   want_paid=False, want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """The same through smmc_engine_simulate_portfolio_cashflow_blocks_to_host: a dict of numpy arrays (stats_raw: bytes)."""
        pf = self.make_portfolio(weights, rebalance_every)
        blocks = self.make_blocks(block_len)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=True)
        self._run(self._L.smmc_engine_simulate_portfolio_cashflow_blocks_to_host, C.byref(sim), C.byref(pf), C.byref(cf),
                  C.byref(blocks), C.byref(o))
        del keep
        return _records_as_bytes(_PFCF_ROWS, res)

    def portfolio_cashflow_blocks_divide_kind(self, sim, weights, block_len, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0,
                                              amounts=None, fractions=None):
        """_lib.DIV_FAST or DIV_EXACT: what portfolio_cashflow_divide_kind says of the same plan (results never depend on it)."""
        pf = self.make_portfolio(weights, rebalance_every)
        blocks = self.make_blocks(block_len)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)  # keep lives until the return
        return self._kind(self._L.smmc_engine_portfolio_cashflow_blocks_divide_kind(self._h, C.byref(sim), C.byref(pf), C.byref(cf),
                                                                                   C.byref(blocks)))

    # -- guardrails: a withdrawal that a review rule adjusts per path (smmc_engine_simulate_guardrails) --------------
    @staticmethod
    def make_guardrails(amount, review_every=12, upper=float("inf"), lower=0.0, cut=0.9, raise_=1.1, index=1.0, amount_min=0.0,
                        amount_max=float("inf"), floor=0.0):
        """smmc_guardrails; the library checks the bounds."""
        gr = _lib.Guardrails()
        gr.struct_size = C.sizeof(_lib.Guardrails)
        gr.review_every = int(review_every)
        gr.amount, gr.index, gr.upper, gr.lower = float(amount), float(index), float(upper), float(lower)
        gr.cut, gr.raise_, gr.amount_min, gr.amount_max, gr.floor = float(cut), float(raise_), float(amount_min), float(amount_max), float(floor)
        return gr

    def simulate_guardrails(self, sim, weights, amount, review_every=12, upper=float("inf"), lower=0.0, cut=0.9, raise_=1.1, index=1.0,
                            amount_min=0.0, amount_max=float("inf"), floor=0.0, rebalance_every=0, means=None, factor=None,
                            want_final=True, want_holdings=False, want_paid=False, want_ruin_period=False, want_stats=False,
                            want_depleted_at=True, want_amount_last=True, want_amount_lowest=True, want_cuts=True, want_raises=True,
                            want_cuts_at=True, want_raises_at=True):
        """simulate_portfolio_cashflow with the constant amount `amount` that a review after every `review_every`-th
        period adjusts per path: multiplied by `index`, then by `cut` if it exceeds `upper` times the value left, else
        by `raise_` if it is below `lower` times it, and clamped to [amount_min, amount_max].  Returns a
        GuardrailsResult; per-path outputs stay on the device, stats and the three count arrays are read back (that
        waits).  include/smmc.h states the arithmetic."""
        raw = self.simulate_guardrails_raw(sim, weights, amount, review_every, upper, lower, cut, raise_, index, amount_min, amount_max,
                                           floor, rebalance_every, means, factor, want_final, want_holdings, want_paid,
                                           want_ruin_period, want_stats, want_depleted_at, want_amount_last, want_amount_lowest,
                                           want_cuts, want_raises, want_cuts_at, want_raises_at)
        res = GuardrailsResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                               n_assets=raw["n_assets"], holdings=raw["holdings"], amount_last=raw["amount_last"],
                               amount_lowest=raw["amount_lowest"], cuts=raw["cuts"], raises=raw["raises"])
        return self._read_back(res, sim, raw, _GUARDRAILS_ROWS)

    def simulate_guardrails_raw(self, sim, weights, amount, review_every=12, upper=float("inf"), lower=0.0, cut=0.9, raise_=1.1,
                                index=1.0, amount_min=0.0, amount_max=float("inf"), floor=0.0, rebalance_every=0, means=None,
                                factor=None, want_final=True, want_holdings=False, want_paid=False, want_ruin_period=False,
                                want_stats=False, want_depleted_at=True, want_amount_last=True, want_amount_lowest=True,
                                want_cuts=True, want_raises=True, want_cuts_at=True, want_raises_at=True):
        """Enqueues the call and returns its device tensors without waiting: a dict with final, holdings, paid,
        amount_last, amount_lowest (float32), ruin_period, cuts, raises (int32 holding uint32 values), stats_raw (uint8,
        the packed record) and depleted_at, cuts_at, raises_at (int64 holding uint64 counts, n_periods + 1); None for
        what was not asked for."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        gr = self.make_guardrails(amount, review_every, upper, lower, cut, raise_, index, amount_min, amount_max, floor)
        K = int(pf.n_assets)
        wants = (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at, want_amount_last,
                 want_amount_lowest, want_cuts, want_raises, want_cuts_at, want_raises_at)
        res, o = self._outputs(_GUARDRAILS_ROWS, _lib.GuardrailsOutputs, sim, wants, host=False, K=K, head={"n_assets": K})
        self._run(self._L.smmc_engine_simulate_guardrails, C.byref(sim), C.byref(pf), C.byref(gr), C.byref(o),
                  device=_buffers(_GUARDRAILS_ROWS, res))
        return res

    def simulate_guardrails_to_host(self, sim, weights, amount, review_every=12, upper=float("inf"), lower=0.0, cut=0.9, raise_=1.1,
                                    index=1.0, amount_min=0.0, amount_max=float("inf"), floor=0.0, rebalance_every=0, means=None,
                                    factor=None, want_final=True, want_holdings=False, want_paid=False, want_ruin_period=False,
                                    want_stats=False, want_depleted_at=True, want_amount_last=True, want_amount_lowest=True,
                                    want_cuts=True, want_raises=True, want_cuts_at=True, want_raises_at=True):
        """The same through smmc_engine_simulate_guardrails_to_host: a dict of numpy arrays (stats_raw: bytes)."""
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        gr = self.make_guardrails(amount, review_every, upper, lower, cut, raise_, index, amount_min, amount_max, floor)
        K = int(pf.n_assets)
        wants = (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at, want_amount_last,
                 want_amount_lowest, want_cuts, want_raises, want_cuts_at, want_raises_at)
        res, o = self._outputs(_GUARDRAILS_ROWS, _lib.GuardrailsOutputs, sim, wants, host=True, K=K, head={"n_assets": K})
        self._run(self._L.smmc_engine_simulate_guardrails_to_host, C.byref(sim), C.byref(pf), C.byref(gr), C.byref(o))
        return _records_as_bytes(_GUARDRAILS_ROWS, res)

    # -- portfolio cash-flow checkpoints: the plan's value distribution at chosen periods
    #    (smmc_engine_simulate_portfolio_cashflow_checkpoints) ---------------------------------------------------------
    @staticmethod
    def _checkpoint_periods(periods):
        per = np.ascontiguousarray([int(p) for p in periods], dtype=np.int64)
        if per.size and (per.min() < 0 or per.max() > 0xFFFFFFFF):
            raise ValueError("periods must be non-negative 32-bit integers")
        return per.astype(np.uint32)

    def simulate_portfolio_cashflow_checkpoints(self, sim, weights, periods, rebalance_every=0, amount=0.0, fraction=0.0,
                                                floor=0.0, amounts=None, fractions=None, means=None, factor=None,
                                                want_final=True, want_holdings=False, want_paid=False, want_ruin_period=False,
                                                want_stats=False, want_depleted_at=True):
        """simulate_portfolio_cashflow with the record of the paths' values after each of `periods` (strictly increasing
        integers in 1 .. n_periods, at most _lib.MAX_CHECKPOINTS; a depleted path counts as 0), in one launch.  Returns a
        PortfolioCashflowCheckpointsResult: its checkpoints carry sim's bucket range, fan(quantiles) draws the fan chart
        of the plan.  Per-path outputs stay on the device; the records are read back (that waits)."""
        raw = self.simulate_portfolio_cashflow_checkpoints_raw(sim, weights, periods, rebalance_every, amount, fraction, floor,
                                                               amounts, fractions, means, factor, want_final, want_holdings,
                                                               want_paid, want_ruin_period, want_stats, want_depleted_at)
        per = raw["periods"]
        res = PortfolioCashflowCheckpointsResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                                                 n_assets=raw["n_assets"], holdings=raw["holdings"], periods=per)
        return self._read_back(res, sim, raw, _PFCF_ROWS, also=[("checkpoints", "records_raw", _RECORD, per.size)])  # always something to read

    def simulate_portfolio_cashflow_checkpoints_raw(self, sim, weights, periods, rebalance_every=0, amount=0.0, fraction=0.0,
                                                    floor=0.0, amounts=None, fractions=None, means=None, factor=None,
                                                    want_final=True, want_holdings=False, want_paid=False,
                                                    want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """Enqueues the call and returns its device tensors without waiting: simulate_portfolio_cashflow_raw's dict with
        records_raw (uint8, n_checkpoints packed records) and periods (numpy uint32)."""
        per = self._checkpoint_periods(periods)
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        rec = int(self._L.smmc_stats_bytes(sim.n_bins))
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=False, head={"periods": per})
        records = self._new(_RECORD, (max(per.size, 1) * rec,), host=False)  # the library wants a buffer even without a period
        self._run(self._L.smmc_engine_simulate_portfolio_cashflow_checkpoints, C.byref(sim), C.byref(pf), C.byref(cf),
                  per.ctypes.data_as(C.c_void_p), per.size, C.byref(o), C.c_void_p(records.data_ptr()),
                  device=[records] + _buffers(_PFCF_ROWS, res))
        del keep
        res["records_raw"] = records[: per.size * rec]
        return res

    def simulate_portfolio_cashflow_checkpoints_to_host(self, sim, weights, periods, rebalance_every=0, amount=0.0, fraction=0.0,
                                                        floor=0.0, amounts=None, fractions=None, means=None, factor=None,
                                                        want_final=True, want_holdings=False, want_paid=False,
                                                        want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """The same through smmc_engine_simulate_portfolio_cashflow_checkpoints_to_host: a dict of numpy arrays (stats_raw
        and records_raw: bytes)."""
        per = self._checkpoint_periods(periods)
        pf = self.make_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        rec = int(self._L.smmc_stats_bytes(sim.n_bins))
        res, o = self._pfcf_outputs(sim, pf.n_assets, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=True, head={"periods": per})
        records = self._new(_RECORD, (max(per.size, 1) * rec,), host=True)
        self._run(self._L.smmc_engine_simulate_portfolio_cashflow_checkpoints_to_host, C.byref(sim), C.byref(pf), C.byref(cf),
                  per.ctypes.data_as(C.c_void_p), per.size, C.byref(o), records.ctypes.data_as(C.c_void_p))
        del keep
        res["records_raw"] = records.tobytes()[: per.size * rec]
        return _records_as_bytes(_PFCF_ROWS, res)

    # -- real cash flows: the schedule in money of period 0, inflation drawn jointly (smmc_engine_simulate_real_cashflow) --
    @staticmethod
    def make_real_portfolio(weights, rebalance_every=0, means=None, factor=None):
        """smmc_portfolio of K = len(weights) invested assets for the real cash-flow calls; means [K + 1] and factor
        [K + 1, K + 1] (lower triangular) describe the joint law in Gaussian mode, the last series being inflation."""
        w = np.asarray(weights, dtype=np.float32).ravel()
        K = int(w.size)
        if not 1 <= K <= _lib.MAX_ASSETS - 1:
            raise ValueError(f"1 .. {_lib.MAX_ASSETS - 1} invested assets: the law's last series is inflation")
        pf = Engine.make_portfolio(np.append(w, np.float32(0.0)), rebalance_every, means, factor)  # checks the law at K + 1
        pf.n_assets = K
        return pf

    def make_real_cashflow_outputs(self, sim, n_assets, want_final=True, want_final_real=True, want_index=False,
                                   want_holdings=False, want_paid=False, want_ruin_period=False, want_stats=False,
                                   want_depleted_at=True):
        """(smmc_real_cashflow_outputs, dict of the device tensors it points to) for a request of sim's size with
        n_assets invested assets; None for what was not asked for."""
        wants = (want_final, want_final_real, want_index, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at)
        res, o = self._outputs(_REAL_ROWS, _lib.RealCashflowOutputs, sim, wants, host=False, K=n_assets, head={"n_assets": int(n_assets)})
        return o, res

    def simulate_real_cashflow(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                               fractions=None, means=None, factor=None, want_final=True, want_final_real=True, want_index=False,
                               want_holdings=False, want_paid=False, want_ruin_period=False, want_stats=False,
                               want_depleted_at=True):
        """simulate_portfolio_cashflow with `amount` / `amounts` and `floor` in money of period 0: K = len(weights)
        invested assets and one more series of the joint law, inflation in percent per period -- the last column of
        set_asset_table's table, or the last entry of means [K + 1] and last row of factor [K + 1, K + 1] -- compound
        a price index per path that scales the period's amount and floor.  Returns a RealCashflowResult; per-path
        outputs stay on the device, stats (of final_real) and depleted_at are read back (that waits).  include/smmc.h
        states the arithmetic."""
        raw = self.simulate_real_cashflow_raw(sim, weights, rebalance_every, amount, fraction, floor, amounts, fractions, means,
                                              factor, want_final, want_final_real, want_index, want_holdings, want_paid,
                                              want_ruin_period, want_stats, want_depleted_at)
        res = RealCashflowResult(int(sim.n_paths), int(sim.n_periods), raw["final"], raw["paid"], raw["ruin_period"],
                                 n_assets=raw["n_assets"], holdings=raw["holdings"], final_real=raw["final_real"], index=raw["index"])
        return self._read_back(res, sim, raw, _REAL_ROWS)

    def simulate_real_cashflow_raw(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                   fractions=None, means=None, factor=None, want_final=True, want_final_real=True,
                                   want_index=False, want_holdings=False, want_paid=False, want_ruin_period=False,
                                   want_stats=False, want_depleted_at=True):
        """Enqueues the call and returns its device tensors without waiting: a dict with final, final_real, index,
        holdings, paid (float32), ruin_period (int32 holding uint32 values), stats_raw (uint8, the packed record of
        final_real) and depleted_at (int64 holding uint64 counts, n_periods + 1); None for what was not asked for."""
        pf = self.make_real_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        o, res = self.make_real_cashflow_outputs(sim, pf.n_assets, want_final, want_final_real, want_index, want_holdings,
                                                 want_paid, want_ruin_period, want_stats, want_depleted_at)
        self._run(self._L.smmc_engine_simulate_real_cashflow, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(o),
                  device=_buffers(_REAL_ROWS, res))
        del keep
        return res

    def simulate_real_cashflow_to_host(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                       fractions=None, means=None, factor=None, want_final=True, want_final_real=True,
                                       want_index=False, want_holdings=False, want_paid=False, want_ruin_period=False,
                                       want_stats=False, want_depleted_at=True):
        """The same through smmc_engine_simulate_real_cashflow_to_host: a dict of numpy arrays (stats_raw: bytes)."""
        pf = self.make_real_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)
        K = int(pf.n_assets)
        wants = (want_final, want_final_real, want_index, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at)
        res, o = self._outputs(_REAL_ROWS, _lib.RealCashflowOutputs, sim, wants, host=True, K=K, head={"n_assets": K})
        self._run(self._L.smmc_engine_simulate_real_cashflow_to_host, C.byref(sim), C.byref(pf), C.byref(cf), C.byref(o))
        del keep
        return _records_as_bytes(_REAL_ROWS, res)

    def real_cashflow_divide_kind(self, sim, weights, rebalance_every=0, amount=0.0, fraction=0.0, floor=0.0, amounts=None,
                                  fractions=None, means=None, factor=None):
        """_lib.DIV_FAST or DIV_EXACT: the divide simulate_real_cashflow uses for this request (results never depend on it)."""
        pf = self.make_real_portfolio(weights, rebalance_every, means, factor)
        cf, keep = self.make_cashflow(int(sim.n_periods), amount, fraction, amounts, fractions, floor)  # keep lives until the return
        return self._kind(self._L.smmc_engine_real_cashflow_divide_kind(self._h, C.byref(sim), C.byref(pf), C.byref(cf)))

    # -- allocation sweeps: up to MAX_SWEEP portfolio strategies on one set of draws (smmc_engine_simulate_allocation_sweep) --
    @staticmethod
    def make_allocation_sweep(weights, rebalance_every=0, amounts=0.0, fractions=0.0, floors=0.0, means=None, factor=None):
        """(array of smmc_portfolio, array of smmc_cashflow, weights float32 [S, K], rebalance_every uint32 [S], amounts,
        fractions, floors float32 [S]): `weights` is a list of S weight vectors of one length K; a scalar rebalance_every,
        amount, fraction or floor broadcasts over the scenarios, a list gives one value per scenario; means and factor
        (Gaussian mode) are the one joint law all scenarios share."""
        w = np.asarray(weights, dtype=np.float32)
        if w.ndim != 2 or not 1 <= w.shape[1] <= _lib.MAX_ASSETS:
            raise ValueError(f"weights must be a list of weight vectors of one length, 1 .. {_lib.MAX_ASSETS} assets")
        S = int(w.shape[0])
        try:
            every, am, fr, fl = (np.broadcast_to(np.asarray(x, dtype=t), (S,)).copy() for x, t in
                                 ((rebalance_every, np.uint32), (amounts, np.float32), (fractions, np.float32), (floors, np.float32)))
        except ValueError:
            raise ValueError("rebalance_every, amounts, fractions and floors must be scalars or hold one value per scenario") from None
        pfs, cfs = (_lib.Portfolio * max(S, 1))(), (_lib.Cashflow * max(S, 1))()
        for s in range(S):
            pfs[s] = Engine.make_portfolio(w[s], int(every[s]), means, factor)
            cfs[s].struct_size = C.sizeof(_lib.Cashflow)
            cfs[s].amount, cfs[s].fraction, cfs[s].floor = float(am[s]), float(fr[s]), float(fl[s])
        return pfs, cfs, w.copy(), every, am, fr, fl

    def simulate_allocation_sweep(self, sim, weights, rebalance_every=0, amounts=0.0, fractions=0.0, floors=0.0, means=None,
                                  factor=None, want_final=False, want_holdings=False, want_paid=False, want_ruin_period=False,
                                  want_stats=False, want_depleted_at=True):
        """Up to MAX_SWEEP portfolio strategies on the SAME jointly drawn paths in one launch: scenario s holds weights[s],
        rebalances every rebalance_every[s] periods, takes amounts[s] + fractions[s] * value out after every period and is
        depleted at floors[s], exactly as simulate_portfolio_cashflow with those five.  Returns an AllocationSweepResult;
        per-path outputs stay on the device, stats and depleted_at are read back (that waits).  include/smmc.h states the
        contract."""
        raw = self.simulate_allocation_sweep_raw(sim, weights, rebalance_every, amounts, fractions, floors, means, factor,
                                                 want_final, want_holdings, want_paid, want_ruin_period, want_stats,
                                                 want_depleted_at)
        _, _, w, every, am, fr, fl = self.make_allocation_sweep(weights, rebalance_every, amounts, fractions, floors, means, factor)
        res = AllocationSweepResult(int(sim.n_paths), int(sim.n_periods), am, fr, fl, raw["final"], raw["paid"], raw["ruin_period"],
                                    weights=w, rebalance_every=every, n_assets=raw["n_assets"], holdings=raw["holdings"])
        return self._read_back(res, sim, raw, _PFCF_ROWS, n_records=am.size)

    def simulate_allocation_sweep_raw(self, sim, weights, rebalance_every=0, amounts=0.0, fractions=0.0, floors=0.0, means=None,
                                      factor=None, want_final=False, want_holdings=False, want_paid=False,
                                      want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """Enqueues the sweep and returns its device tensors without waiting: a dict with final, paid (float32
        [S, n_paths]), holdings (float32 [S, K, n_paths]), ruin_period (int32 holding uint32 values), stats_raw (uint8
        [S, smmc_stats_bytes(n_bins)]) and depleted_at (int64 holding uint64 counts, [S, n_periods + 1]); None for what
        was not asked for."""
        pfs, cfs, w, _, _, _, _ = self.make_allocation_sweep(weights, rebalance_every, amounts, fractions, floors, means, factor)
        S, K = w.shape
        res, o = self._pfcf_outputs(sim, K, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=False, S=S, struct=_lib.AllocationSweepOutputs)
        self._run(self._L.smmc_engine_simulate_allocation_sweep, C.byref(sim), pfs, cfs, S, C.byref(o), device=_buffers(_PFCF_ROWS, res))
        return res

    def simulate_allocation_sweep_to_host(self, sim, weights, rebalance_every=0, amounts=0.0, fractions=0.0, floors=0.0,
                                          means=None, factor=None, want_final=False, want_holdings=False, want_paid=False,
                                          want_ruin_period=False, want_stats=False, want_depleted_at=True):
        """The same through smmc_engine_simulate_allocation_sweep_to_host: a dict of numpy arrays, scenario-major
        (stats_raw: the S packed records as bytes)."""
        pfs, cfs, w, _, _, _, _ = self.make_allocation_sweep(weights, rebalance_every, amounts, fractions, floors, means, factor)
        S, K = w.shape
        res, o = self._pfcf_outputs(sim, K, (want_final, want_holdings, want_paid, want_ruin_period, want_stats, want_depleted_at),
                                    host=True, S=S, struct=_lib.AllocationSweepOutputs)
        self._run(self._L.smmc_engine_simulate_allocation_sweep_to_host, C.byref(sim), pfs, cfs, S, C.byref(o))
        return _records_as_bytes(_PFCF_ROWS, res)

    def allocation_sweep_divide_kind(self, sim, weights, rebalance_every=0, amounts=0.0, fractions=0.0, floors=0.0, means=None,
                                     factor=None):
        """_lib.DIV_FAST or DIV_EXACT: the divide simulate_allocation_sweep uses for this request: FAST only if every
        scenario's own rule says so (results never depend on it)."""
        pfs, cfs, w, _, _, _, _ = self.make_allocation_sweep(weights, rebalance_every, amounts, fractions, floors, means, factor)
        return self._kind(self._L.smmc_engine_allocation_sweep_divide_kind(self._h, C.byref(sim), pfs, cfs, int(w.shape[0])))

    def read_stats(self, stats_raw):
        """Copies a device record to the host after the engine stream has drained."""
        self.sync()
        return stats_from_bytes(stats_raw.cpu().numpy().tobytes())

    def stream_handle(self):
        """The hipStream_t (as an int) launches currently go to."""
        raw = C.c_void_p()
        _lib.check(self._L.smmc_engine_get_stream(self._h, C.byref(raw)))
        return int(raw.value or 0)

    # -- statistics of values already in HBM ---------------------
    def _check_values(self, values):
        torch = self._torch
        if not (values.is_cuda and values.dtype == torch.float32 and values.is_contiguous() and values.dim() == 1):
            raise ValueError("values must be a contiguous 1-D float32 tensor on the engine's device")

    def values_stats(self, values, below_threshold=1000.0, n_bins=0, hist_lo=0.0, hist_hi=1.0):
        """One HBM pass over a device tensor -> packed statistics record (device uint8 tensor)."""
        self._check_values(values)
        rec = self._torch.empty(int(self._L.smmc_stats_bytes(n_bins)), dtype=self._torch.uint8, device=self.tdevice)
        cur = self._enter()
        _lib.check(self._L.smmc_engine_values_stats(self._h, C.c_void_p(values.data_ptr()), values.numel(),
                                                    below_threshold, n_bins, hist_lo, hist_hi,
                                                    C.c_void_p(rec.data_ptr())))
        self._leave(cur, rec, values)
        return rec

    def order_statistics(self, values, ranks):
        """Exact k-th smallest values (0-based ranks) of a device tensor, unsorted input."""
        self._check_values(values)
        r = np.ascontiguousarray(ranks, dtype=np.uint64)
        out = np.empty(r.size, dtype=np.float32)
        self._leave(self._enter(), values)  # synchronous call: only the input needs ordering
        _lib.check(self._L.smmc_engine_order_statistics(self._h, C.c_void_p(values.data_ptr()), values.numel(),
                                                        r.ctypes.data_as(C.c_void_p), r.size,
                                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def quartiles(self, values):
        """{min, Q1, Q2, Q3, max}: update_quartiles, examples/visualize_returns_cpu_v2.cpp:83-111."""
        self._check_values(values)
        out = np.empty(5, dtype=np.float32)
        self._leave(self._enter(), values)
        _lib.check(self._L.smmc_engine_quartiles(self._h, C.c_void_p(values.data_ptr()), values.numel(),
                                                 out.ctypes.data_as(C.c_void_p)))
        return out

    def reduce_mean_host(self, host_values):
        v = np.ascontiguousarray(host_values, dtype=np.float32)
        mean, total = C.c_float(), C.c_double()
        _lib.check(self._L.smmc_engine_reduce_mean_host(self._h, v.ctypes.data_as(C.c_void_p), v.size,
                                                        C.byref(mean), C.byref(total)))
        return mean.value, total.value

    def divide_kind(self, sim, keepdata=False):
        """DIV_FAST / DIV_EXACT / DIV_CHECKED: which divide-by-100 a launch of `sim` uses (results
        never depend on it)."""
        return self._kind(self._L.smmc_engine_divide_kind(self._h, C.byref(sim), 1 if keepdata else 0))

    def paths_form(self, sim):
        """1 when a `simulate` launch of `sim` gets the kernel that holds the path id's bits 63..32 in a scalar
        register (every path of the launch shares them, counter stream v3, SMMC_UNIFORM_HI not 0), else 0
        (results never depend on it)."""
        self._uniform_hi_from_env()
        return self._kind(self._L.smmc_engine_paths_form(self._h, C.byref(sim)))

    def simulate_keepdata(self, sim, want_final=True):
        torch = self._torch
        n, p = int(sim.n_paths), int(sim.n_periods)
        traj = torch.empty((n, p + 1), dtype=torch.float32, device=self.tdevice)
        final = torch.empty(n, dtype=torch.float32, device=self.tdevice) if want_final else None
        if n:
            cur = self._enter()
            _lib.check(self._L.smmc_engine_simulate_keepdata(
                self._h, C.byref(sim), C.c_void_p(traj.data_ptr()),
                C.c_void_p(final.data_ptr()) if final is not None else None))
            self._leave(cur, traj, final)
        return traj, final

    def simulate_to_host(self, sim, out=None, want_stats=False, want_chunk_stats=False, progress=None):
        """Final values (and optionally per-256-path means/variances) straight into host
        memory: chunked, D2H overlapped with compute.  Returns (final, stats, (means, vars))."""
        n = int(sim.n_paths)
        host = out if out is not None else np.empty(n, dtype=np.float32)
        assert host.dtype == np.float32 and host.size >= n and host.flags.c_contiguous
        st = _lib.Stats()
        hist = np.zeros(max(int(sim.n_bins), 1), dtype=np.uint64)
        nc = (n + _lib.CHUNK - 1) // _lib.CHUNK
        cm = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
        cv = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        self._enter()  # synchronous: returns with both of its streams drained
        _lib.check(self._L.smmc_engine_simulate_to_host(
            self._h, C.byref(sim), vp(host), vp(cm), vp(cv), C.byref(progress) if progress is not None else None,
            C.byref(st) if want_stats else None, vp(hist) if want_stats else None))
        stats = None
        if want_stats:
            stats = Stats(st.count, st.below, st.underflow, st.overflow, st.sum, st.sumsq, st.min, st.max,
                          hist[: int(sim.n_bins)])
        return host, stats, (cm, cv)

    def simulate_keepdata_to_host(self, sim):
        n, p = int(sim.n_paths), int(sim.n_periods)
        traj = np.empty((n, p + 1), dtype=np.float32)
        final = np.empty(n, dtype=np.float32)
        self._enter()
        _lib.check(self._L.smmc_engine_simulate_keepdata_to_host(
            self._h, C.byref(sim), traj.ctypes.data_as(C.c_void_p), final.ctypes.data_as(C.c_void_p)))
        return traj, final


class Group:
    """Several devices of this process behind one call (smmc_group_*, include/smmc.h): the request is
    sharded by contiguous global path ids, every device streams its share to its place in the host
    arrays, and ONE merged statistics record comes back -- merged on the host in device order
    (merge="host") or by one RCCL all-reduce of the integer fields (merge="rccl", distinct devices).
    Reference: mc_simulations_multi_gpu_launcher_async, src/simulations.cu:576-655."""

    def __init__(self, devices, merge="host"):
        self._L = _lib.lib()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        kind = {"host": _lib.MERGE_HOST, "rccl": _lib.MERGE_RCCL}[merge]
        _lib.check(self._L.smmc_group_create(devs, len(devices), kind, C.byref(h)))
        self._h = h
        self.merge = merge

    def close(self):
        if getattr(self, "_h", None):
            self._L.smmc_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self._L.smmc_group_size(self._h))

    def set_table(self, returns_percent):
        t = np.ascontiguousarray(returns_percent, dtype=np.float32)
        _lib.check(self._L.smmc_group_set_table(self._h, t.ctypes.data_as(C.c_void_p), t.size))

    def shard(self, n_paths, index):
        first, count = C.c_uint64(), C.c_uint64()
        _lib.check(self._L.smmc_group_shard(self._h, n_paths, index, C.byref(first), C.byref(count)))
        return first.value, count.value

    def simulate(self, sim, out=None, want_final=True, want_stats=False, want_chunk_stats=False, progress=None):
        """Returns (final or None, Stats or None, (chunk means, chunk variances))."""
        n = int(sim.n_paths)
        host = None
        if want_final:
            host = out if out is not None else np.empty(n, dtype=np.float32)
            assert host.dtype == np.float32 and host.size >= n and host.flags.c_contiguous
        st = _lib.Stats()
        hist = np.zeros(max(int(sim.n_bins), 1), dtype=np.uint64)
        nc = (n + _lib.CHUNK - 1) // _lib.CHUNK
        cm = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
        cv = np.empty(nc, dtype=np.float32) if want_chunk_stats else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        _lib.check(self._L.smmc_group_simulate(
            self._h, C.byref(sim), vp(host), vp(cm), vp(cv), C.byref(progress) if progress is not None else None,
            C.byref(st) if want_stats else None, vp(hist) if want_stats else None))
        stats = None
        if want_stats:
            stats = Stats(st.count, st.below, st.underflow, st.overflow, st.sum, st.sumsq, st.min, st.max,
                          hist[: int(sim.n_bins)])
        return host, stats, (cm, cv)

    def device_record(self, index):
        """merge="rccl": device pointer (int) of device `index`'s copy of the merged packed record."""
        p = C.c_void_p()
        _lib.check(self._L.smmc_group_device_record(self._h, index, C.byref(p)))
        return int(p.value or 0)

    def timings(self):
        """(engines up, communicator init, merge step of the last simulate) in milliseconds."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _lib.check(self._L.smmc_group_timings(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value


# ---------------------------------------------------------------------------
# Reference-named functions (include/stock_market_monte_carlo/simulations.h)
# ---------------------------------------------------------------------------

_engines = {}


def _engine(device=0, lane=0):
    """One engine per (device, lane); lane > 0 only when SMMC_DEVICE_MAP puts several shards of one
    call on the same device."""
    e = _engines.get((device, lane))
    if e is None:
        e = _engines[(device, lane)] = Engine(device)
    return e


def _device_map(n_gpus):
    """Shard g of an n_gpus-way call runs on device map[g]: g itself, or SMMC_DEVICE_MAP="0,0,1"
    (the same hook as the C++ layer's, csrc/smmc_dropin.cpp)."""
    import torch
    env = os.environ.get("SMMC_DEVICE_MAP")
    devs = [int(x) for x in env.split(",")][:n_gpus] if env else list(range(n_gpus))
    if len(devs) < n_gpus:
        raise ValueError("SMMC_DEVICE_MAP names fewer devices than n_gpus")
    have = torch.cuda.device_count()
    if n_gpus < 1 or any(d < 0 or d >= have for d in devs):
        raise ValueError(f"n_gpus={n_gpus} but {have} device(s) visible")
    return devs


def _seed(seed):
    # the reference seeds every path from std::random_device (src/simulations.cpp:245-246)
    return int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)


def update_fund(fund_value, period_return):
    """simulations.h:9, src/simulations.cpp:14-16."""
    return float(_lib.lib().smmc_update_fund(float(fund_value), float(period_return)))


def many_updates(fund_value, returns, n_periods):
    """simulations.h:11-13, src/simulations.cpp:24-39: n_periods + 1 values, [0] = fund_value."""
    r = np.ascontiguousarray(returns, dtype=np.float32)
    if r.size < n_periods:
        raise ValueError("returns holds fewer than n_periods entries")
    out = np.empty(n_periods + 1, dtype=np.float32)
    out[0] = np.float32(fund_value)
    _lib.lib().smmc_many_updates(r.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), n_periods)
    return out


def read_historical_returns(csv_fpath):
    """simulations.h:31, src/simulations.cpp:83-93: the `returns` column of a CSV, percent units.
    Rows whose cell is empty (first month of python/get_data.py:59 output) are skipped."""
    vals = []
    with open(csv_fpath) as f:
        header = [h.strip() for h in f.readline().rstrip("\r\n").split(",")]
        if "returns" not in header:
            raise ValueError(f"{csv_fpath}: no column named 'returns'")
        col = header.index("returns")
        for line in f:
            cells = line.rstrip("\r\n").split(",")
            if col < len(cells) and cells[col].strip() not in ("", "nan", "NaN"):
                vals.append(np.float32(cells[col]))
    return np.array(vals, dtype=np.float32)


_groups = {}


def _group(devices):
    """One cached Group (smmc_group_*, host merge) per device list, like the C++ layer's."""
    key = tuple(devices)
    g = _groups.get(key)
    if g is None:
        g = _groups[key] = Group(list(devices))
    return g


def mc_simulations_gpu(max_n_simulations, n_periods, initial_capital, returns, n_gpus=1, seed=None, stream=3):
    """simulations.h:73-79, src/simulations.cu:661-680: final value of every path (host array).
    stream: 3 (default) / 2 the build's counter streams; "ref" the reference CPU engine's own stream --
    path id draws from mt19937(seed + id) through libstdc++'s uniform_int_distribution.
    Paths shard over n_gpus devices of this process by contiguous global id ranges through the C entry
    for several devices (smmc_group_simulate: one host thread per device, so that all devices compute and
    copy at once -- the reference's async launcher, src/simulations.cu:599-626; the N mod G remainder is
    kept).  SMMC_DEVICE_MAP="0,0,1" places shard g on device map[g]."""
    devs = _device_map(n_gpus)
    n = int(max_n_simulations)
    g = _group(devs)
    g.set_table(returns)
    sim = Engine.make_sim(n, n_periods, MODE_TABLE, _seed(seed), initial_capital=initial_capital, stream=stream)
    out, _, _ = g.simulate(sim)
    return out


def mc_simulations(max_n_simulations, n_periods, initial_capital, historical_returns, final_values=None, seed=None,
                   stream=3):
    """simulations.h:49-54, src/simulations.cpp:204-266 (the CPU v2 engine), run on the GPU.
    With stream="ref" and seed=s the result is, bit for bit, what that engine computes when the
    std::random_device of path id returns s + id (src/simulations.cpp:245-246).
    final_values, if given, must be pre-sized like the reference's caller does
    (examples/benchmark_mc_cpu_v2.cpp:26) and is filled in place."""
    n = int(max_n_simulations)
    if final_values is not None and (final_values.size < n or final_values.dtype != np.float32):
        raise ValueError("final_values must be a float32 array of at least max_n_simulations entries")
    e = _engine(0)
    e.set_table(historical_returns)
    sim = Engine.make_sim(n, n_periods, MODE_TABLE, _seed(seed), initial_capital=initial_capital, stream=stream)
    out, _, _ = e.simulate_to_host(sim, out=final_values)
    return out[:n]


def mc_simulations_gpu_reduceBlock(max_n_simulations, n_periods, initial_capital, returns, n_gpus=1, seed=None):
    """simulations.h:81-88, src/simulations.cu:682-697: (means, variances), one pair per 256 paths."""
    if n_gpus != 1:
        # src/simulations.cu:693 throws std::invalid_argument
        raise ValueError("mc_simulations_gpu_reduceBlock supports n_gpus == 1 only")
    e = _engine(0)
    e.set_table(returns)
    sim = Engine.make_sim(int(max_n_simulations), n_periods, MODE_TABLE, _seed(seed), initial_capital=initial_capital)
    r = e.simulate(sim, want_final=False, want_chunk_stats=True)
    e.sync()
    return r.chunk_mean.cpu().numpy(), r.chunk_var.cpu().numpy()


def mc_simulations_keepdata(max_n_simulations, n_periods, initial_capital, historical_returns, seed=None):
    """simulations.h:57-63, src/simulations.cpp:139-202: (mc_data [N, P+1], final_values)."""
    e = _engine(0)
    e.set_table(historical_returns)
    sim = Engine.make_sim(int(max_n_simulations), n_periods, MODE_TABLE, _seed(seed), initial_capital=initial_capital)
    return e.simulate_keepdata_to_host(sim)


def reduce_mean_gpu(vec, n=None):
    """simulations.h:71, src/simulations.cu:269-341: mean of the first n entries of a host array."""
    v = np.ascontiguousarray(vec, dtype=np.float32)
    n = v.size if n is None else int(n)
    return _engine(0).reduce_mean_host(v[:n])[0]


def vector_add_gpu(a, b):
    """out = a + b for two host float arrays on the MI355X (src/gpu.cu:17-47, include/.../gpu.h:2; the
    demo north_star names beside the engine).  Returns (out, seconds of the launch alone)."""
    x = np.ascontiguousarray(a, dtype=np.float32)
    y = np.ascontiguousarray(b, dtype=np.float32)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("vector_add_gpu takes two 1-D arrays of one length")
    out = np.empty_like(x)
    sec = C.c_double()
    _lib.check(_lib.lib().smmc_vector_add(out.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                          y.ctypes.data_as(C.c_void_p), x.size, C.byref(sec)))
    return out, sec.value


def _to_device(values, n_el):
    import torch
    v = np.ascontiguousarray(values, dtype=np.float32)[: int(n_el)]
    return torch.from_numpy(v).to(_engine(0).tdevice)


def update_quartiles(vec, n_el):
    """examples/visualize_returns_cpu_v2.cpp:83-111: [min, Q1, Q2, Q3, max] of vec[:n_el]."""
    return _engine(0).quartiles(_to_device(vec, n_el))


def update_mean_std(v, n_el):
    """examples/visualize_returns_cpu_v2.cpp:113-123: (mean, population std) as floats."""
    e = _engine(0)
    st = e.read_stats(e.values_stats(_to_device(v, n_el)))
    # variance from the DOUBLE mean, clamped, then rounded: with the float-rounded mean the error
    # 2 * mean * ulp(mean) swamps a small variance (the reference sums (v - mean)^2 instead)
    m = st.sum / n_el
    return float(np.float32(m)), float(np.float32(np.sqrt(max(st.sumsq / n_el - m * m, 0.0))))


def update_count_below_min(min_final_amount, final_values, n_simulations):
    """examples/visualize_returns_cpu_v2.cpp:125-138: count of final_values[:n] < min_final_amount."""
    e = _engine(0)
    return e.read_stats(e.values_stats(_to_device(final_values, n_simulations), below_threshold=min_final_amount)).below
