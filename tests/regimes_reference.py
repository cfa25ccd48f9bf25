"""Regime-switching Gaussian paths of include/smmc.h (smmc_engine_simulate_regimes) restated with numpy over the CPU
oracle: the reference of tests/test_regimes_cpu.py and tests/test_regimes_gpu.py.

z_t is portfolio_reference.standard_normals for one asset (the Philox block (t / 4, id lo, id hi, 1) through the oracle's v3
draw at scale 1, shift 0); field f_t is a 16-bit half of word (t % 8) / 2 of the Philox block (t / 8, id lo, id hi, 4) with
the launch's key (oracle.philox4x32_10_bulk, built as stationary_reference.fields builds its own with tag 2); s_0 = (f_0 <
start1_q16), s_t = s_{t-1} ^ (f_t < leave_q16[s_{t-1}]), a loop over t; the multiplier is portfolio_reference.fma32(std[s],
z, fl(100 + mean[s])), one rounding; the step is update_fund as three numpy binary32 operations, the first and last paths
re-done through oracle.many_updates.  Statistics come from oracle.values_stats and oracle.chunk_mean_var
(blocks_reference.record_of)."""
import functools

import numpy as np

import blocks_reference as bref
import portfolio_reference as pref

f32 = np.float32
SEED = pref.SEED                   # both halves non-zero
FIRST_PATH = pref.FIRST_PATH       # 2^32 - 100: the id crosses word 1 inside every launch
CAPITAL = 1000.0
BINS, LO, HI, BELOW = bref.BINS, bref.LO, bref.HI, bref.BELOW
REGIME_TAG = 4         # fourth counter word of the regime fields
ONE = 65536            # a q16 of probability 1
M64 = (1 << 64) - 1
MEANS, STDS = (0.9, -1.5), (3.5, 7.0)   # far enough apart that one wrong state changes the bits


def fields(oracle, seed, first_path, n_paths, n_periods, tag=REGIME_TAG):
    """[n_paths, n_periods] 16-bit fields of the Philox blocks (t / 8, id lo, id hi, tag), each in [0, 65536)."""
    n_blocks = -(-n_periods // 8)
    if n_paths == 0 or n_blocks == 0:
        return np.zeros((n_paths, n_periods), np.int64)
    with np.errstate(over="ignore"):
        ids = np.uint64(first_path & M64) + np.arange(n_paths, dtype=np.uint64)
    ctr = np.empty((n_paths, n_blocks, 4), np.uint32)
    ctr[:, :, 0] = np.arange(n_blocks, dtype=np.uint32)[None, :]
    ctr[:, :, 1] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[:, :, 2] = (ids >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[:, :, 3] = tag
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    words = oracle.philox4x32_10_bulk(ctr.reshape(-1, 4), key).reshape(n_paths, n_blocks, 4).astype(np.int64)
    halves = np.stack([words & 0xFFFF, words >> 16], axis=-1)  # [path, block, word, half]: low half first
    return halves.reshape(n_paths, n_blocks * 8)[:, :n_periods]


def states(oracle, seed, first_path, n_paths, n_periods, leave_q16, start1_q16):
    """[n_paths, n_periods] regime of every period of every path, 0 or 1."""
    f = fields(oracle, seed, first_path, n_paths, n_periods)
    leave = np.asarray(leave_q16, dtype=np.int64)
    s = np.empty((n_paths, n_periods), np.int64)
    for t in range(n_periods):
        s[:, t] = (f[:, t] < start1_q16) if t == 0 else s[:, t - 1] ^ (f[:, t] < leave[s[:, t - 1]])
    return s


def multipliers(oracle, seed, first_path, n_paths, n_periods, means, stds, leave_q16, start1_q16):
    """[n_paths, n_periods] a_t = fma(std[s_t], z_t, fl(100 + mean[s_t]))."""
    z = pref.standard_normals(oracle, 1, seed, first_path, n_paths, n_periods)[:, :, 0]
    s = states(oracle, seed, first_path, n_paths, n_periods, leave_q16, start1_q16)
    scale = np.asarray(stds, dtype=f32)[s]
    shift = (f32(100.0) + np.asarray(means, dtype=f32))[s]
    a = np.empty((n_paths, n_periods), f32)
    for lo in range(0, n_paths, 1 << 13):  # in slices: fma32 works in binary64 temporaries
        a[lo:lo + (1 << 13)] = pref.fma32(scale[lo:lo + (1 << 13)], z[lo:lo + (1 << 13)], shift[lo:lo + (1 << 13)])
    return a


def _compound(oracle, a, capital, tests_only=False):
    n_paths, n_periods = a.shape
    v, at = np.full(n_paths, capital, f32), []
    with np.errstate(all="ignore"):
        for t in range(n_periods - (n_periods % 8 if tests_only else 0)):
            v = (v * a[:, t]) / f32(100.0)
            if t % 8 == 7:
                at.append(v)
        assert v.dtype == f32
        if tests_only:
            return np.stack(at, axis=1) if at else np.empty((n_paths, 0), f32)
        for i in sorted({0, n_paths - 1} if n_paths else ()):
            # many_updates takes returns r and forms fl(100 + r): r = a - 100 is exact and gives a back for 50 <= a <= 200
            # (Sterbenz); a path with a multiplier outside is not re-done
            if n_periods and ((a[i] >= 50.0) & (a[i] <= 200.0)).all():
                once = oracle.many_updates(capital, a[i] - f32(100.0), n_periods)[n_periods]
                assert f32(once).view(np.uint32) == v[i].view(np.uint32), (i, once, v[i])
    return v


def finals_bulk(oracle, seed, first_path, n_paths, n_periods, means, stds, leave_q16, start1_q16, capital=CAPITAL):
    return _compound(oracle, multipliers(oracle, seed, first_path, n_paths, n_periods, means, stds, leave_q16, start1_q16), capital)


def values_at_window_tests(oracle, seed, first_path, n_paths, n_periods, means, stds, leave_q16, start1_q16, capital=CAPITAL):
    """[n_paths, n_periods // 8] values after periods 8, 16, ...: where the kernel tests SMMC_DIV_CHECKED's window."""
    a = multipliers(oracle, seed, first_path, n_paths, n_periods, means, stds, leave_q16, start1_q16)
    return _compound(oracle, a, capital, tests_only=True)


def result(oracle, n_paths, n_periods, leave_q16, start1_q16, means=MEANS, stds=STDS, seed=SEED, first_path=FIRST_PATH, capital=CAPITAL,
           n_bins=BINS, lo=LO, hi=HI, below=BELOW):
    """dict(final, stats, hist, chunk_mean, chunk_var) of one request."""
    final = finals_bulk(oracle, seed, first_path, n_paths, n_periods, means, stds, leave_q16, start1_q16, capital)
    return bref.record_of(oracle, final, n_bins, lo, hi, below)


@functools.lru_cache(maxsize=None)
def _cached(oracle, n_paths, n_periods, leave_q16, start1_q16, means, stds, capital):
    out = result(oracle, n_paths, n_periods, leave_q16, start1_q16, means, stds, capital=capital)
    for k in ("final", "hist", "chunk_mean", "chunk_var"):
        out[k].setflags(write=False)
    return out


def cached_result(oracle, n_paths, n_periods, leave_q16, start1_q16, means=MEANS, stds=STDS, capital=CAPITAL):
    """result() at the module's seed, first path and histogram: computed once per request and shared, never modified."""
    return _cached(oracle, n_paths, n_periods, tuple(leave_q16), int(start1_q16), tuple(means), tuple(stds), capital)


def stationary_start(leave_q16):
    """The chain's stationary share of regime 1, l0 / (l0 + l1), rounded to q16: what make_regimes takes for start=None."""
    l0, l1 = leave_q16
    return int(round(ONE * l0 / (l0 + l1)))
