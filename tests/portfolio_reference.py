"""The portfolio contract of include/smmc.h (smmc_engine_simulate_portfolio) restated with numpy float32 over the CPU
oracle: the reference of tests/test_portfolio_cpu.py and tests/test_portfolio_gpu.py.

Table mode: the row of period t of a path is the index the table stream draws for it (oracle.counter_indices with a table of
n_rows entries); every asset reads that row.  Gaussian mode: asset j's standard normals of the periods 4b .. 4b + 3 are
what the oracle's v3 draw (oracle.multipliers_of_words with gauss_mean = -100, gauss_std = 1: scale 1, shift 0) makes of
the Philox block (b, id lo, id hi, 1 + 2 j) (oracle.philox4x32_10_bulk); the multiplier is the chain of fused
multiply-adds over L's row from s_k = fl(100 + mean_k).  Numpy has no fused multiply-add: fma32 below is one, and
tests/test_portfolio_cpu.py compares it with libm's fmaf.  The step is three numpy binary32 operations per asset and
period (numpy never fuses); the value is the left-to-right binary32 sum of the holdings."""
import functools

import numpy as np

f32 = np.float32
SEED = 0x5EED0123456789AB          # both halves non-zero
FIRST_PATH = (1 << 32) - 100       # the id crosses 2^32 inside every launch
CAPITAL = 1000.0
BINS, LO, HI, BELOW = 64, 0.0, 4000.0, 1000.0
WEIGHTS = {1: (1.0,), 2: (0.6, 0.4), 3: (0.5, 0.3, 0.2), 4: (0.4, 0.3, 0.2, 0.1)}
WEIGHTS_WITH_ZERO = {2: (0.0, 1.0), 3: (0.5, 0.0, 0.5), 4: (0.25, 0.5, 0.0, 0.25)}


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise over float32 arrays.  The product of two binary32 numbers is exact
    in binary64; adding c rounds once more (TwoSum gives the error of that sum exactly); where the error is not zero the
    binary64 sum is replaced by whichever of it and its neighbour towards the error has an odd last bit (rounding to odd
    keeps what the final rounding needs to know); the cast to binary32 then rounds as one fused operation would."""
    a, b, c = (np.asarray(x, dtype=f32) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        towards = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        even = (s.view(np.uint64) & np.uint64(1)) == 0 if s.ndim else (np.float64(s).view(np.uint64) & np.uint64(1)) == 0
        fix = np.isfinite(s) & (err != 0) & even
        return np.where(fix, towards, s).astype(f32)


def make_asset_table(T, K):
    """A deterministic table of T months x K assets, returns in percent: N(0.6, 4.3) clipped to +-30, columns mixed."""
    rng = np.random.default_rng(7000 + 10 * T + K)
    x = rng.normal(0.0, 1.0, (T, K))
    mix = np.eye(K) + 0.4 * np.tri(K, k=-1)
    return np.clip(0.6 + 4.3 * (x @ mix.T) / np.sqrt((mix ** 2).sum(axis=1)), -30.0, 30.0).astype(f32)


def row_indices(oracle, n_rows, seed, first_path, n_paths, n_periods):
    """[n_paths, n_periods] rows: the table stream's indices for a table of n_rows entries."""
    if n_periods == 0 or n_paths == 0:
        return np.zeros((n_paths, n_periods), dtype=np.int64)
    p = oracle.make_params(oracle.MODE_TABLE, n_periods, n_paths, seed, first_path=first_path, table=np.zeros(n_rows, f32))
    return oracle.counter_indices(p).astype(np.int64)


def table_multipliers(oracle, table, seed, first_path, n_paths, n_periods):
    """[n_paths, n_periods, K] multipliers a = 100.0f + r of the joint rows."""
    t = np.asarray(table, dtype=f32)
    assert t.ndim == 2
    a = f32(100.0) + t
    return a[row_indices(oracle, t.shape[0], seed, first_path, n_paths, n_periods)]


def standard_normals(oracle, K, seed, first_path, n_paths, n_periods):
    """[n_paths, n_periods, K] standard normals: asset j from the Philox blocks (b, id lo, id hi, 1 + 2 j)."""
    nb = -(-n_periods // 4)
    z = np.empty((n_paths, nb * 4, K), dtype=f32)
    if nb == 0 or n_paths == 0:
        return z[:, :n_periods]
    ids = np.uint64(first_path) + np.arange(n_paths, dtype=np.uint64)
    ctr = np.empty((n_paths, nb, 4), dtype=np.uint32)
    ctr[:, :, 0] = np.arange(nb, dtype=np.uint32)[None, :]
    ctr[:, :, 1] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[:, :, 2] = (ids >> np.uint64(32)).astype(np.uint32)[:, None]
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    unit = oracle.make_params(oracle.MODE_GAUSSIAN, 4, 1, seed, gauss_mean=-100.0, gauss_std=1.0)  # scale 1, shift 0
    for j in range(K):
        ctr[:, :, 3] = 1 + 2 * j
        words = oracle.philox4x32_10_bulk(ctr.reshape(-1, 4), key)
        z[:, :, j] = oracle.multipliers_of_words(unit, words).reshape(n_paths, nb * 4)
    return z[:, :n_periods]


def mix(z, means, factor):
    """a_k = fma(L[k][k], z_k, ... fma(L[k][0], z_0, s_k)), s_k = fl(100 + mean_k); z [n, ..., K] -> a [n, ..., K]."""
    z = np.asarray(z, dtype=f32)
    K = z.shape[-1]
    L = np.asarray(factor, dtype=f32).reshape(K, K)
    a = np.empty_like(z)
    for lo in range(0, z.shape[0], 1 << 15):  # in slices: fma32 works in binary64 temporaries
        zs = z[lo:lo + (1 << 15)]
        for k in range(K):
            acc = np.full(zs.shape[:-1], f32(100.0) + f32(means[k]), dtype=f32)
            for j in range(k + 1):
                acc = fma32(L[k, j], zs[..., j], acc)
            a[lo:lo + (1 << 15), ..., k] = acc
    return a


def gauss_multipliers(oracle, means, factor, seed, first_path, n_paths, n_periods):
    K = len(means)
    return mix(standard_normals(oracle, K, seed, first_path, n_paths, n_periods), means, factor)


def value(h):
    v = h[0]
    for x in h[1:]:
        v = v + x
    return v


def simulate(a, weights, rebalance_every, capital=CAPITAL):
    """a [n, P, K] multipliers -> (values [n, P + 1] with V_t in column t, final holdings [K, n])."""
    a = np.asarray(a, dtype=f32)
    n, P, K = a.shape
    w = np.asarray(weights, dtype=f32)
    assert w.size == K
    R = int(rebalance_every)
    with np.errstate(all="ignore"):
        h = [np.full(n, f32(capital) * w[k], dtype=f32) for k in range(K)]
        values = np.empty((n, P + 1), dtype=f32)
        values[:, 0] = value(h)
        for t in range(1, P + 1):
            h = [(h[k] * a[:, t - 1, k]) / f32(100.0) for k in range(K)]
            v = value(h)
            values[:, t] = v
            if R and t % R == 0 and t != P:  # the holdings a run of P periods ends with are those before a rebalance at P
                h = [v * w[k] for k in range(K)]
    assert all(x.dtype == f32 for x in h)
    return values, np.stack(h)


def gauss_setup(K):
    """(means, stds, correlation matrix) of the K-asset Gaussian cases: every pairwise entry non-zero."""
    means = [0.5, 0.2, 0.35, -0.1][:K]
    stds = [4.0, 1.5, 2.5, 6.0][:K]
    corr = np.array([[1.0, 0.6, -0.3, 0.2], [0.6, 1.0, 0.1, -0.25], [-0.3, 0.1, 1.0, 0.4], [0.2, -0.25, 0.4, 1.0]])[:K, :K]
    return means, stds, corr


def factor_of(stds, corr):
    sd = np.asarray(stds, dtype=np.float64)
    return np.linalg.cholesky(sd[:, None] * np.asarray(corr, dtype=np.float64) * sd[None, :]).astype(f32)


@functools.lru_cache(maxsize=None)
def _asset_table(T, K):
    t = make_asset_table(T, K)
    t.setflags(write=False)
    return t


def asset_table(T, K):
    """make_asset_table, computed once, shared, read-only."""
    return _asset_table(int(T), int(K))


@functools.lru_cache(maxsize=None)
def _multipliers(oracle, shape, K, n_paths, n_periods):
    if shape == "gauss":
        means, stds, corr = gauss_setup(K)
        a = gauss_multipliers(oracle, means, factor_of(stds, corr), SEED, FIRST_PATH, n_paths, n_periods)
    else:
        a = table_multipliers(oracle, asset_table(int(shape[1:]), K), SEED, FIRST_PATH, n_paths, n_periods)
    a.setflags(write=False)
    return a


def multipliers(oracle, shape, K, n_paths, n_periods):
    """[n_paths, n_periods, K] multipliers of shape 'gauss' or 't<rows>' at the module's seed and first path: computed
    once per request and shared, never modified.  A run of fewer periods or paths is a slice: the draws depend on
    neither."""
    return _multipliers(oracle, str(shape), int(K), int(n_paths), int(n_periods))
