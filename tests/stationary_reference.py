"""The stationary bootstrap of include/smmc.h (smmc_engine_simulate_stationary) restated with numpy over the CPU oracle:
the reference of tests/test_stationary_cpu.py and tests/test_stationary_gpu.py.

Candidate start c_t of period t is the index the i.i.d. table stream draws for that path at period t
(oracle.counter_indices over P periods); renewal field f_t is a 16-bit half of word (t % 8) / 2 of the Philox block
(t / 8, id lo, id hi, 2) with the launch's key (oracle.philox4x32_10_bulk); i_0 = c_0, i_t = c_t if f_t < q else
(i_{t-1} + 1) mod T; the step is update_fund as three numpy binary32 operations, the first and last paths re-done through
oracle.many_updates.  Statistics come from oracle.values_stats and oracle.chunk_mean_var (blocks_reference.record_of)."""
import functools

import numpy as np

import blocks_reference as bref

f32 = np.float32
SEED, FIRST_PATH, CAPITAL = bref.SEED, bref.FIRST_PATH, bref.CAPITAL
RENEW_TAG = 2          # fourth counter word of the renewal fields
ONE = 65536            # renew_q16 of probability 1
M64 = (1 << 64) - 1


def candidates(oracle, table, seed, first_path, n_paths, n_periods):
    """[n_paths, n_periods] candidate starts: the table stream's own indices."""
    if n_paths == 0 or n_periods == 0:
        return np.zeros((n_paths, n_periods), np.int64)
    p = oracle.make_params(oracle.MODE_TABLE, n_periods, n_paths, seed, first_path=first_path, table=table)
    return oracle.counter_indices(p).astype(np.int64)


def fields(oracle, seed, first_path, n_paths, n_periods):
    """[n_paths, n_periods] renewal fields, each in [0, 65536)."""
    n_blocks = -(-n_periods // 8)
    if n_paths == 0 or n_blocks == 0:
        return np.zeros((n_paths, n_periods), np.int64)
    with np.errstate(over="ignore"):
        ids = np.uint64(first_path & M64) + np.arange(n_paths, dtype=np.uint64)  # wraps at 2^64, as the ids do
    ctr = np.empty((n_paths, n_blocks, 4), np.uint32)
    ctr[:, :, 0] = np.arange(n_blocks, dtype=np.uint32)[None, :]
    ctr[:, :, 1] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[:, :, 2] = (ids >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[:, :, 3] = RENEW_TAG
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32)
    words = oracle.philox4x32_10_bulk(ctr.reshape(-1, 4), key).reshape(n_paths, n_blocks, 4).astype(np.int64)
    halves = np.stack([words & 0xFFFF, words >> 16], axis=-1)  # [path, block, word, half]: low half first
    return halves.reshape(n_paths, n_blocks * 8)[:, :n_periods]


def indices_bulk(oracle, table, seed, first_path, n_paths, n_periods, q):
    """[n_paths, n_periods] table index of every period of every path."""
    T = int(np.asarray(table).size)
    c = candidates(oracle, table, seed, first_path, n_paths, n_periods)
    f = fields(oracle, seed, first_path, n_paths, n_periods)
    idx = np.empty_like(c)
    for t in range(n_periods):
        idx[:, t] = c[:, t] if t == 0 else np.where(f[:, t] < q, c[:, t], (idx[:, t - 1] + 1) % T)
    return idx


def finals_bulk(oracle, table, seed, first_path, n_paths, n_periods, q, capital=CAPITAL):
    table = np.asarray(table, dtype=f32)
    idx = indices_bulk(oracle, table, seed, first_path, n_paths, n_periods, q)
    v = np.full(n_paths, capital, f32)
    with np.errstate(all="ignore"):
        for t in range(n_periods):
            v = (v * (f32(100.0) + table[idx[:, t]])) / f32(100.0)
        assert v.dtype == f32
        for i in sorted({0, n_paths - 1} if n_paths else ()):
            once = oracle.many_updates(capital, table[idx[i]], n_periods)[n_periods]
            assert f32(once).view(np.uint32) == v[i].view(np.uint32), (i, once, v[i])
    return v


def values_at_window_tests(oracle, table, seed, first_path, n_paths, n_periods, q, capital=CAPITAL):
    """[n_paths, n_periods // 8] values after periods 8, 16, ...: where the kernel tests SMMC_DIV_CHECKED's window."""
    table = np.asarray(table, dtype=f32)
    idx = indices_bulk(oracle, table, seed, first_path, n_paths, n_periods, q)
    v, out = np.full(n_paths, capital, f32), []
    with np.errstate(all="ignore"):
        for t in range(n_periods - n_periods % 8):
            v = (v * (f32(100.0) + table[idx[:, t]])) / f32(100.0)
            if t % 8 == 7:
                out.append(v)
    return np.stack(out, axis=1) if out else np.empty((n_paths, 0), f32)


def chunk_mean_var_device_order(values, chunk=256):
    """Chunk means and population variances with the kernels' own association, for a comparison as bits: one pass in
    binary64 over x and x * x, lanes beyond the end adding 0; per wave of 64 lanes the tree v[i] += v[i + off] for off = 32,
    16, .. 1; the four waves added in order; a full chunk scaled by 2^-8, the last ragged one divided by its length; the
    variance E[x^2] - mean^2 clamped at 0; each rounded to binary32 once."""
    v = np.asarray(values, dtype=f32).astype(np.float64)
    n = v.size
    nc = -(-n // chunk)
    x = np.zeros(nc * chunk)
    x[:n] = v
    sums = []
    with np.errstate(all="ignore"):
        for a in (x, x * x):
            w = a.reshape(nc, chunk // 64, 64)
            off = 32
            while off:
                w = w[:, :, :off] + w[:, :, off:2 * off]
                off //= 2
            w = w[:, :, 0]
            t = w[:, 0].copy()
            for k in range(1, chunk // 64):
                t = t + w[:, k]
            sums.append(t)
        length = np.full(nc, float(chunk))
        if n % chunk:
            length[-1] = float(n % chunk)
        full = length == chunk
        mean = np.where(full, sums[0] * 2.0 ** -8, sums[0] / length)
        var = np.where(full, sums[1] * 2.0 ** -8, sums[1] / length) - mean * mean
        return mean.astype(f32), np.where(var > 0.0, var, 0.0).astype(f32)


def result(oracle, table, n_paths, n_periods, q, seed=SEED, first_path=FIRST_PATH, capital=CAPITAL, n_bins=bref.BINS, lo=bref.LO,
           hi=bref.HI, below=bref.BELOW):
    """dict(final, stats, hist, chunk_mean, chunk_var) of one request."""
    return bref.record_of(oracle, finals_bulk(oracle, table, seed, first_path, n_paths, n_periods, q, capital), n_bins, lo, hi, below)


@functools.lru_cache(maxsize=None)
def _cached(oracle, key, n_paths, n_periods, q, capital):
    out = result(oracle, bref.table_of(key), n_paths, n_periods, q, capital=capital)
    for k in ("final", "hist", "chunk_mean", "chunk_var"):
        out[k].setflags(write=False)
    return out


def cached_result(oracle, key, n_paths, n_periods, q, capital=CAPITAL):
    """result() at the module's seed, first path and histogram: computed once per request and shared, never modified."""
    return _cached(oracle, str(key), n_paths, n_periods, q, capital)
