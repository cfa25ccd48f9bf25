"""The circular block bootstrap of include/smmc.h (smmc_engine_simulate_blocks) restated with numpy and the CPU
oracle: the reference of tests/test_blocks_cpu.py and tests/test_blocks_gpu.py.

Block b of a path starts at the table index the i.i.d. table stream draws for that path at period b
(oracle.counter_path_indices over ceil(P / L) periods); period t reads entry (s_{t div L} + t mod L) mod T; the step is
the oracle's update_fund (oracle.many_updates: three binary32 roundings per period).  Statistics come from
oracle.values_stats and oracle.chunk_mean_var over the final values."""
import functools

import numpy as np

f32 = np.float32
SEED = 0x5EED0123456789AB          # both halves non-zero
FIRST_PATH = (1 << 33) + 3         # path ids beyond 2^32
CAPITAL = 1000.0
BINS, LO, HI, BELOW = 64, 0.0, 4000.0, 900.0


def make_table(T):
    """A deterministic table of T monthly returns in percent, N(0.6, 4.3) clipped to +-30."""
    rng = np.random.default_rng(1000 + T)
    return np.clip(rng.normal(0.6, 4.3, T), -30.0, 30.0).astype(f32)


def redo_table():
    """Five months of +100 % then three of -50 %: with blocks of four, a third of the paths leave the checked window."""
    return np.array([100.0] * 5 + [-50.0] * 3, dtype=f32)


def starts(oracle, table, seed, path, n_blocks):
    """Table indices at which blocks 0 .. n_blocks - 1 of global path `path` begin."""
    p = oracle.make_params(oracle.MODE_TABLE, n_blocks, 1, seed, table=table)
    return oracle.counter_path_indices(p, path)


def indices(oracle, table, seed, path, n_periods, block_len):
    """Table index of every period of a path."""
    T = int(np.asarray(table).size)
    s = starts(oracle, table, seed, path, -(-n_periods // block_len)).astype(np.int64)
    t = np.arange(n_periods, dtype=np.int64)
    return ((s[t // block_len] + t % block_len) % T).astype(np.uint32)


def trajectory(oracle, table, seed, path, n_periods, block_len, capital=CAPITAL):
    """n_periods + 1 values of a path; [0] is the capital."""
    r = np.asarray(table, dtype=f32)[indices(oracle, table, seed, path, n_periods, block_len)]
    return oracle.many_updates(capital, r, n_periods)


def finals(oracle, table, seed, first_path, n_paths, n_periods, block_len, capital=CAPITAL):
    out = np.empty(n_paths, dtype=f32)
    with np.errstate(all="ignore"):
        for i in range(n_paths):
            out[i] = trajectory(oracle, table, seed, first_path + i, n_periods, block_len, capital)[n_periods]
    return out


def starts_bulk(oracle, table, seed, first_path, n_paths, n_blocks):
    """[n_paths, n_blocks] block starts of paths first_path ..: starts() of every path in one oracle call."""
    p = oracle.make_params(oracle.MODE_TABLE, n_blocks, n_paths, seed, first_path=first_path, table=table)
    return oracle.counter_indices(p).astype(np.int64)


def finals_bulk(oracle, table, seed, first_path, n_paths, n_periods, block_len, capital=CAPITAL):
    """finals() for many paths: starts_bulk and the oracle's update_fund as three numpy binary32 operations per
    period (100.0f + r, the product, the divide; numpy never fuses).  The first and last paths are compared with finals()."""
    table = np.asarray(table, dtype=f32)
    T = int(table.size)
    s = starts_bulk(oracle, table, seed, first_path, n_paths, -(-n_periods // block_len))
    v = np.full(n_paths, capital, f32)
    with np.errstate(all="ignore"):
        for t in range(n_periods):
            r = table[(s[:, t // block_len] + t % block_len) % T]
            v = (v * (f32(100.0) + r)) / f32(100.0)
    assert v.dtype == f32
    head, tail = min(n_paths, 8), max(n_paths - 8, 0)
    assert np.array_equal(v[:head].view(np.uint32), finals(oracle, table, seed, first_path, head, n_periods, block_len, capital).view(np.uint32))
    assert np.array_equal(v[tail:].view(np.uint32),
                          finals(oracle, table, seed, first_path + tail, n_paths - tail, n_periods, block_len, capital).view(np.uint32))
    return v


def result(oracle, table, n_paths, n_periods, block_len, seed=SEED, first_path=FIRST_PATH, capital=CAPITAL, n_bins=BINS,
           lo=LO, hi=HI, below=BELOW):
    """dict(final, stats, hist, chunk_mean, chunk_var) of one request."""
    final = finals(oracle, table, seed, first_path, n_paths, n_periods, block_len, capital)
    return record_of(oracle, final, n_bins, lo, hi, below)


def record_of(oracle, final, n_bins=BINS, lo=LO, hi=HI, below=BELOW):
    """result()'s dict for final values already computed (a prefix of a longer run's: paths do not depend on n_paths)."""
    n_paths = int(final.size)
    st, hist = oracle.values_stats(final, below, n_bins, lo, hi)
    if n_paths:
        cm, cv = oracle.chunk_mean_var(final)
    else:
        cm, cv = np.empty(0, f32), np.empty(0, f32)
    return {"final": final, "stats": st, "hist": hist, "chunk_mean": cm, "chunk_var": cv}


@functools.lru_cache(maxsize=None)
def _table(key):
    if key == "bundled":
        from conftest import load_table
        t = load_table()
    elif key == "extremes":  # the bundled months with the S&P 500's best and worst month put in, as tests/test_gpu_parity.py
        from conftest import load_table
        t = load_table().copy()
        t[7], t[100] = 42.2, -29.7
    elif key == "redo":
        t = redo_table()
    else:
        t = make_table(int(key))
    t.setflags(write=False)
    return t


def table_of(key):
    """'bundled' (the 1127 months of data/), 'extremes' (those with a +42.2 % and a -29.7 % month), 'redo', or a length: computed once, shared, read-only."""
    return _table(str(key))


@functools.lru_cache(maxsize=None)
def _cached(oracle, key, n_paths, n_periods, block_len, capital):
    out = result(oracle, table_of(key), n_paths, n_periods, block_len, capital=capital)
    for k in ("final", "hist", "chunk_mean", "chunk_var"):
        out[k].setflags(write=False)
    return out


def cached_result(oracle, key, n_paths, n_periods, block_len, capital=CAPITAL):
    """result() at the module's seed, first path and histogram: computed once per request and shared, never modified."""
    return _cached(oracle, str(key), n_paths, n_periods, block_len, capital)
