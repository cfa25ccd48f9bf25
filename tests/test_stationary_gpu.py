"""The stationary bootstrap (smmc_engine_simulate_stationary and its _to_host form, through
stock_market_monte_carlo_amd.stationary) on the GPU against the numpy restatement over the CPU oracle
(tests/stationary_reference.py).

Compared as bits: the final values; the chunk means and variances, against the restatement's one-pass sums in the
kernels' own association (stationary_reference.chunk_mean_var_device_order); the record's counters, minimum, maximum and
every bucket.  The record's two binary64 sums are added per lane, per wave, per workgroup and then over the launch's
workgroups, an order that follows the launch shape and that no restatement of the contract knows: they are held to the
relative 1e-12 of tests/test_gpu_parity.py here, and to their BYTES where the device itself is the reference -- the two
identities (q = 65536 against Engine.simulate, q = 0 against Engine.simulate_blocks with one block), which compare whole
records.  The oracle's own chunk statistics (oracle.chunk_mean_var, two passes) are looked at as well, at the 1e-6 / 1e-5
of tests/test_blocks_gpu.py, so that the one-pass restatement is itself held to an independent statement.

Shapes: 3 * 256 + 7 paths (three full chunks and a ragged one), ids from 2^33 + 3, both halves of the seed non-zero; run
lengths 1, 7, 8, 9 and 41 (one period, a remainder alone, a whole group of eight fields, one more, five groups and one);
tables of 1, 2, 7 and 37 entries (the wrap inside a group), the bundled 1127 and 2500 (four candidates per Philox block:
3, 4, 5, 12, 13 periods put the remainder on either side of the second candidate block); q = 0, 1, 1/12, 1/2, 65535 and
65536 (never, almost never, the typical use, a coin, almost always, always)."""
import contextlib

import numpy as np
import pytest

import blocks_reference as bref
import stationary_reference as ref

pytestmark = pytest.mark.gpu

N = 3 * 256 + 7
QS = (0, 1, 5461, 32768, 65535, 65536)
GRID = [(key, P) for key in ("1", "2", "7", "37", "bundled") for P in (1, 7, 8, 9, 41)] + [("2500", P) for P in (3, 4, 5, 12, 13)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engines():
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(key):
        if key not in made:
            made[key] = S.Engine(0)
            made[key].set_table(bref.table_of(key))
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _sim(n, P, first=ref.FIRST_PATH, exact_div=False, n_bins=bref.BINS, capital=ref.CAPITAL, seed=ref.SEED):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(n, P, S.MODE_TABLE, seed, first_path=first, initial_capital=capital, n_bins=n_bins, hist_lo=bref.LO,
                             hist_hi=bref.HI, below_threshold=bref.BELOW, exact_div=exact_div)


def _host(raw):
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in raw.items()}
    if out["stats_raw"] is not None:
        out["stats_raw"] = out["stats_raw"].tobytes()
    return out


def _run(eng, sim, q, final=True, chunks=True, stats=True):
    import stock_market_monte_carlo_amd as S
    raw = S.simulate_stationary_raw(eng, sim, renew_q16=q, want_final=final, want_chunk_stats=chunks, want_stats=stats)
    eng.sync()
    return _host(raw)


def _check(got, want, n, tag):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    if got["final"] is not None:
        assert got["final"].size == n and np.array_equal(_bits(got["final"]), _bits(want["final"])), tag
    if got["stats_raw"] is not None:
        st, ost = stats_from_bytes(got["stats_raw"]), want["stats"]
        assert st.count == ost.count == n, tag
        assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
        assert np.array_equal(st.hist, want["hist"]), tag
        if n:
            assert st.min == ost.min and st.max == ost.max, tag
        if np.isfinite(ost.sumsq):
            assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag
        else:
            assert st.sum == ost.sum and st.sumsq == ost.sumsq, tag
    if got["chunk_mean"] is not None:
        assert got["chunk_mean"].size == got["chunk_var"].size == -(-n // 256), tag
    if got["chunk_mean"] is not None and n:
        cm, cv = ref.chunk_mean_var_device_order(want["final"])
        assert np.array_equal(_bits(got["chunk_mean"]), _bits(cm)) and np.array_equal(_bits(got["chunk_var"]), _bits(cv)), tag
        if np.isfinite(want["final"]).all():
            assert np.allclose(cm, want["chunk_mean"], rtol=1e-6, atol=0.0), tag
            assert np.allclose(cv, want["chunk_var"], rtol=1e-5, atol=1e-6 * float(np.max(want["chunk_var"]) + 1)), tag


def _same_bytes(a, b, tag):
    """Two device results: every output, every byte."""
    assert np.array_equal(_bits(a["final"]), _bits(b["final"])), tag
    assert a["stats_raw"] == b["stats_raw"], tag
    assert np.array_equal(_bits(a["chunk_mean"]), _bits(b["chunk_mean"])) and np.array_equal(_bits(a["chunk_var"]), _bits(b["chunk_var"])), tag


@pytest.mark.parametrize("key,P", GRID)
def test_against_the_restatement(engines, oracle, key, P):
    for q in QS:
        _check(_run(engines(key), _sim(N, P), q), ref.cached_result(oracle, key, N, P, q), N, (key, P, q))


@pytest.mark.parametrize("n", [0, 1, 255])
def test_few_paths_and_none(engines, oracle, n):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    got = _run(engines("bundled"), _sim(n, 41), 5461)
    _check(got, ref.cached_result(oracle, "bundled", n, 41, 5461), n, n)
    assert stats_from_bytes(got["stats_raw"]).count == n and got["final"].size == n


def test_probability_one_is_simulate(engines):
    """q = 65536 against smmc_engine_simulate in table mode on the same engine: every output, every byte."""
    for key in ("bundled", "2500", "7"):
        eng, sim = engines(key), _sim(N, 41)
        r = eng.simulate(sim, want_final=True, want_chunk_stats=True, want_stats=True)
        eng.sync()
        plain = _host({"final": r.final, "chunk_mean": r.chunk_mean, "chunk_var": r.chunk_var, "stats_raw": r.stats_raw})
        _same_bytes(_run(eng, sim, 65536), plain, key)


def test_probability_zero_is_one_block(engines):
    """q = 0 against smmc_engine_simulate_blocks with block_len = n_periods on the same engine: every output, every byte."""
    for key in ("bundled", "2500", "7"):
        eng, sim = engines(key), _sim(N, 41)
        raw = eng.simulate_blocks_raw(sim, 41, want_final=True, want_chunk_stats=True, want_stats=True)
        eng.sync()
        _same_bytes(_run(eng, sim, 0), _host(raw), key)


# ---- the divides: each instantiation's divide is reached, and says so -----------------------------------------------

def _kind(eng, sim, q):
    import stock_market_monte_carlo_amd as S
    return S.stationary_divide_kind(eng, sim, renew_q16=q)


def test_fast_divide_on_a_calm_table(oracle):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import _lib
    calm = S.Engine(0)
    try:
        table = np.where(np.arange(64) % 3 == 0, -1.0, 1.0).astype(np.float32)
        calm.set_table(table)
        assert _kind(calm, _sim(N, 360), 5461) == _lib.DIV_FAST
        _check(_run(calm, _sim(N, 360), 5461), ref.result(oracle, table, N, 360, 5461), N, "fast")
    finally:
        calm.close()


def test_checked_and_exact_divide_with_the_extreme_months(engines, oracle):
    """The 1127 months with a +42.2 % and a -29.7 % month cannot be proven safe for the fast divide over 360 periods:
    CHECKED; the flag asks for EXACT; the same bits either way."""
    from stock_market_monte_carlo_amd import _lib
    eng = engines("extremes")
    assert _kind(eng, _sim(N, 360), 5461) == _lib.DIV_CHECKED
    assert _kind(eng, _sim(N, 360, exact_div=True), 5461) == _lib.DIV_EXACT
    assert _kind(engines("bundled"), _sim(N, 360), 5461) == _lib.DIV_FAST
    want = ref.cached_result(oracle, "extremes", N, 360, 5461)
    _check(_run(eng, _sim(N, 360), 5461), want, N, "checked")
    _check(_run(eng, _sim(N, 360, exact_div=True), 5461), want, N, "exact")


def test_redo_of_paths_that_leave_the_checked_window(engines, oracle):
    """Five +100 % and three -50 % months in runs of mean length 4 over 360 periods: CHECKED with the window
    [2^-81, 2^(126 - 7 - log2 200)] (divide_kind, smmc_capi.cpp: grow = shrink = 1 bit per period); part of the paths, not
    all, are outside it at one of the kernel's tests (after periods 8, 16, ...) and are redone with the IEEE divide."""
    from stock_market_monte_carlo_amd import _lib
    eng, n, q = engines("redo"), 2048, 16384
    sim = _sim(n, 360)
    assert _kind(eng, sim, q) == _lib.DIV_CHECKED
    lo, hi = np.float32(2.0 ** -81), np.float32(2.0 ** (126.0 - 7.0 - np.log2(200.0)))
    at = ref.values_at_window_tests(oracle, bref.table_of("redo"), ref.SEED, ref.FIRST_PATH, n, 360, q)
    left = (~((at > lo) & (at < hi))).any(axis=1)
    print(f"redo case: {left.mean():.3f} of the paths leave the window")
    assert 0.0 < left.mean() < 1.0
    want = ref.cached_result(oracle, "redo", n, 360, q)
    with np.errstate(all="ignore"):
        _check(_run(eng, sim, q), want, n, "redo")
        _check(_run(eng, _sim(n, 360, exact_div=True), q), want, n, "redo, exact")


# ---- the chunk walk --------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _one_block_per_cu(monkeypatch, table):
    """An engine whose grid is one workgroup per compute unit (the knob is read when the engine is made)."""
    import stock_market_monte_carlo_amd as S
    monkeypatch.setenv("SMMC_BLOCKS_PER_CU", "1")
    e = S.Engine(0)
    try:
        e.set_table(table)
        grid, _, cus = e.geometry()
        assert grid == cus  # host_enqueue_paths caps its grid at this
        yield e, cus
    finally:
        e.close()


def _several_chunks_sizes(vgrid):
    """tests/test_walk_trips_gpu.py's _blocks_sizes, restated: workgroup b walks the chunks b, b + vgrid, ...  With
    3 vgrid + 2 chunks workgroups 0 and 1 make a fourth trip, the second on a last chunk of 7 paths; with 2 vgrid - 1 the
    last workgroup is one trip short; with 2 vgrid - 2 + 1 the last is, and the one before it ends on a chunk of one path."""
    return [256 * (3 * vgrid + 1) + 7, 256 * (2 * vgrid - 1), 256 * (2 * vgrid - 2) + 1]


def test_when_workgroups_walk_several_chunks(oracle, monkeypatch):
    """The chunk walk and its alternating reduction slots under this walk: final values, record, chunk statistics."""
    with _one_block_per_cu(monkeypatch, bref.table_of("bundled")) as (eng, cus):
        sizes = _several_chunks_sizes(cus)
        final = ref.finals_bulk(oracle, bref.table_of("bundled"), ref.SEED, ref.FIRST_PATH, max(sizes), 97, 5461)
        for n in sizes:
            _check(_run(eng, _sim(n, 97), 5461), bref.record_of(oracle, final[:n]), n, n)


# ---- the host form, prefixes, fuzz -----------------------------------------------------------------------------------

def test_to_host_against_the_device_result(oracle, monkeypatch):
    """1000 paths through chunks of 256 into a pageable buffer: the device call's values, merged record and chunks."""
    import stock_market_monte_carlo_amd as S
    monkeypatch.setenv("SMMC_HOST_CHUNK_PATHS", "256")
    eng = S.Engine(0)  # the knobs are read when an engine is created
    try:
        eng.set_table(bref.table_of("bundled"))
        n, q, sim = 1000, 5461, _sim(1000, 41)
        dev = _run(eng, sim, q)
        host, st, (cm, cv) = S.simulate_stationary_to_host(eng, sim, renew_q16=q, out=np.full(n, -1.0, dtype=np.float32), want_stats=True,
                                                           want_chunk_stats=True)
        want = ref.cached_result(oracle, "bundled", n, 41, q)
        assert np.array_equal(_bits(host), _bits(dev["final"])) and np.array_equal(_bits(host), _bits(want["final"]))
        ost = want["stats"]
        assert (st.count, st.below, st.underflow, st.overflow) == (n, ost.below, ost.underflow, ost.overflow)
        assert st.min == ost.min and st.max == ost.max and np.array_equal(st.hist, want["hist"])
        assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12)
        # chunks of 256 paths are the chunk statistics' own groups: the device call's bits
        assert np.array_equal(_bits(cm), _bits(dev["chunk_mean"])) and np.array_equal(_bits(cv), _bits(dev["chunk_var"]))
        plain, none, (no_cm, no_cv) = S.simulate_stationary_to_host(eng, sim, mean_block_len=12)  # round(65536 / 12) = 5461
        assert none is None and no_cm is None and no_cv is None and np.array_equal(_bits(plain), _bits(host))
    finally:
        eng.close()


def test_the_first_paths_of_a_longer_run(engines):
    """A path does not depend on n_paths: the first n final values of a run of 1000 are the run of n."""
    eng = engines("bundled")
    whole = _run(eng, _sim(1000, 41), 5461, chunks=False, stats=False)["final"]
    for n in (1, 255, 300, 512):
        assert np.array_equal(_bits(_run(eng, _sim(n, 41), 5461, chunks=False, stats=False)["final"]), _bits(whole[:n])), n


def _fuzz_cases():
    rng = np.random.default_rng(0x57A7)
    out = []
    for i in range(24):
        q = int(rng.choice([int(rng.integers(0, 65537)), int(rng.integers(0, 65537)), 0, 65536, int(rng.integers(1, 64))]))
        T = int(rng.integers(1, 3001)) if i % 3 else int(rng.integers(2049, 3001))
        out.append(dict(q=q, T=T, P=int(rng.integers(1, 65)), n=int(rng.integers(1, 1501)),
                        seed=int(rng.integers(1, 1 << 63)) * 2 + int(rng.integers(0, 2)), first=int(rng.integers(0, 1 << 62)), table_seed=1000 + i))
    return out


FUZZ = _fuzz_cases()


@pytest.fixture(scope="module")
def fuzz_engine():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("c", FUZZ, ids=["q%d-T%d-P%d-n%d" % (c["q"], c["T"], c["P"], c["n"]) for c in FUZZ])
def test_seeded_fuzz(fuzz_engine, oracle, c):
    table = np.clip(np.random.default_rng(c["table_seed"]).normal(0.6, 4.3, c["T"]), -30.0, 30.0).astype(np.float32)
    fuzz_engine.set_table(table)
    want = ref.result(oracle, table, c["n"], c["P"], c["q"], seed=c["seed"], first_path=c["first"])
    _check(_run(fuzz_engine, _sim(c["n"], c["P"], first=c["first"], seed=c["seed"]), c["q"]), want, c["n"], c)


def test_refusals_on_the_device(engines):
    import stock_market_monte_carlo_amd as S
    eng = engines("bundled")
    with pytest.raises(S.SmmcError, match="SMMC_MODE_TABLE"):
        S.simulate_stationary(eng, S.Engine.make_sim(10, 5, S.MODE_GAUSSIAN, 1), renew_q16=100)
    with pytest.raises(S.SmmcError, match="V2"):
        S.simulate_stationary(eng, S.Engine.make_sim(10, 5, S.MODE_TABLE, 1, stream=2), renew_q16=100)
    with pytest.raises(ValueError):
        S.simulate_stationary(eng, _sim(10, 5), renew_q16=65537)
    with pytest.raises(ValueError):
        S.simulate_stationary(eng, _sim(10, 5))
