"""Checkpoint statistics (smmc_engine_simulate_checkpoints) on the GPU against the CPU oracle.

Record k of a call is the record values_stats forms of column periods[k] of the trajectories keepdata writes for
the same request: the oracle's counter_mc(want_traj=True)["traj"][:, p] through the oracle's values_stats.  Integer
fields, min, max and bucket counts are compared with ==, the two double sums to the relative 1e-12 of
tests/test_gpu_parity.py (the device adds in another order).
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
FIB = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987]


def _big_table():
    """3001 entries: above the 2048 up to which a Philox block yields eight draws, so the four-draw form runs."""
    rng = np.random.default_rng(20240611)
    return rng.normal(0.6, 4.0, 3001).clip(-25.0, 25.0).astype(np.float32)


@pytest.fixture(scope="module")
def eng(table):
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    e.set_table(table)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_big():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    e.set_table(_big_table())
    yield e
    e.close()


def _mode(name):
    from stock_market_monte_carlo_amd import MODE_GAUSSIAN, MODE_TABLE
    return MODE_GAUSSIAN if name == "gaussian" else MODE_TABLE


def _sets(p):
    """The checkpoint sets of a path of p periods (at most 64 per call: SMMC_MAX_CHECKPOINTS)."""
    return {"yearly": list(range(12, p + 1, 12))[:64], "first": [1], "last": [p],
            "inside": [x for x in FIB if x <= p], "every": list(range(1, min(p, 64) + 1))}


def _same_sum(got, want):
    if math.isfinite(want):
        assert got == pytest.approx(want, rel=1e-12)
    else:
        assert (math.isnan(got) and math.isnan(want)) or got == want, (got, want)


def _check(oracle, stats, traj, periods, below, n_bins, lo, hi, what=None):
    assert len(stats) == len(periods)
    for st, p in zip(stats, periods):
        ost, ohist = oracle.values_stats(traj[:, p], below, n_bins, lo, hi)
        tag = (what, p)
        assert st.count == ost.count == traj.shape[0], tag
        assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
        assert st.min == ost.min and st.max == ost.max, tag
        assert len(st.hist) == n_bins and np.array_equal(st.hist, ohist), tag
        if n_bins:
            assert int(st.hist.sum()) + st.underflow + st.overflow == st.count, tag
        _same_sum(st.sum, ost.sum)
        _same_sum(st.sumsq, ost.sumsq)


_traj_cache = {}


def _oracle_traj(oracle, mode_name, tab, n, p, first=0, seed=SEED, cap=1000.0, mean=0.5, std=0.83333):
    key = (mode_name, None if tab is None else tab.tobytes(), n, p, first, seed, cap, mean, std)
    if key not in _traj_cache:
        _traj_cache.clear()  # one entry: the parametrisation keeps equal requests together
        op = oracle.make_params(_mode(mode_name), p, n, seed, first_path=first, initial_capital=cap, table=tab,
                                gauss_mean=mean, gauss_std=std)
        _traj_cache[key] = oracle.counter_mc(op, want_traj=True)
    return _traj_cache[key]


def _pick(eng, eng_big, table, mode_name):
    if mode_name == "table_big":
        return eng_big, _big_table()
    return eng, (table if mode_name == "table" else None)


@pytest.mark.parametrize("n_bins", [0, 100])
@pytest.mark.parametrize("set_name", ["yearly", "first", "last", "inside", "every"])
@pytest.mark.parametrize("n", [1, 255, 4099, 2 * 4099 + 1])
@pytest.mark.parametrize("p", [7, 360, 1000])
@pytest.mark.parametrize("mode_name", ["table", "table_big", "gaussian"])
def test_oracle_parity(eng, eng_big, oracle, table, mode_name, p, n, set_name, n_bins):
    from stock_market_monte_carlo_amd import Engine, SmmcError
    e, tab = _pick(eng, eng_big, table, mode_name)
    periods = _sets(p)[set_name]
    sim = Engine.make_sim(n, p, _mode(mode_name), SEED, first_path=3, n_bins=n_bins, hist_lo=0.0, hist_hi=20000.0,
                          below_threshold=1100.0)
    if not periods:  # no year ends inside 7 periods: an empty set is an argument error, not an empty answer
        with pytest.raises(SmmcError, match="n_checkpoints"):
            e.simulate_checkpoints(sim, periods)
        return
    stats, final = e.simulate_checkpoints(sim, periods, want_final=True)
    o = _oracle_traj(oracle, mode_name, tab, n, p, first=3)
    _check(oracle, stats, o["traj"], periods, 1100.0, n_bins, 0.0, 20000.0, (mode_name, p, n, set_name))
    assert np.array_equal(final.cpu().numpy().view(np.uint32), o["final"].view(np.uint32))


@pytest.mark.parametrize("mode_name", ["table", "gaussian"])
def test_path_ids_above_32_bits(eng, oracle, table, mode_name):
    from stock_market_monte_carlo_amd import Engine
    tab = table if mode_name == "table" else None
    for first in ((1 << 32) - 100, (1 << 40) + 12345):
        sim = Engine.make_sim(700, 36, _mode(mode_name), SEED, first_path=first, n_bins=100, hist_lo=500.0, hist_hi=2000.0)
        periods = [1, 7, 12, 24, 35, 36]
        stats, final = eng.simulate_checkpoints(sim, periods, want_final=True)
        o = _oracle_traj(oracle, mode_name, tab, 700, 36, first=first)
        _check(oracle, stats, o["traj"], periods, 1000.0, 100, 500.0, 2000.0, first)
        assert np.array_equal(final.cpu().numpy().view(np.uint32), o["final"].view(np.uint32))


@pytest.mark.parametrize("mode_name", ["table", "gaussian"])
def test_exact_divide_flag(eng, oracle, table, mode_name):
    from stock_market_monte_carlo_amd import Engine, _lib
    sim = Engine.make_sim(3000, 360, _mode(mode_name), SEED, n_bins=100, hist_lo=0.0, hist_hi=20000.0, exact_div=True)
    assert eng.divide_kind(sim, keepdata=True) == _lib.DIV_EXACT
    periods = _sets(360)["yearly"]
    stats, _ = eng.simulate_checkpoints(sim, periods)
    o = _oracle_traj(oracle, mode_name, table if mode_name == "table" else None, 3000, 360)
    _check(oracle, stats, o["traj"], periods, 1000.0, 100, 0.0, 20000.0)


def test_table_that_cannot_be_proven_safe_takes_the_ieee_divide(oracle, table):
    """The +42.2 / -29.7 % months of tests/test_gpu_parity.py: final-value launches run the checked divide, a
    checkpoint launch -- its values must be right when they are taken -- follows the keepdata rule."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import Engine, MODE_TABLE, _lib
    real = table.copy()
    real[7], real[100] = 42.2, -29.7
    e = S.Engine(0)
    try:
        e.set_table(real)
        sim = Engine.make_sim(20_000, 360, MODE_TABLE, SEED, n_bins=100, hist_lo=0.0, hist_hi=1.0e6)
        assert e.divide_kind(sim) == _lib.DIV_CHECKED
        assert e.divide_kind(sim, keepdata=True) == _lib.DIV_EXACT
        periods = sorted(_sets(360)["yearly"] + [355, 359])  # 348, 355, 359, 360: three in the last two blocks
        stats, final = e.simulate_checkpoints(sim, periods, want_final=True)
        o = _oracle_traj(oracle, "table", real, 20_000, 360)
        _check(oracle, stats, o["traj"], periods, 1000.0, 100, 0.0, 1.0e6)
        assert np.array_equal(final.cpu().numpy().view(np.uint32), o["final"].view(np.uint32))
    finally:
        e.close()


@pytest.mark.parametrize("mode_name, p", [("table", 360), ("table", 1000), ("gaussian", 360), ("gaussian", 7)])
def test_last_checkpoint_is_the_final_value_record(eng, table, mode_name, p):
    """A checkpoint at n_periods against smmc_engine_simulate's own record and final values."""
    from stock_market_monte_carlo_amd import Engine
    n = 100_003
    sim = Engine.make_sim(n, p, _mode(mode_name), 77, first_path=11, n_bins=100, hist_lo=0.0, hist_hi=20000.0)
    stats, final = eng.simulate_checkpoints(sim, [1, p], want_final=True)
    r = eng.simulate(sim, want_final=True, want_stats=True)
    w, st = eng.read_stats(r.stats_raw), stats[-1]
    assert (st.count, st.below, st.underflow, st.overflow) == (w.count, w.below, w.underflow, w.overflow)
    assert st.count == n and st.min == w.min and st.max == w.max and np.array_equal(st.hist, w.hist)
    assert st.sum == pytest.approx(w.sum, rel=1e-12) and st.sumsq == pytest.approx(w.sumsq, rel=1e-12)
    assert np.array_equal(final.cpu().numpy().view(np.uint32), r.final.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("mode_name", ["table", "gaussian"])
def test_against_keepdata_columns_on_the_device(eng, mode_name):
    """1e6 x 360, yearly, 100 buckets: every record against values_stats of the column keepdata wrote."""
    from stock_market_monte_carlo_amd import Engine
    n, p = 1_000_000, 360
    sim = Engine.make_sim(n, p, _mode(mode_name), SEED, n_bins=100, hist_lo=0.0, hist_hi=20000.0, below_threshold=1500.0)
    periods = list(range(12, p + 1, 12))
    stats, _ = eng.simulate_checkpoints(sim, periods)
    traj, _ = eng.simulate_keepdata(sim, want_final=False)
    for st, q in zip(stats, periods):
        w = eng.read_stats(eng.values_stats(traj[:, q].contiguous(), below_threshold=1500.0, n_bins=100, hist_lo=0.0,
                                            hist_hi=20000.0))
        assert (st.count, st.below, st.underflow, st.overflow) == (w.count, w.below, w.underflow, w.overflow), q
        assert st.count == n and st.min == w.min and st.max == w.max and np.array_equal(st.hist, w.hist), q
        assert st.sum == pytest.approx(w.sum, rel=1e-12) and st.sumsq == pytest.approx(w.sumsq, rel=1e-12)


@pytest.mark.parametrize("mode_name", ["table", "gaussian"])
def test_shards_merge_to_the_one_launch_records(eng, mode_name):
    from stock_market_monte_carlo_amd import Engine
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes, stats_from_bytes
    n, p, periods = 100_003, 48, [1, 5, 12, 24, 47, 48]
    kw = dict(n_bins=64, hist_lo=800.0, hist_hi=1500.0)
    rec = 64 + 8 * 64
    whole, _ = eng.simulate_checkpoints_raw(Engine.make_sim(n, p, _mode(mode_name), 99, first_path=5, **kw), periods)
    cuts = [0, 33_333, 33_334 + 511, n]  # no cut on a multiple of 256
    assert all(c % 256 for c in cuts[1:-1])
    parts = [eng.simulate_checkpoints_raw(Engine.make_sim(b - a, p, _mode(mode_name), 99, first_path=5 + a, **kw), periods)[0]
             for a, b in zip(cuts[:-1], cuts[1:])]
    for k in range(len(periods)):
        m = stats_from_bytes(merge_stats_bytes([x[k * rec:(k + 1) * rec] for x in parts]))
        w = stats_from_bytes(whole[k * rec:(k + 1) * rec])
        assert (m.count, m.below, m.underflow, m.overflow) == (w.count, w.below, w.underflow, w.overflow)
        assert m.count == n and m.min == w.min and m.max == w.max and np.array_equal(m.hist, w.hist)
        assert m.sum == pytest.approx(w.sum, rel=1e-12) and m.sumsq == pytest.approx(w.sumsq, rel=1e-12)


@pytest.mark.parametrize("mode_name", ["table", "gaussian"])
def test_identical_calls_give_identical_bytes(eng, mode_name):
    from stock_market_monte_carlo_amd import Engine
    periods = list(range(12, 361, 12))
    mk = lambda seed: Engine.make_sim(300_007, 360, _mode(mode_name), seed, n_bins=100, hist_lo=0.0, hist_hi=20000.0)  # noqa: E731
    a, _ = eng.simulate_checkpoints_raw(mk(5), periods)
    b, _ = eng.simulate_checkpoints_raw(mk(5), periods)
    c, _ = eng.simulate_checkpoints_raw(mk(6), periods)
    assert len(a) == 30 * 864 and a == b
    assert a != c


def test_histogram_budget_edge(eng, oracle, table):
    """The largest n_checkpoints * n_bins runs and is exact; one more bucket is an argument error."""
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN, MODE_TABLE, SmmcError, _lib
    assert _lib.MAX_CHECKPOINT_BINS >= 64 * 128 and _lib.MAX_CHECKPOINT_BINS >= 31 * 256
    for mode_name, k, n_bins in (("table", 64, _lib.MAX_CHECKPOINT_BINS // 64), ("gaussian", 64, _lib.MAX_CHECKPOINT_BINS // 64),
                                 ("gaussian", 31, _lib.MAX_CHECKPOINT_BINS // 31), ("table", 2, 4096)):
        periods = list(range(3, 3 + 5 * k, 5))
        assert k * n_bins <= _lib.MAX_CHECKPOINT_BINS < (k + 1) * n_bins or n_bins == 4096
        sim = Engine.make_sim(5000, 360, _mode(mode_name), SEED, n_bins=n_bins, hist_lo=500.0, hist_hi=6000.0)
        stats, _ = eng.simulate_checkpoints(sim, periods)
        o = _oracle_traj(oracle, mode_name, table if mode_name == "table" else None, 5000, 360)
        _check(oracle, stats, o["traj"], periods, 1000.0, n_bins, 500.0, 6000.0, (mode_name, k, n_bins))
    for mode, k, n_bins in ((MODE_TABLE, 64, _lib.MAX_CHECKPOINT_BINS // 64 + 1), (MODE_GAUSSIAN, 31, _lib.MAX_CHECKPOINT_BINS // 31 + 1)):
        sim = Engine.make_sim(5000, 360, mode, SEED, n_bins=n_bins, hist_lo=500.0, hist_hi=6000.0)
        with pytest.raises(SmmcError, match="SMMC_MAX_CHECKPOINT_BINS"):
            eng.simulate_checkpoints(sim, list(range(1, k + 1)))


def test_wide_gaussian_underflow_overflow_and_non_finite_values(eng, oracle):
    """gauss_std 9 over 1000 periods (the request of the checked-divide tests): values run out of the bucket range
    on both sides and to inf; every one lands where the oracle puts it."""
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN
    n, p, lo, hi = 6000, 1000, 10.0, 1.0e9
    periods = [1, 10, 100, 250, 500, 750, 999, 1000]
    sim = Engine.make_sim(n, p, MODE_GAUSSIAN, SEED, gauss_mean=2.0, gauss_std=9.0, n_bins=100, hist_lo=lo, hist_hi=hi,
                          initial_capital=2.0 ** 100)
    stats, final = eng.simulate_checkpoints(sim, periods, want_final=True)
    o = _oracle_traj(oracle, "gaussian", None, n, p, cap=2.0 ** 100, mean=2.0, std=9.0)
    assert not np.isfinite(o["traj"][:, 1000]).all()
    _check(oracle, stats, o["traj"], periods, 2.0 ** 100, 100, lo, hi)
    assert np.array_equal(final.cpu().numpy().view(np.uint32), o["final"].view(np.uint32))
    sim = Engine.make_sim(n, p, MODE_GAUSSIAN, SEED, gauss_mean=2.0, gauss_std=9.0, n_bins=100, hist_lo=500.0, hist_hi=1.0e6)
    stats, _ = eng.simulate_checkpoints(sim, periods)
    o = _oracle_traj(oracle, "gaussian", None, n, p, mean=2.0, std=9.0)
    _check(oracle, stats, o["traj"], periods, 1000.0, 100, 500.0, 1.0e6)
    assert any(st.underflow and st.overflow and st.hist.sum() for st in stats)


def test_nan_values_go_to_overflow(oracle):
    """A table with a -100 % and a huge month: 0 * inf arises along the paths; NaN counts as overflow, and min / max skip it."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import Engine, MODE_TABLE
    wild = np.array([3.0e38, -100.0, 3.0e38, 5.0, 3.0e38], dtype=np.float32)
    e = S.Engine(0)
    try:
        e.set_table(wild)
        periods = [1, 2, 3, 4, 8, 16, 40]
        sim = Engine.make_sim(3000, 40, MODE_TABLE, SEED, n_bins=16, hist_lo=0.0, hist_hi=1.0e38, initial_capital=1.0e30)
        stats, final = e.simulate_checkpoints(sim, periods, want_final=True)
        o = _oracle_traj(oracle, "table", wild, 3000, 40, cap=1.0e30)
        assert np.isnan(o["traj"][:, 40]).any()
        _check(oracle, stats, o["traj"], periods, 1.0e30, 16, 0.0, 1.0e38)
        assert np.array_equal(final.cpu().numpy().view(np.uint32), o["final"].view(np.uint32))
    finally:
        e.close()


@pytest.mark.parametrize("mode_name", ["table", "gaussian"])
def test_to_host_entry_returns_the_same_bytes(eng, mode_name):
    from stock_market_monte_carlo_amd import Engine
    sim = Engine.make_sim(70_001, 120, _mode(mode_name), 31, n_bins=100, hist_lo=0.0, hist_hi=5000.0)
    periods = [1, 12, 60, 119, 120]
    a, fa = eng.simulate_checkpoints_raw(sim, periods, want_final=True)
    b, fb = eng.simulate_checkpoints_raw(sim, periods, want_final=True, to_host=True)
    c, fc = eng.simulate_checkpoints_raw(sim, periods, want_final=False, to_host=True)
    assert a == b == c and fc is None and len(a) == 5 * 864
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))


def test_fuzz(eng, eng_big, oracle, table):
    """Seeded draws of mode, lengths, checkpoint sets, buckets and range; every drawn case is checked."""
    from stock_market_monte_carlo_amd import Engine
    rng = np.random.default_rng(0xC0FFEE)
    for case in range(40):
        mode_name = ["table", "table_big", "gaussian"][int(rng.integers(3))]
        e, tab = _pick(eng, eng_big, table, mode_name)
        p = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 100, 360, 361, 500]))
        n = int(rng.choice([1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4099, 20_011]))
        k = int(rng.integers(1, min(p, 64) + 1))
        periods = sorted(int(x) for x in rng.choice(np.arange(1, p + 1), size=k, replace=False))
        n_bins = int(rng.choice([0, 1, 7, 100, 128]))
        lo = float(rng.choice([0.0, 900.0, 1000.0]))
        hi = lo + float(rng.choice([50.0, 1000.0, 1.0e5]))
        below = float(rng.choice([900.0, 1000.0, 1100.0]))
        first = int(rng.choice([0, 1, 255, (1 << 32) - 7, 1 << 45]))
        seed = int(rng.integers(1, 1 << 62))
        exact = bool(rng.integers(2))
        sim = Engine.make_sim(n, p, _mode(mode_name), seed, first_path=first, n_bins=n_bins, hist_lo=lo, hist_hi=hi,
                              below_threshold=below, exact_div=exact)
        stats, final = e.simulate_checkpoints(sim, periods, want_final=True)
        o = _oracle_traj(oracle, mode_name, tab, n, p, first=first, seed=seed)
        _check(oracle, stats, o["traj"], periods, below, n_bins, lo, hi, (case, mode_name, p, n, periods))
        assert np.array_equal(final.cpu().numpy().view(np.uint32), o["final"].view(np.uint32)), case
