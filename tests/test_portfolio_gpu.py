"""smmc_engine_simulate_portfolio on the device against the numpy restatement of its contract
(tests/portfolio_reference.py): per-path outputs, integer counters, buckets, min and max on their bits, the two double
sums to the relative 1e-12 of tests/test_gpu_parity.py against math.fsum of the restated binary32 values and of their
squares (as tests/test_walk_trips_gpu.py).

Shapes: a joint table of 37 rows (a Philox block yields eight row indices), one of 2500 rows x 2 assets (four per block)
and Gaussian mode; path ids from 2^32 - 100 on; 64 kW 2 + 37 paths with kW = 4 (table) or 8 (Gaussian) waves per
workgroup: whole chunks, a ragged last chunk and inactive lanes.

The later walk trips run in a fresh child process with SMMC_BLOCKS_PER_CU=1 (the knob is read when an engine is made).
Their sizes, 2 * 64 kW G + 37 and 3 * 64 kW G - 1 paths with G = the engine's grid (Engine.geometry()), rest on
host_wave_walk_grid (smmc_capi.cpp) capping a portfolio launch at min(chunks, grid) workgroups -- kPortfolioGroupsPerCU = 32
per CU in smmc_portfolio.cpp does not bind at one workgroup per CU; if those caps change, the sizes must follow.

On the commit before this feature every test here fails: the symbols do not exist.  A build with a deliberate contract
error -- the countdown to the rebalance started at 1 instead of R, so that the kernel rebalances at t mod R == 1
(tools/variant_build.py, loaded through SMMC_LIB) -- fails test_final_values_and_holdings_bit_for_bit[t37-2] on the
device."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import portfolio_reference as ref

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("portfolio")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("t37", 1), ("t37", 2), ("t37", 3), ("t37", 4), ("t2500", 2), ("gauss", 1), ("gauss", 2), ("gauss", 3), ("gauss", 4)]
REBALANCE = [0, 1, 5, 12]
BINS, LO, HI, BELOW = ref.BINS, ref.LO, ref.HI, ref.BELOW


def _periods(shape):
    return [0, 1, 7, 8, 9, 38 if shape == "gauss" else 41]


def _n_paths(shape):
    return 64 * (8 if shape == "gauss" else 4) * 2 + 37


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gauss_args(shape, K):
    if shape != "gauss":
        return {}
    means, stds, corr = ref.gauss_setup(K)
    return {"means": means, "factor": ref.factor_of(stds, corr)}


@pytest.fixture(scope="module")
def engines():
    """One engine per shape, made on first use; table-mode engines have no single-series table unless a test sets one."""
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(shape, K):
        key = (shape, K if shape != "gauss" else 0)
        if key not in made:
            made[key] = S.Engine(0)
            if shape != "gauss":
                made[key].set_asset_table(ref.asset_table(int(shape[1:]), K))
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _sim(shape, n, P, **kw):
    import stock_market_monte_carlo_amd as S
    mode = S.MODE_GAUSSIAN if shape == "gauss" else S.MODE_TABLE
    return S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL, **kw)


def _exact_sums(values):
    d = np.ascontiguousarray(values, dtype=np.float64)
    return math.fsum(d.tolist()), math.fsum((d * d).tolist())


def _check_record(oracle, st, values, tag):
    ost, ohist = oracle.values_stats(values, BELOW, BINS, LO, HI)
    assert st.count == ost.count == values.size, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert st.min == ost.min and st.max == ost.max, tag
    assert np.array_equal(st.hist, ohist) and int(st.hist.sum()) + st.underflow + st.overflow == values.size, tag
    s1, s2 = _exact_sums(values)
    assert st.sum == pytest.approx(s1, rel=1e-12) and st.sumsq == pytest.approx(s2, rel=1e-12), tag


# 1
@pytest.mark.parametrize("shape,K", SHAPES)
def test_final_values_and_holdings_bit_for_bit(oracle, engines, shape, K):
    """Every R and P, block boundaries and the partial block included; once more with one weight of exactly 0."""
    eng, n = engines(shape, K), _n_paths(shape)
    a = ref.multipliers(oracle, shape, K, n, max(_periods(shape)))
    for weights in [ref.WEIGHTS[K]] + ([ref.WEIGHTS_WITH_ZERO[K]] if K > 1 else []):
        for R in REBALANCE:
            for P in _periods(shape):
                values, holdings = ref.simulate(a[:, :P], weights, R)
                r = eng.simulate_portfolio(_sim(shape, n, P), weights, R, want_holdings=True, **_gauss_args(shape, K))
                tag = (shape, K, weights, R, P)
                assert np.array_equal(_bits(r.final.cpu().numpy()), _bits(values[:, P])), tag
                assert r.holdings.shape == (K, n) and np.array_equal(_bits(r.holdings.cpu().numpy()), _bits(holdings)), tag


# 2
@pytest.mark.parametrize("T", [37, 2500])
@pytest.mark.parametrize("R", [0, 5])
def test_one_asset_with_weight_one_is_simulate_on_that_column(T, R):
    import stock_market_monte_carlo_amd as S
    column = ref.asset_table(T, 1)
    n, P = _n_paths("t"), 41
    eng = S.Engine(0)
    try:
        eng.set_table(column[:, 0])
        eng.set_asset_table(column)
        sim = _sim("t", n, P, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
        plain = eng.simulate(sim, want_final=True, want_stats=True)
        want = eng.read_stats(plain.stats_raw)
        got = eng.simulate_portfolio(sim, (1.0,), R, want_stats=True)
        assert np.array_equal(_bits(got.final.cpu().numpy()), _bits(plain.final.cpu().numpy()))
        st = got.stats
        assert (st.count, st.below, st.underflow, st.overflow) == (want.count, want.below, want.underflow, want.overflow)
        assert st.min == want.min and st.max == want.max and np.array_equal(st.hist, want.hist)
        assert st.sum == pytest.approx(want.sum, rel=1e-12) and st.sumsq == pytest.approx(want.sumsq, rel=1e-12)
    finally:
        eng.close()


# 3
@pytest.mark.parametrize("shape,K", [("t37", 3), ("t2500", 2), ("gauss", 4)])
def test_the_record_of_the_final_values(oracle, engines, shape, K):
    eng, n, P = engines(shape, K), _n_paths(shape), max(_periods(shape))
    values, _ = ref.simulate(ref.multipliers(oracle, shape, K, n, P), ref.WEIGHTS[K], 12)
    sim = _sim(shape, n, P, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
    r = eng.simulate_portfolio(sim, ref.WEIGHTS[K], 12, want_final=False, want_stats=True, **_gauss_args(shape, K))
    assert r.final is None
    _check_record(oracle, r.stats, values[:, P], (shape, K))


# 4
@pytest.mark.parametrize("shape,K", [("t37", 2), ("gauss", 2)])
def test_determinism_and_the_accumulator_is_left_zero(oracle, engines, table, shape, K):
    import stock_market_monte_carlo_amd as S
    eng, n, P = engines(shape, K), _n_paths(shape), 24
    sim = _sim(shape, n, P, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
    runs = []
    for _ in range(2):
        raw = eng.simulate_portfolio_raw(sim, ref.WEIGHTS[K], 5, want_holdings=True, want_stats=True, **_gauss_args(shape, K))
        eng.sync()
        runs.append({k: raw[k].cpu().numpy().tobytes() for k in ("final", "holdings", "stats_raw")})
    assert runs[0] == runs[1]
    # a plain simulate with buckets straight afterwards: its record is its own
    plain = S.Engine.make_sim(1000, 36, S.MODE_GAUSSIAN, 99, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
    st = eng.read_stats(eng.simulate(plain, want_final=False, want_stats=True).stats_raw)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 36, 1000, 99, n_bins=BINS, hist_lo=LO, hist_hi=HI,
                                             below_threshold=BELOW))
    assert np.array_equal(st.hist, o["hist"]) and st.below == o["stats"].below and st.count == 1000


# 5
def test_the_divide_form(oracle, engines):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import _lib
    eng, n, P = engines("t37", 2), _n_paths("t37"), 41
    fast = _sim("t37", n, P)
    assert eng.portfolio_divide_kind(fast, ref.WEIGHTS[2], 5) == _lib.DIV_FAST
    exact = _sim("t37", n, P, exact_div=True)
    assert eng.portfolio_divide_kind(exact, ref.WEIGHTS[2], 5) == _lib.DIV_EXACT
    a = eng.simulate_portfolio(fast, ref.WEIGHTS[2], 5, want_holdings=True)
    b = eng.simulate_portfolio(exact, ref.WEIGHTS[2], 5, want_holdings=True)
    assert np.array_equal(_bits(a.final.cpu().numpy()), _bits(b.final.cpu().numpy()))
    assert np.array_equal(_bits(a.holdings.cpu().numpy()), _bits(b.holdings.cpu().numpy()))
    doubling = ref.asset_table(37, 2).copy()
    doubling[5, 0] = 100.0
    e2 = S.Engine(0)
    try:
        e2.set_asset_table(doubling)
        assert e2.portfolio_divide_kind(_sim("t37", n, 360), ref.WEIGHTS[2], 12) == _lib.DIV_EXACT
        # ... and the run the host then makes with the IEEE divide is the restatement's, +100 % months included
        values, holdings = ref.simulate(ref.table_multipliers(oracle, doubling, ref.SEED, ref.FIRST_PATH, n, 360), ref.WEIGHTS[2], 12)
        assert (values[:, 1:] > 1.4 * values[:, :-1]).any()  # a value up by 40 % in one month: the planted month is drawn
        r = e2.simulate_portfolio(_sim("t37", n, 360), ref.WEIGHTS[2], 12, want_holdings=True)
        assert np.array_equal(_bits(r.final.cpu().numpy()), _bits(values[:, 360]))
        assert np.array_equal(_bits(r.holdings.cpu().numpy()), _bits(holdings))
    finally:
        e2.close()


# 6
@pytest.mark.parametrize("shape,K", [("t37", 3), ("gauss", 3)])
def test_two_shards_split_at_an_odd_path_are_the_whole_request(engines, shape, K):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes
    eng, n, P, cut = engines(shape, K), _n_paths(shape), 24, 333
    kw = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
    g = _gauss_args(shape, K)

    def run(first, count):
        mode = S.MODE_GAUSSIAN if shape == "gauss" else S.MODE_TABLE
        sim = S.Engine.make_sim(count, P, mode, ref.SEED, first_path=ref.FIRST_PATH + first, initial_capital=ref.CAPITAL, **kw)
        raw = eng.simulate_portfolio_raw(sim, ref.WEIGHTS[K], 5, want_holdings=True, want_stats=True, **g)
        eng.sync()
        return raw["final"].cpu().numpy(), raw["holdings"].cpu().numpy(), raw["stats_raw"].cpu().numpy().tobytes()

    whole, lo, hi = run(0, n), run(0, cut), run(cut, n - cut)
    assert np.array_equal(_bits(np.concatenate([lo[0], hi[0]])), _bits(whole[0]))
    assert np.array_equal(_bits(np.concatenate([lo[1], hi[1]], axis=1)), _bits(whole[1]))
    merged, want = S.engine.stats_from_bytes(merge_stats_bytes([lo[2], hi[2]])), S.engine.stats_from_bytes(whole[2])
    assert (merged.count, merged.below, merged.underflow, merged.overflow) == (want.count, want.below, want.underflow, want.overflow)
    assert merged.min == want.min and merged.max == want.max and np.array_equal(merged.hist, want.hist)
    assert merged.sum == pytest.approx(want.sum, rel=1e-12) and merged.sumsq == pytest.approx(want.sumsq, rel=1e-12)


# 7
@pytest.mark.parametrize("shape,K", [("t37", 4), ("gauss", 2)])
def test_the_host_form_is_the_device_form(engines, shape, K):
    eng, n, P = engines(shape, K), _n_paths(shape), 24
    sim = _sim(shape, n, P, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
    g = _gauss_args(shape, K)
    raw = eng.simulate_portfolio_raw(sim, ref.WEIGHTS[K], 12, want_holdings=True, want_stats=True, **g)
    eng.sync()
    host = eng.simulate_portfolio_to_host(sim, ref.WEIGHTS[K], 12, want_holdings=True, want_stats=True, **g)
    assert host["final"].tobytes() == raw["final"].cpu().numpy().tobytes()
    assert host["holdings"].tobytes() == raw["holdings"].cpu().numpy().tobytes()
    assert host["stats_raw"] == raw["stats_raw"].cpu().numpy().tobytes()


# 8
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import portfolio_reference as ref
import stock_market_monte_carlo_amd as S
out, K, R = sys.argv[3], 3, 5
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
eng.set_asset_table(ref.asset_table(37, K))
means, stds, corr = ref.gauss_setup(K)
res = {"grid": grid}
for shape, mode, kW, P, extra in (("t37", S.MODE_TABLE, 4, 41, {}), ("gauss", S.MODE_GAUSSIAN, 8, 38, {"means": means, "factor": ref.factor_of(stds, corr)})):
    for n in (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1):
        sim = S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL, n_bins=ref.BINS,
                                hist_lo=ref.LO, hist_hi=ref.HI, below_threshold=ref.BELOW)
        raw = eng.simulate_portfolio_raw(sim, ref.WEIGHTS[K], R, want_holdings=True, want_stats=True, **extra)
        eng.sync()
        res[f"{shape}:{n}:final"] = raw["final"].cpu().numpy()
        res[f"{shape}:{n}:holdings"] = raw["holdings"].cpu().numpy()
        res[f"{shape}:{n}:stats"] = raw["stats_raw"].cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 3, R = 5, both modes: every wave makes a second and a third trip, the lanes' records persist across them."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid, K, R = int(got["grid"]), 3, 5
    for shape, kW, P in (("t37", 4, 41), ("gauss", 8, 38)):
        sizes = (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1)
        a = ref.multipliers(oracle, shape, K, max(sizes), P)
        values, holdings = ref.simulate(a, ref.WEIGHTS[K], R)
        for n in sizes:
            tag = (shape, n)
            assert np.array_equal(_bits(got[f"{shape}:{n}:final"]), _bits(values[:n, P])), tag
            assert np.array_equal(_bits(got[f"{shape}:{n}:holdings"]), _bits(holdings[:, :n])), tag
            _check_record(oracle, S.engine.stats_from_bytes(got[f"{shape}:{n}:stats"].tobytes()), values[:n, P], tag)
