"""smmc_engine_simulate_portfolio_cashflow on the device against the numpy restatement of its contract
(tests/portfolio_cashflow_reference.py): final values, holdings, totals paid, periods of depletion and the depletion
counts on their bits; of the record the integer counters, buckets, min and max on their bits, the two double sums to the
relative 1e-12 of tests/test_gpu_parity.py against math.fsum of the restated binary32 values and of their squares.

Shapes: a joint table of 37 rows (a Philox block yields eight row indices) with K = 1 .. 4, one of 2500 rows x 2 assets
(four per block) and Gaussian mode with K = 1 .. 4; path ids from 2^32 - 100 on; 64 kW 2 + 37 paths with kW = 4 (table)
or 8 (Gaussian) waves per workgroup: whole chunks, a ragged last chunk and inactive lanes; P in 1, 7, 8, 9 and 41
(table) or 38 (Gaussian); R in 0, 1, 5, 12.  Schedules (sized in the reference module, checked in
tests/test_portfolio_cashflow_cpu.py to deplete between 10 % and 90 % of the paths at the longest P): a constant amount, a
fraction with a high floor, arrays of contributions followed by rising withdrawals, and amount plus fraction with floor
0.01; once more with a weight of exactly 0.

The later walk trips run in a fresh child process with SMMC_BLOCKS_PER_CU=1 (the knob is read when an engine is made).
Their sizes, 2 * 64 kW G + 37 and 3 * 64 kW G - 1 paths with G = the engine's grid (Engine.geometry()), rest on
host_wave_walk_grid (smmc_capi.cpp) capping the launch at min(chunks, grid) workgroups -- kGroupsPerCU = 32 per CU in
smmc_portfolio_cashflow.cpp does not bind at one workgroup per CU; if those caps change, the sizes must follow.

On the commit before this feature every test here fails: the symbols do not exist.  A build with a deliberate contract
error -- the rebalance takes the weights' shares of g, the value before the flow, instead of vn
(tools/variant_build.py, loaded through SMMC_LIB) -- fails test_outputs_bit_for_bit[t37-2-weights1] on the device."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import portfolio_cashflow_reference as ref

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("portfolio_cashflow")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, LO, HI, BELOW = ref.BINS, ref.LO, ref.HI, ref.BELOW
STATS = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
ALL = dict(want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
KEYS = ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at")


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


def _sim(shape, n, P, first=0, **kw):
    import stock_market_monte_carlo_amd as S
    mode = S.MODE_GAUSSIAN if shape == "gauss" else S.MODE_TABLE
    return S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH + first, initial_capital=ref.CAPITAL, **kw)


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


def _check_outputs(r, want, tag):
    assert np.array_equal(_bits(r.final.cpu().numpy()), _bits(want["final"])), tag
    assert r.holdings.shape == want["holdings"].shape and np.array_equal(_bits(r.holdings.cpu().numpy()), _bits(want["holdings"])), tag
    assert np.array_equal(_bits(r.paid.cpu().numpy()), _bits(want["paid"])), tag
    assert np.array_equal(r.ruin_period.cpu().numpy().view(np.uint32), want["ruin_period"]), tag
    assert np.array_equal(r.depleted_at, want["depleted_at"]) and int(r.depleted_at.sum()) == want["final"].size, tag


def _cases():
    for shape, K in ref.SHAPES:
        yield shape, K, ref.WEIGHTS[K]
    yield ref.ZERO_WEIGHT + (ref.WEIGHTS_WITH_ZERO[ref.ZERO_WEIGHT[1]],)


# 1
@pytest.mark.parametrize("shape,K,weights", list(_cases()))
def test_outputs_bit_for_bit(oracle, engines, shape, K, weights):
    """Every schedule, R and P, block boundaries and the partial block included."""
    eng, n = engines(shape, K), ref.n_paths(shape)
    sched = ref.schedules(oracle, shape, K, weights)
    want_wants = {k: v for k, v in ALL.items() if k != "want_stats"}
    for name in ref.SCHEDULES:
        for R in ref.REBALANCE:
            for P in ref.periods(shape):
                want = ref.reference(oracle, shape, K, weights, R, name, P)
                r = eng.simulate_portfolio_cashflow(_sim(shape, n, P), weights, R, **ref.cut(sched[name], P), **want_wants,
                                                    **_gauss_args(shape, K))
                _check_outputs(r, want, (shape, K, weights, name, R, P))


# 2
@pytest.mark.parametrize("shape,K,name", [("t37", 3, "amount"), ("t2500", 2, "varying"), ("gauss", 4, "floor")])
def test_the_record_of_the_final_values(oracle, engines, shape, K, name):
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    want = ref.reference(oracle, shape, K, ref.WEIGHTS[K], 12, name, P)
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)
    r = eng.simulate_portfolio_cashflow(_sim(shape, n, P, **STATS), ref.WEIGHTS[K], 12, want_final=False, want_stats=True, **kw,
                                        **_gauss_args(shape, K))
    assert r.final is None and r.holdings is None and r.paid is None
    _check_record(oracle, r.stats, want["final"], (shape, K, name))
    assert np.array_equal(r.depleted_at, want["depleted_at"])
    assert r.survival()[-1] == pytest.approx(want["depleted_at"][0] / n)


# 3
@pytest.mark.parametrize("T", [37, 2500])
@pytest.mark.parametrize("name", ["amount", "varying"])
def test_one_asset_with_weight_one_is_simulate_cashflow_on_that_column(oracle, T, name):
    import stock_market_monte_carlo_amd as S
    shape, column = "t%d" % T, ref.asset_table(T, 1)
    n, P = ref.n_paths(shape), 41
    kw = ref.cut(ref.schedules(oracle, shape, 1, (1.0,))[name], P)
    eng = S.Engine(0)
    try:
        eng.set_table(column[:, 0])
        eng.set_asset_table(column)
        sim = _sim(shape, n, P, **STATS)
        want = eng.simulate_cashflow(sim, want_paid=True, want_ruin_period=True, want_stats=True, **kw)
        assert 0 < want.depleted_at[0] < n
        for R in (0, 5):
            got = eng.simulate_portfolio_cashflow(sim, (1.0,), R, **ALL, **kw)
            for key in ("final", "paid", "ruin_period"):
                assert getattr(got, key).cpu().numpy().tobytes() == getattr(want, key).cpu().numpy().tobytes(), (key, R)
            assert got.holdings.cpu().numpy().tobytes() == want.final.cpu().numpy().tobytes(), R
            assert np.array_equal(got.depleted_at, want.depleted_at), R
            a, b = got.stats, want.stats
            assert (a.count, a.below, a.underflow, a.overflow, a.min, a.max) == (b.count, b.below, b.underflow, b.overflow, b.min, b.max)
            assert np.array_equal(a.hist, b.hist)
            assert a.sum == pytest.approx(b.sum, rel=1e-12) and a.sumsq == pytest.approx(b.sumsq, rel=1e-12)
    finally:
        eng.close()


@pytest.mark.parametrize("shape,K", [("t37", 3), ("gauss", 4)])
@pytest.mark.parametrize("R", [0, 5])
def test_zero_flows_are_simulate_portfolio(engines, shape, K, R):
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    g = _gauss_args(shape, K)
    want = eng.simulate_portfolio(_sim(shape, n, P), ref.WEIGHTS[K], R, want_holdings=True, **g)
    got = eng.simulate_portfolio_cashflow(_sim(shape, n, P), ref.WEIGHTS[K], R, **ALL, **g)
    final = want.final.cpu().numpy()
    assert np.isfinite(final).all() and (final > 0).all()
    assert got.final.cpu().numpy().tobytes() == final.tobytes()
    assert got.holdings.cpu().numpy().tobytes() == want.holdings.cpu().numpy().tobytes()
    assert not got.paid.cpu().numpy().any() and not got.ruin_period.cpu().numpy().any() and got.depleted_at[0] == n


# 4
@pytest.mark.parametrize("shape,K,name", [("t37", 2, "varying"), ("gauss", 2, "amount")])
def test_determinism_and_the_accumulators_are_left_zero(oracle, engines, shape, K, name):
    import stock_market_monte_carlo_amd as S
    eng, n, P = engines(shape, K), ref.n_paths(shape), 24
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)
    runs = []
    for _ in range(2):
        raw = eng.simulate_portfolio_cashflow_raw(_sim(shape, n, P, **STATS), ref.WEIGHTS[K], 5, **ALL, **kw, **_gauss_args(shape, K))
        eng.sync()
        runs.append({k: raw[k].cpu().numpy().tobytes() for k in KEYS})
    assert runs[0] == runs[1]
    assert int(np.frombuffer(runs[0]["depleted_at"], dtype=np.uint64).sum()) == n
    # a plain simulate with buckets straight afterwards: its record is its own
    plain = S.Engine.make_sim(1000, 36, S.MODE_GAUSSIAN, 99, **STATS)
    st = eng.read_stats(eng.simulate(plain, want_final=False, want_stats=True).stats_raw)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 36, 1000, 99, **STATS))
    assert np.array_equal(st.hist, o["hist"]) and st.below == o["stats"].below and st.count == 1000
    # and a cash flow of fewer periods straight after that: its depletion counts are its own
    short = eng.simulate_portfolio_cashflow(_sim(shape, n, 7), ref.WEIGHTS[K], 5, **ref.cut(kw, 7), **_gauss_args(shape, K))
    assert np.array_equal(short.depleted_at, ref.reference(oracle, shape, K, ref.WEIGHTS[K], 5, name, 7)["depleted_at"])


# 5
@pytest.mark.parametrize("shape,K,kw", [("t37", 2, dict(amount=27.0, floor=0.01)), ("t37", 2, dict(amount=-15.0)),
                                        ("gauss", 3, dict(amount=27.0, floor=0.01))])
def test_the_divide_form(engines, shape, K, kw):
    """A request the rule proves safe for the reciprocal-multiply form, and the same with SMMC_FLAG_EXACT_DIV: equal bits."""
    from stock_market_monte_carlo_amd import _lib
    eng, n, P = engines(shape, K), ref.n_paths(shape), ref.longest(shape)
    g = _gauss_args(shape, K)
    fast, exact = _sim(shape, n, P), _sim(shape, n, P, exact_div=True)
    assert eng.portfolio_cashflow_divide_kind(fast, ref.WEIGHTS[K], 5, **kw, **g) == _lib.DIV_FAST
    assert eng.portfolio_cashflow_divide_kind(exact, ref.WEIGHTS[K], 5, **kw, **g) == _lib.DIV_EXACT
    assert eng.portfolio_cashflow_divide_kind(fast, ref.WEIGHTS[K], 5, fraction=0.004, **g) == _lib.DIV_EXACT  # unproven
    wants = {k: v for k, v in ALL.items() if k != "want_stats"}
    a = eng.simulate_portfolio_cashflow_raw(fast, ref.WEIGHTS[K], 5, **kw, **wants, **g)
    b = eng.simulate_portfolio_cashflow_raw(exact, ref.WEIGHTS[K], 5, **kw, **wants, **g)
    eng.sync()
    for key in ("final", "holdings", "paid", "ruin_period", "depleted_at"):
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key
    if kw["amount"] > 0:  # buy and hold: holdings turn negative, the form covers both signs
        a = eng.simulate_portfolio_cashflow_raw(fast, ref.WEIGHTS[K], 0, **kw, **wants, **g)
        b = eng.simulate_portfolio_cashflow_raw(exact, ref.WEIGHTS[K], 0, **kw, **wants, **g)
        eng.sync()
        assert eng.portfolio_cashflow_divide_kind(fast, ref.WEIGHTS[K], 0, **kw, **g) == _lib.DIV_FAST
        assert (a["holdings"].cpu().numpy() < 0).any()
        for key in ("final", "holdings", "paid", "ruin_period", "depleted_at"):
            assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key


# 6
@pytest.mark.parametrize("shape,K,name", [("t37", 3, "varying"), ("gauss", 3, "floor")])
def test_two_shards_split_at_an_odd_path_are_the_whole_request(oracle, engines, shape, K, name):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes
    eng, n, P, cut = engines(shape, K), ref.n_paths(shape), 24, 333
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)

    def run(first, count):
        raw = eng.simulate_portfolio_cashflow_raw(_sim(shape, count, P, first=first, **STATS), ref.WEIGHTS[K], 5, **ALL, **kw,
                                                  **_gauss_args(shape, K))
        eng.sync()
        return {k: raw[k].cpu().numpy() for k in KEYS}

    whole, lo, hi = run(0, n), run(0, cut), run(cut, n - cut)
    for key in ("final", "paid", "ruin_period"):
        assert np.concatenate([lo[key], hi[key]]).tobytes() == whole[key].tobytes(), key
    assert np.concatenate([lo["holdings"], hi["holdings"]], axis=1).tobytes() == whole["holdings"].tobytes()
    assert np.array_equal(lo["depleted_at"] + hi["depleted_at"], whole["depleted_at"])
    merged = S.engine.stats_from_bytes(merge_stats_bytes([lo["stats_raw"].tobytes(), hi["stats_raw"].tobytes()]))
    want = S.engine.stats_from_bytes(whole["stats_raw"].tobytes())
    assert (merged.count, merged.below, merged.underflow, merged.overflow) == (want.count, want.below, want.underflow, want.overflow)
    assert merged.min == want.min and merged.max == want.max and np.array_equal(merged.hist, want.hist)
    assert merged.sum == pytest.approx(want.sum, rel=1e-12) and merged.sumsq == pytest.approx(want.sumsq, rel=1e-12)


# 7
@pytest.mark.parametrize("shape,K,name", [("t37", 4, "varying"), ("gauss", 2, "fraction")])
def test_the_host_form_is_the_device_form(oracle, engines, shape, K, name):
    eng, n, P = engines(shape, K), ref.n_paths(shape), 24
    kw = ref.cut(ref.schedules(oracle, shape, K, ref.WEIGHTS[K])[name], P)
    g = _gauss_args(shape, K)
    sim = _sim(shape, n, P, **STATS)
    raw = eng.simulate_portfolio_cashflow_raw(sim, ref.WEIGHTS[K], 12, **ALL, **kw, **g)
    eng.sync()
    host = eng.simulate_portfolio_cashflow_to_host(sim, ref.WEIGHTS[K], 12, **ALL, **kw, **g)
    for key in KEYS:
        h = host[key] if isinstance(host[key], bytes) else host[key].tobytes()
        assert h == raw[key].cpu().numpy().tobytes(), key
    empty = eng.simulate_portfolio_cashflow_to_host(_sim(shape, 0, P, **STATS), ref.WEIGHTS[K], 12, **ALL, **kw, **g)
    assert not empty["depleted_at"].any() and empty["final"].size == 0 and empty["holdings"].shape == (K, 0)
    assert not np.frombuffer(empty["stats_raw"], dtype=np.uint64)[:4].any()  # count, below, underflow, overflow


# 8
_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import portfolio_cashflow_reference as ref
import stock_market_monte_carlo_amd as S
out, K, R = sys.argv[3], 3, 5
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
eng.set_asset_table(ref.asset_table(37, K))
means, stds, corr = ref.gauss_setup(K)
res = {"grid": grid}
for shape, mode, kW, extra in (("t37", S.MODE_TABLE, 4, {}), ("gauss", S.MODE_GAUSSIAN, 8, {"means": means, "factor": ref.factor_of(stds, corr)})):
    P = ref.longest(shape)
    kw = ref.schedules(O, shape, K, ref.WEIGHTS[K])["varying"]
    for n in (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1):
        sim = S.Engine.make_sim(n, P, mode, ref.SEED, first_path=ref.FIRST_PATH, initial_capital=ref.CAPITAL, n_bins=ref.BINS,
                                hist_lo=ref.LO, hist_hi=ref.HI, below_threshold=ref.BELOW)
        raw = eng.simulate_portfolio_cashflow_raw(sim, ref.WEIGHTS[K], R, want_holdings=True, want_paid=True, want_ruin_period=True,
                                                  want_stats=True, **kw, **extra)
        eng.sync()
        for key in ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at"):
            res[f"{shape}:{n}:{key}"] = raw[key].cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 3, R = 5, the varying schedule, both modes: every wave makes a second and a third trip, the lanes' records
    persist across them and the schedule is read again from its start."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid, K, R = int(got["grid"]), 3, 5
    for shape, kW in (("t37", 4), ("gauss", 8)):
        P = ref.longest(shape)
        sizes = (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1)
        a = ref.multipliers(oracle, shape, K, max(sizes), P)
        want = ref.simulate(a, ref.WEIGHTS[K], R, **ref.schedules(oracle, shape, K, ref.WEIGHTS[K])["varying"])
        for n in sizes:
            tag = (shape, n)
            assert np.array_equal(_bits(got[f"{shape}:{n}:final"]), _bits(want["final"][:n])), tag
            assert np.array_equal(_bits(got[f"{shape}:{n}:holdings"]), _bits(want["holdings"][:, :n])), tag
            assert np.array_equal(_bits(got[f"{shape}:{n}:paid"]), _bits(want["paid"][:n])), tag
            assert np.array_equal(got[f"{shape}:{n}:ruin_period"].view(np.uint32), want["ruin_period"][:n]), tag
            assert np.array_equal(got[f"{shape}:{n}:depleted_at"].view(np.uint64), np.bincount(want["ruin_period"][:n], minlength=P + 1)), tag
            _check_record(oracle, S.engine.stats_from_bytes(got[f"{shape}:{n}:stats_raw"].tobytes()), want["final"][:n], tag)
