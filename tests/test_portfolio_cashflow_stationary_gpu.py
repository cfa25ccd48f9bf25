"""smmc_engine_simulate_portfolio_cashflow_stationary on the device against the numpy restatement of its contract
(tests/portfolio_cashflow_stationary_reference.py), bit for bit: final values, holdings, totals paid, periods of depletion
and the depletion counts; of the record the integer counters, buckets, min and max on their bits, the two double sums to
the relative 1e-12 of tests/test_gpu_parity.py against math.fsum of the restated binary32 values and of their squares.

Tables: 37 rows with K = 1 .. 4 (eight candidates per Philox block), 2500 rows x 2 assets (four; K = 1, 3, 4 once each and
in the test of the instantiations), 5 rows x 2 assets (fewer rows than a segment) and 1 row x 1 asset; path ids from
2^32 - 100 on; 64 * 4 * 2 + 37 = 549 paths: whole chunks, a ragged one and inactive lanes.  renew_q16 in 0, 1, 5461, 21845,
32768, 65535, 65536, P in 1, 7, 8, 9, 16, 41, R in 0, 1, 5, 12 on the sparse, covering product of the reference module (every
(q, P) with every R, the four schedules cycling), once more with a weight of exactly 0.
tests/test_portfolio_cashflow_stationary_cpu.py shows that the reviewed edges of the row rule occur among these cases and
that the schedules deplete 10 % .. 90 % of the paths.

The three identities of include/smmc.h run against the other entries of the same engine, bytes against bytes.  The later
walk trips run in a fresh child process with SMMC_BLOCKS_PER_CU=1 (the knob is read when an engine is made), as
tests/test_real_cashflow_gpu.py does; their sizes rest on host_wave_walk_grid capping the launch at min(chunks, grid).

On the commit before this feature every test here fails: the symbols do not exist."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import portfolio_cashflow_stationary_reference as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, LO, HI, BELOW = Q.BINS, Q.LO, Q.HI, Q.BELOW
STATS = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
ALL = dict(want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
WANTS = {k: v for k, v in ALL.items() if k != "want_stats"}
KEYS = ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _st():
    from stock_market_monte_carlo_amd import stationary
    return stationary


@pytest.fixture(scope="module")
def engines():
    """One engine per table, made on first use; none has a single-series table unless a test sets one."""
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(T, K):
        if (T, K) not in made:
            made[T, K] = S.Engine(0)
            made[T, K].set_asset_table(Q.asset_table(T, K))
        return made[T, K]

    yield get
    for e in made.values():
        e.close()


def _sim(n, P, first=0, **kw):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(n, P, S.MODE_TABLE, Q.SEED, first_path=Q.FIRST_PATH + first, initial_capital=Q.CAPITAL, **kw)


def _run(eng, sim, weights, q, R, **kw):
    return _st().simulate_portfolio_cashflow_stationary(eng, sim, weights, renew_q16=q, rebalance_every=R, **kw)


def _raw(eng, sim, weights, q, R, **kw):
    raw = _st().simulate_portfolio_cashflow_stationary_raw(eng, sim, weights, renew_q16=q, rebalance_every=R, **kw)
    eng.sync()
    return raw


def _bytes(raw):
    return {k: None if raw[k] is None else raw[k].cpu().numpy().tobytes() for k in KEYS}


def _check_record(oracle, st, values, tag):
    ost, ohist = oracle.values_stats(values, BELOW, BINS, LO, HI)
    assert st.count == ost.count == values.size, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert st.min == ost.min and st.max == ost.max, tag
    assert np.array_equal(st.hist, ohist) and int(st.hist.sum()) + st.underflow + st.overflow == values.size, tag
    d = np.ascontiguousarray(values, dtype=np.float64)
    assert st.sum == pytest.approx(math.fsum(d.tolist()), rel=1e-12) and st.sumsq == pytest.approx(math.fsum((d * d).tolist()), rel=1e-12), tag


def _check_outputs(r, want, tag):
    assert np.array_equal(_bits(r.final.cpu().numpy()), _bits(want["final"])), tag
    assert r.holdings.shape == want["holdings"].shape and np.array_equal(_bits(r.holdings.cpu().numpy()), _bits(want["holdings"])), tag
    assert np.array_equal(_bits(r.paid.cpu().numpy()), _bits(want["paid"])), tag
    assert np.array_equal(r.ruin_period.cpu().numpy().view(np.uint32), want["ruin_period"]), tag
    assert np.array_equal(r.depleted_at, want["depleted_at"]) and int(r.depleted_at.sum()) == want["final"].size, tag


def _cases():
    for T, K in Q.TABLES:
        yield T, K, Q.WEIGHTS[K]
    yield Q.ZERO_WEIGHT + (Q.WEIGHTS_WITH_ZERO[Q.ZERO_WEIGHT[1]],)


# 1
@pytest.mark.parametrize("T,K,weights", list(_cases()))
def test_outputs_bit_for_bit(oracle, engines, T, K, weights):
    """Every q and P with every R, the schedules cycling; the record of the final values with every fourth case."""
    eng = engines(T, K)
    for i, (q, P, R, name) in enumerate(Q.device_cases(T)):
        want = Q.reference(oracle, T, K, weights, R, name, P, q)
        kw = Q.cut(Q.schedules(oracle, T, K, weights, q)[name], P)
        record = i % 4 == 0
        r = _run(eng, _sim(Q.N, P, **(STATS if record else {})), weights, q, R, **kw, **WANTS, want_stats=record)
        _check_outputs(r, want, (T, K, weights, q, P, R, name))
        if record:
            _check_record(oracle, r.stats, want["final"], (T, K, q, P, R, name))


# 2
@pytest.mark.parametrize("T,K", Q.FOUR_DRAW_ONCE)
def test_the_four_draw_table_with_the_other_widths(oracle, engines, T, K):
    """2500 rows with K = 1, 3, 4: a varying and a fraction schedule, P = 41 and 9 (a tail of one period: one candidate block)."""
    eng, w = engines(T, K), Q.WEIGHTS[K]
    for q, P, R, name in ((21845, Q.LONGEST, 5, "varying"), (5461, 9, 12, "fraction"), (32768, 16, 1, "amount")):
        want = Q.reference(oracle, T, K, w, R, name, P, q)
        r = _run(eng, _sim(Q.N, P), w, q, R, **Q.cut(Q.schedules(oracle, T, K, w, q)[name], P), **WANTS)
        _check_outputs(r, want, (T, K, q, P, R, name))


# 3
@pytest.mark.parametrize("T", [37, 2500])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_every_instantiation_and_both_divides(oracle, engines, T, K):
    """(dense | four-draw table) x K x (constant | varying schedule) x (IEEE | reciprocal-multiply divide): a request whose
    rule says FAST, the same with SMMC_FLAG_EXACT_DIV, and the reference, equal bits; q = 5461 and 32768, R = 5, P = 41."""
    from stock_market_monte_carlo_amd import _lib
    eng, w, P, R = engines(T, K), Q.WEIGHTS[K], Q.LONGEST, 5
    for q in (5461, 32768):
        for form, kw in Q.fast_schedules(oracle, T, K, w, q).items():
            fast, exact = _sim(Q.N, P), _sim(Q.N, P, exact_div=True)
            kind = lambda sim: _st().portfolio_cashflow_stationary_divide_kind(eng, sim, w, renew_q16=q, rebalance_every=R, **kw)  # noqa: E731
            assert kind(fast) == _lib.DIV_FAST and kind(exact) == _lib.DIV_EXACT, (form, q)
            assert eng.portfolio_cashflow_divide_kind(fast, w, R, **kw) == _lib.DIV_FAST
            want = Q.pcref.simulate(Q.multipliers(oracle, T, K, q), w, R, **kw)
            if form == "constant":
                assert 0.10 <= 1.0 - want["depleted_at"][0] / Q.N <= 0.90, (T, K, q)
            for sim in (fast, exact):
                _check_outputs(_run(eng, sim, w, q, R, **kw, **WANTS), want, (T, K, q, form))
        # unproven requests take the IEEE divide, as the parent says
        assert _st().portfolio_cashflow_stationary_divide_kind(eng, _sim(Q.N, P), w, renew_q16=q, rebalance_every=R, fraction=0.004) == _lib.DIV_EXACT


def _same_bytes(got, want, tag):
    for key in KEYS:
        assert got[key] is not None and got[key] == want[key], tag + (key,)


# 4: identity 1
@pytest.mark.parametrize("T,K", [(37, 1), (37, 4), (2500, 2), (2500, 3), (5, 2), (1, 1)])
def test_probability_one_is_simulate_portfolio_cashflow(oracle, engines, T, K):
    eng, w = engines(T, K), Q.WEIGHTS[K]
    for name, R, P in (("amount", 5, Q.LONGEST), ("varying", 12, Q.LONGEST), ("floor", 1, 9), ("fraction", 0, 7), ("varying", 5, 16)):
        kw = Q.cut(Q.schedules(oracle, T, K, w, 65536)[name], P)
        sim = _sim(Q.N, P, **STATS)
        want = eng.simulate_portfolio_cashflow_raw(sim, w, R, **kw, **ALL)
        eng.sync()
        _same_bytes(_bytes(_raw(eng, sim, w, 65536, R, **kw, **ALL)), _bytes(want), (T, K, name))


# 5: identity 2
@pytest.mark.parametrize("T,K", [(37, 1), (37, 3), (2500, 2), (2500, 4), (5, 2), (1, 1)])
def test_probability_zero_is_one_block_of_the_block_plan(oracle, engines, T, K):
    eng, w = engines(T, K), Q.WEIGHTS[K]
    for name, R, P, L in (("amount", 5, Q.LONGEST, Q.LONGEST), ("varying", 12, Q.LONGEST, 64), ("floor", 1, 9, 9), ("fraction", 0, 7, 5000),
                          ("varying", 5, 16, 16)):
        kw = Q.cut(Q.schedules(oracle, T, K, w, 0)[name], P)
        sim = _sim(Q.N, P, **STATS)
        want = eng.simulate_portfolio_cashflow_blocks_raw(sim, w, L, R, **kw, **ALL)
        eng.sync()
        _same_bytes(_bytes(_raw(eng, sim, w, 0, R, **kw, **ALL)), _bytes(want), (T, K, name))


# 6: identity 3
@pytest.mark.parametrize("T", [37, 2500, 5])
def test_one_asset_without_flows_is_simulate_stationary_on_that_column(T):
    import stock_market_monte_carlo_amd as S
    column = Q.asset_table(T, 1)
    eng = S.Engine(0)
    try:
        eng.set_table(column[:, 0])
        eng.set_asset_table(column)
        for q in Q.RENEW:
            for P in (9, 16, Q.LONGEST):
                for exact in (False, True):  # whatever divide either call takes
                    sim = _sim(Q.N, P, exact_div=exact)
                    want = _st().simulate_stationary(eng, sim, renew_q16=q).final.cpu().numpy()
                    assert np.isfinite(want).all() and (want > 0).all()
                    got = _run(eng, sim, (1.0,), q, 0, **WANTS)
                    assert not got.ruin_period.cpu().numpy().any() and got.depleted_at[0] == Q.N  # all 549 paths are compared
                    assert got.final.cpu().numpy().tobytes() == want.tobytes(), (T, q, P, exact)
                    assert got.holdings.cpu().numpy().tobytes() == want.tobytes() and not got.paid.cpu().numpy().any()
    finally:
        eng.close()


# 7
def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream(oracle):
    """Every want on: the device tensors, read through torch's stream without an engine sync, against the host entry's."""
    import stock_market_monte_carlo_amd as S
    T, K, q, P, R, name = 37, 3, 21845, 24, 3, "varying"
    w = Q.WEIGHTS[K]
    kw = Q.cut(Q.schedules(oracle, T, K, w, q)[name], P)
    eng = S.Engine(0, stream="new")
    try:
        assert eng.own_stream
        eng.set_asset_table(Q.asset_table(T, K))
        sim = _sim(Q.N, P, **STATS)
        raw = _st().simulate_portfolio_cashflow_stationary_raw(eng, sim, w, renew_q16=q, rebalance_every=R, **ALL, **kw)
        device = _bytes(raw)  # no engine sync
        host = _st().simulate_portfolio_cashflow_stationary_to_host(eng, sim, w, renew_q16=q, rebalance_every=R, **ALL, **kw)
        empty = _st().simulate_portfolio_cashflow_stationary_to_host(eng, _sim(0, P, **STATS), w, renew_q16=q, rebalance_every=R, **ALL, **kw)
    finally:
        eng.close()
    for key in KEYS:
        h = host[key] if isinstance(host[key], bytes) else np.ascontiguousarray(host[key]).tobytes()
        assert device[key] is not None and len(h) > 0 and h == device[key], key
    assert np.array_equal(_bits(np.frombuffer(device["final"], dtype=np.float32)), _bits(Q.reference(oracle, T, K, w, R, name, P, q)["final"]))
    assert not empty["depleted_at"].any() and empty["final"].size == 0 and empty["holdings"].shape == (K, 0)
    assert not np.frombuffer(empty["stats_raw"], dtype=np.uint64)[:4].any()  # count, below, underflow, overflow


# 8
def test_null_outputs_singly_and_all_together(oracle, engines):
    T, K, q, P, R, name = 37, 3, 21845, 24, 5, "varying"
    eng, w = engines(T, K), Q.WEIGHTS[K]
    kw = Q.cut(Q.schedules(oracle, T, K, w, q)[name], P)
    sim = _sim(Q.N, P, **STATS)
    full = _bytes(_raw(eng, sim, w, q, R, **ALL, **kw))
    wants = dict(want_final=True, **ALL)
    for left_out in list(wants) + [None]:
        asked = {k: left_out is not None and k != left_out for k in wants}  # None: every output NULL
        got = _bytes(_raw(eng, sim, w, q, R, **asked, **kw))
        for key in KEYS:
            want_key = "want_" + ("stats" if key == "stats_raw" else key)
            assert got[key] == (full[key] if asked[want_key] else None), (left_out, key)


# 9
@pytest.mark.parametrize("T,K,name,q", [(37, 2, "varying", 5461), (2500, 2, "amount", 32768)])
def test_determinism_and_the_accumulators_are_left_zero(oracle, engines, T, K, name, q):
    import stock_market_monte_carlo_amd as S
    eng, P, w = engines(T, K), 24, Q.WEIGHTS[K]
    kw = Q.cut(Q.schedules(oracle, T, K, w, q)[name], P)
    runs = [_bytes(_raw(eng, _sim(Q.N, P, **STATS), w, q, 5, **ALL, **kw)) for _ in range(2)]
    assert runs[0] == runs[1]
    assert int(np.frombuffer(runs[0]["depleted_at"], dtype=np.uint64).sum()) == Q.N
    # a plain simulate with buckets straight afterwards: its record is its own
    plain = S.Engine.make_sim(1000, 36, S.MODE_GAUSSIAN, 99, **STATS)
    st = eng.read_stats(eng.simulate(plain, want_final=False, want_stats=True).stats_raw)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 36, 1000, 99, **STATS))
    assert np.array_equal(st.hist, o["hist"]) and st.below == o["stats"].below and st.count == 1000
    # and a run of fewer periods straight after that: its depletion counts are its own
    short = _run(eng, _sim(Q.N, 7), w, q, 5, **Q.cut(kw, 7))
    assert np.array_equal(short.depleted_at, Q.reference(oracle, T, K, w, 5, name, 7, q)["depleted_at"])


# 10
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import portfolio_cashflow_stationary_reference as Q
import stock_market_monte_carlo_amd as S
from stock_market_monte_carlo_amd import stationary
out, T, K, R, q, P = sys.argv[3], 37, 3, 5, 21845, 9
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
eng.set_asset_table(Q.asset_table(T, K))
res = {"grid": grid}
kw = Q.cut(Q.schedules(O, T, K, Q.WEIGHTS[K], q)["varying"], P)
for n in (2 * 256 * grid + 37, 3 * 256 * grid - 1):
    sim = S.Engine.make_sim(n, P, S.MODE_TABLE, Q.SEED, first_path=Q.FIRST_PATH, initial_capital=Q.CAPITAL, n_bins=Q.BINS,
                            hist_lo=Q.LO, hist_hi=Q.HI, below_threshold=Q.BELOW)
    raw = stationary.simulate_portfolio_cashflow_stationary_raw(eng, sim, Q.WEIGHTS[K], renew_q16=q, rebalance_every=R, want_holdings=True,
                                                                want_paid=True, want_ruin_period=True, want_stats=True, **kw)
    eng.sync()
    for key in ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at"):
        res[f"{n}:{key}"] = raw[key].cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 3, q = 21845, R = 5, the varying schedule, P = 9 (a whole segment and a tail): every wave makes a second and a
    third trip, the lanes' records persist across them, and the index, the period count and the schedule begin again with
    every path."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid, T, K, R, q, P = int(got["grid"]), 37, 3, 5, 21845, 9
    sizes = (2 * 256 * grid + 37, 3 * 256 * grid - 1)
    a = Q.multipliers_of(oracle, Q.asset_table(T, K), max(sizes), P, q)
    want = Q.pcref.simulate(a, Q.WEIGHTS[K], R, **Q.cut(Q.schedules(oracle, T, K, Q.WEIGHTS[K], q)["varying"], P))
    for n in sizes:
        assert np.array_equal(_bits(got[f"{n}:final"]), _bits(want["final"][:n])), n
        assert np.array_equal(_bits(got[f"{n}:holdings"]), _bits(want["holdings"][:, :n])), n
        assert np.array_equal(_bits(got[f"{n}:paid"]), _bits(want["paid"][:n])), n
        assert np.array_equal(got[f"{n}:ruin_period"].view(np.uint32), want["ruin_period"][:n]), n
        assert np.array_equal(got[f"{n}:depleted_at"].view(np.uint64), np.bincount(want["ruin_period"][:n], minlength=P + 1)), n
        _check_record(oracle, S.engine.stats_from_bytes(got[f"{n}:stats_raw"].tobytes()), want["final"][:n], n)
