"""smmc_engine_simulate_portfolio_cashflow_regimes on the device against the numpy restatement of its contract
(tests/portfolio_cashflow_regimes_reference.py), bit for bit: final values, holdings, totals paid, periods of depletion and
the depletion counts; of the record the integer counters, buckets, min and max on their bits, the two double sums to the
relative 1e-12 of tests/test_gpu_parity.py against math.fsum of the restated binary32 values and of their squares.

K = 1 .. 4; path ids from 2^32 + 0x1234567 on; 2 * 512 + 65 = 1089 paths: two workgroups' worth and a partial last wave.
P in 1, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 17, 37 (every remainder against the 4-draw block and the 8-period field block), R in 0, 1,
4, 12, P, seven settings of the probabilities (a flip at every period, sojourns of 40 and 8, each regime never left, the
three starts), four schedules that deplete 10 % .. 90 % of the paths and two the divide rule proves safe, on the sparse,
covering product of the reference module, every other one with the IEEE divide forced.  The two regimes' laws differ in
mean, deviation and the sign of every correlation.

The four identities of include/smmc.h run against the other entries of the same engine, bytes against bytes.  The later
walk trips run in a fresh child process with SMMC_BLOCKS_PER_CU=1 (the knob is read when an engine is made), as
tests/test_walk_trips_gpu.py does.

On the commit before this feature every test here fails: the symbols do not exist."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import portfolio_cashflow_regimes_reference as Q
import regimes_reference as rref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, LO, HI, BELOW = Q.BINS, Q.LO, Q.HI, Q.BELOW
STATS = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
ALL = dict(want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
WANTS = {k: v for k, v in ALL.items() if k != "want_stats"}
KEYS = ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rg():
    from stock_market_monte_carlo_amd import regimes
    return regimes


@pytest.fixture(scope="module")
def eng():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _sim(n, P, first=0, **kw):
    import stock_market_monte_carlo_amd as S
    # gauss_mean and gauss_std are not read: values that would change every bit if they were
    return S.Engine.make_sim(n, P, S.MODE_GAUSSIAN, Q.SEED, first_path=Q.FIRST_PATH + first, initial_capital=Q.CAPITAL, gauss_mean=3.0,
                             gauss_std=11.0, **kw)


def _law(K, prob, means=None, factors=None):
    m, f = Q.laws(K)
    return dict(means=m if means is None else means, factors=f if factors is None else factors, leave_q16=prob[0], start1_q16=prob[1])


def _run(eng, sim, K, prob, R, P, law=None, **kw):
    return _rg().simulate_portfolio_cashflow_regimes(eng, sim, Q.WEIGHTS[K], rebalance_every=Q.rebalance(R, P), **(law or _law(K, prob)), **kw)


def _raw(eng, sim, K, prob, R, P, law=None, **kw):
    raw = _rg().simulate_portfolio_cashflow_regimes_raw(eng, sim, Q.WEIGHTS[K], rebalance_every=Q.rebalance(R, P), **(law or _law(K, prob)), **kw)
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


def _kind(eng, sim, K, prob, R, P, **kw):
    return _rg().portfolio_cashflow_regimes_divide_kind(eng, sim, Q.WEIGHTS[K], rebalance_every=Q.rebalance(R, P), **_law(K, prob), **kw)


# 1
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_outputs_bit_for_bit_and_every_instantiation_is_reached(oracle, eng, K):
    """Every (probabilities, P) pair with R, the schedule and the forced divide cycling; the record with every fourth case.
    The divide-kind call says which of (fast | IEEE) x (constant | varying schedule) each case ran: all four occur for this K."""
    from stock_market_monte_carlo_amd import _lib
    reached = set()
    for i, (prob, P, R, name, forced) in enumerate(Q.device_cases(K)):
        want = Q.reference(oracle, K, prob, R, name, P)
        kw = Q.cut(Q.schedules(oracle, K, prob)[name], P)
        record = i % 4 == 0
        sim = _sim(Q.N, P, exact_div=forced, **(STATS if record else {}))
        kind = _kind(eng, sim, K, prob, R, P, **kw)
        # forced is IEEE, a schedule the rule proves safe is fast; the rule may prove more (the first periods of the
        # varying schedule are contributions only), and whatever it says is what the launch takes
        assert kind in (_lib.DIV_FAST, _lib.DIV_EXACT) and (not forced or kind == _lib.DIV_EXACT), (K, prob, P, R, name, forced)
        assert forced or name not in Q.FAST_SCHEDULES or kind == _lib.DIV_FAST, (K, prob, P, R, name)
        reached.add((kind, "amounts" in kw or "fractions" in kw))
        r = _run(eng, sim, K, prob, R, P, **kw, **WANTS, want_stats=record)
        _check_outputs(r, want, (K, prob, P, R, name, forced))
        if record:
            _check_record(oracle, r.stats, want["final"], (K, prob, P, R, name))
    assert reached == {(d, v) for d in (_lib.DIV_FAST, _lib.DIV_EXACT) for v in (False, True)}


# 2
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_the_schedules_deplete_a_good_part_of_the_reference_paths_and_both_regimes_occur(oracle, K):
    """Checked on the reference, here on the CPU: a comparison of paths that all survive or all deplete would show little."""
    for prob in Q.PROBS:
        for name in Q.SCHEDULES + ["fast_constant"]:
            got = Q.reference(oracle, K, prob, 0, name, Q.LONGEST)
            depleted = 1.0 - got["depleted_at"][0] / Q.N
            assert 0.10 <= depleted <= 0.90, (K, prob, name, depleted)
    s = Q.states(oracle, Q.N, Q.LONGEST, Q.PROBS[1])
    assert 0.05 < s.mean() < 0.95 and (s[:, 1:] != s[:, :-1]).any()


# 3: identity 1
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_equal_regimes_are_simulate_portfolio_cashflow(oracle, eng, K):
    (m0, m1), (f0, f1) = Q.laws(K)
    for r, (m, f) in enumerate(((m0, f0), (m1, f1))):
        for prob, name, R, P in ((Q.PROBS[0], "amount", 4, Q.LONGEST), (Q.PROBS[1], "varying", 12, 17), (Q.PROBS[3], "floor", 1, 9),
                                 (Q.PROBS[1], "fast_constant", 4, 12)):
            kw = Q.cut(Q.schedules(oracle, K, prob)[name], P)
            sim = _sim(Q.N, P, **STATS)
            want = eng.simulate_portfolio_cashflow_raw(sim, Q.WEIGHTS[K], R, means=m, factor=f, **kw, **ALL)
            eng.sync()
            got = _bytes(_raw(eng, sim, K, prob, R, P, law=_law(K, prob, (m, m), (f, f)), **kw, **ALL))
            for key in KEYS:  # the grid rule is the parent's: the record's two binary64 sums are byte-equal too
                assert got[key] is not None and got[key] == _bytes(want)[key], (K, r, name, key)


# 4: identity 2
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_a_regime_never_left_is_simulate_portfolio_cashflow_with_its_law(oracle, eng, K):
    (m0, m1), (f0, f1) = Q.laws(K)
    for prob, m, f in ((((0, 12345), 0), m0, f0), (((54321, 0), rref.ONE), m1, f1)):
        for name, R, P in (("amount", 4, Q.LONGEST), ("varying", 1, 16), ("fraction", 0, 7)):
            kw = Q.cut(Q.schedules(oracle, K, Q.PROBS[1])[name], P)
            sim = _sim(Q.N, P, **STATS)
            want = _bytes(eng.simulate_portfolio_cashflow_raw(sim, Q.WEIGHTS[K], R, means=m, factor=f, **kw, **ALL))
            eng.sync()
            got = _bytes(_raw(eng, sim, K, prob, R, P, **kw, **ALL))
            for key in KEYS:
                assert got[key] is not None and got[key] == want[key], (K, prob, name, key)


# 5: identity 3
@pytest.mark.parametrize("prob", Q.PROBS)
def test_one_asset_without_flows_is_simulate_regimes(eng, prob):
    (m0, m1), (f0, f1) = Q.laws(1)
    for P in (7, 16, Q.LONGEST):
        for R in (0, 4):
            for exact in (False, True):  # whatever divide either call takes
                sim = _sim(Q.N, P, exact_div=exact)
                want = _rg().simulate_regimes(eng, sim, (m0[0], m1[0]), (float(f0[0, 0]), float(f1[0, 0])), leave_q16=prob[0],
                                              start1_q16=prob[1]).final.cpu().numpy()
                assert np.isfinite(want).all() and (want > 0).all()
                got = _run(eng, sim, 1, prob, R, P, **WANTS)
                assert not got.ruin_period.cpu().numpy().any() and got.depleted_at[0] == Q.N
                assert got.final.cpu().numpy().tobytes() == want.tobytes(), (prob, P, R, exact)
                assert got.holdings.cpu().numpy().tobytes() == want.tobytes() and not got.paid.cpu().numpy().any()


# 6: identity 4
@pytest.mark.parametrize("K", [2, 4])
def test_a_shorter_run_is_the_prefix_of_a_longer_one(oracle, eng, K):
    prob, R = Q.PROBS[1], 4
    kw = Q.schedules(oracle, K, prob)["varying"]
    long = _run(eng, _sim(Q.N, Q.LONGEST), K, prob, R, Q.LONGEST, **kw, **WANTS)
    ruin_long = long.ruin_period.cpu().numpy().view(np.uint32)
    for P in (5, 9, 16):
        short = _run(eng, _sim(Q.N, P), K, prob, R, P, **Q.cut(kw, P), **WANTS)
        ruin = short.ruin_period.cpu().numpy().view(np.uint32)
        assert np.array_equal(np.where(ruin_long <= P, ruin_long, 0), ruin), P
        assert np.array_equal(long.depleted_at[1:P + 1], short.depleted_at[1:]), P
    assert (ruin_long > 0).any() and (ruin_long == 0).any()


# 7
def test_two_shards_merge_to_the_whole(oracle, eng):
    import stock_market_monte_carlo_amd as S
    K, prob, R, P, name = 3, Q.PROBS[1], 12, Q.LONGEST, "floor"
    kw = Q.schedules(oracle, K, prob)[name]
    want = Q.reference(oracle, K, prob, R, name, P)
    cut_at = Q.GROUP + 100  # a shard that ends inside a wave
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes
    parts = [{k: v.cpu().numpy() for k, v in _raw(eng, _sim(n, P, first=first, **STATS), K, prob, R, P, **kw, **ALL).items() if k in KEYS}
             for first, n in ((0, cut_at), (cut_at, Q.N - cut_at))]
    assert np.array_equal(_bits(np.concatenate([p["final"] for p in parts])), _bits(want["final"]))
    assert np.array_equal(_bits(np.concatenate([p["holdings"] for p in parts], axis=1)), _bits(want["holdings"]))
    assert np.array_equal(_bits(np.concatenate([p["paid"] for p in parts])), _bits(want["paid"]))
    assert np.array_equal(np.concatenate([p["ruin_period"].view(np.uint32) for p in parts]), want["ruin_period"])
    assert np.array_equal(parts[0]["depleted_at"].view(np.uint64) + parts[1]["depleted_at"].view(np.uint64), want["depleted_at"])
    merged = S.engine.stats_from_bytes(merge_stats_bytes([p["stats_raw"].tobytes() for p in parts]))
    _check_record(oracle, merged, want["final"], "merged")


# 8
def test_two_identical_calls_give_the_same_bytes_and_to_host_the_same_again(oracle, eng):
    K, prob, R, P, name = 4, Q.PROBS[0], 4, 17, "varying"
    kw = Q.cut(Q.schedules(oracle, K, prob)[name], P)
    sim = _sim(Q.N, P, **STATS)
    runs = [_bytes(_raw(eng, sim, K, prob, R, P, **kw, **ALL)) for _ in range(2)]
    assert runs[0] == runs[1] and all(runs[0][k] is not None for k in KEYS)
    host = _rg().simulate_portfolio_cashflow_regimes_to_host(eng, sim, Q.WEIGHTS[K], rebalance_every=R, **_law(K, prob), **kw, **ALL)
    for key in KEYS:
        h = host[key] if isinstance(host[key], bytes) else np.ascontiguousarray(host[key]).tobytes()
        assert h == runs[0][key], key
    empty = _rg().simulate_portfolio_cashflow_regimes_to_host(eng, _sim(0, P, **STATS), Q.WEIGHTS[K], rebalance_every=R, **_law(K, prob), **kw, **ALL)
    assert not empty["depleted_at"].any() and empty["final"].size == 0 and empty["holdings"].shape == (K, 0)


# 9
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import portfolio_cashflow_regimes_reference as Q
import stock_market_monte_carlo_amd as S
from stock_market_monte_carlo_amd import regimes
out, K, R, P = sys.argv[3], 2, 12, 38
prob = Q.PROBS[1]
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
res = {"grid": grid}
means, factors = Q.laws(K)
amounts = np.linspace(5.0, 50.0, P).astype(np.float32)
for n in (2 * Q.GROUP * grid + 37, 3 * Q.GROUP * grid - 1):
    sim = S.Engine.make_sim(n, P, S.MODE_GAUSSIAN, Q.SEED, first_path=Q.FIRST_PATH, initial_capital=Q.CAPITAL, n_bins=Q.BINS,
                            hist_lo=Q.LO, hist_hi=Q.HI, below_threshold=Q.BELOW)
    raw = regimes.simulate_portfolio_cashflow_regimes_raw(eng, sim, Q.WEIGHTS[K], means, factors, leave_q16=prob[0], start1_q16=prob[1],
                                                          rebalance_every=R, amounts=amounts, want_holdings=True, want_paid=True,
                                                          want_ruin_period=True, want_stats=True)
    eng.sync()
    for key in ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at"):
        res[f"{n}:{key}"] = raw[key].cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 2, sojourns of 40 and 8, R = 12, a varying schedule, 38 periods (four whole field blocks, a draw block and two
    periods): every wave makes a second and a third trip; the state, the countdown and the schedule begin again with every
    path."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid, K, R, P, prob = int(got["grid"]), 2, 12, 38, Q.PROBS[1]
    sizes = (2 * Q.GROUP * grid + 37, 3 * Q.GROUP * grid - 1)
    means, factors = Q.laws(K)
    a = Q.multipliers_of(oracle, means, factors, max(sizes), P, prob)
    want = Q.pcref.simulate(a, Q.WEIGHTS[K], R, amounts=np.linspace(5.0, 50.0, P).astype(np.float32))
    assert 0.10 <= (want["ruin_period"] > 0).mean() <= 0.90
    for n in sizes:
        assert np.array_equal(_bits(got[f"{n}:final"]), _bits(want["final"][:n])), n
        assert np.array_equal(_bits(got[f"{n}:holdings"]), _bits(want["holdings"][:, :n])), n
        assert np.array_equal(_bits(got[f"{n}:paid"]), _bits(want["paid"][:n])), n
        assert np.array_equal(got[f"{n}:ruin_period"].view(np.uint32), want["ruin_period"][:n]), n
        assert np.array_equal(got[f"{n}:depleted_at"].view(np.uint64), np.bincount(want["ruin_period"][:n], minlength=P + 1)), n
        _check_record(oracle, S.engine.stats_from_bytes(got[f"{n}:stats_raw"].tobytes()), want["final"][:n], n)
