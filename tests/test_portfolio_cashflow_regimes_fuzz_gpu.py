"""Seeded random differential test of smmc_engine_simulate_portfolio_cashflow_regimes: the cases of
tests/portfolio_cashflow_regimes_fuzz.py -- seeds, path ids up to 2^62, K, laws, probabilities, P, R, weights and schedules
nobody wrote down by hand, drawn from fixed numpy seeds so that a failure names a reproducible case -- each compared with
the restatement: every per-path output and the depletion counts on their bits, the record's integer fields, min, max and
buckets exactly and its two double sums to relative 1e-12 against math.fsum.  Every drawn case is run and compared, one test
per case (a test sizes its own case's schedule on the restatement); none is skipped, and a case the header refuses fails the
test.

On the commit before this feature every test here fails: the symbols do not exist."""
import math

import numpy as np
import pytest

import portfolio_cashflow_regimes_fuzz as F

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def drawn():
    return F.draw()


@pytest.fixture(scope="module")
def engine():
    import stock_market_monte_carlo_amd as S
    eng = S.Engine(0)
    yield eng
    eng.close()


def check_case(oracle, eng, c):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import regimes
    n_bins, lo, hi, below = c["hist"]
    want = F.reference(oracle, c)
    sim = S.Engine.make_sim(c["n"], c["P"], S.MODE_GAUSSIAN, c["seed"], first_path=c["first"], initial_capital=c["capital"], n_bins=n_bins,
                            hist_lo=lo, hist_hi=hi, below_threshold=below, exact_div=c["exact"])
    r = regimes.simulate_portfolio_cashflow_regimes(eng, sim, c["weights"], c["means"], c["factors"], leave_q16=c["prob"][0],
                                                    start1_q16=c["prob"][1], rebalance_every=c["R"], want_holdings=True, want_paid=True,
                                                    want_ruin_period=True, want_stats=True, want_depleted_at=True, **c["schedule"])
    assert np.array_equal(_bits(r.final.cpu().numpy()), _bits(want["final"])), "final"
    assert r.holdings.shape == want["holdings"].shape and np.array_equal(_bits(r.holdings.cpu().numpy()), _bits(want["holdings"])), "holdings"
    assert np.array_equal(_bits(r.paid.cpu().numpy()), _bits(want["paid"])), "paid"
    assert np.array_equal(r.ruin_period.cpu().numpy().view(np.uint32), want["ruin_period"]), "ruin_period"
    assert np.array_equal(r.depleted_at, want["depleted_at"]) and int(r.depleted_at.sum()) == c["n"], "depleted_at"
    st, values = r.stats, want["final"]
    ost, ohist = oracle.values_stats(values, below, n_bins, lo, hi)
    assert st.count == ost.count == values.size, "count"
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), "counters"
    assert st.min == ost.min and st.max == ost.max, "extremes"
    assert np.array_equal(st.hist[:n_bins], ohist[:n_bins]), "buckets"
    d = np.ascontiguousarray(values, dtype=np.float64)
    assert st.sum == pytest.approx(math.fsum(d.tolist()), rel=1e-12) and st.sumsq == pytest.approx(math.fsum((d * d).tolist()), rel=1e-12), "sums"


@pytest.mark.parametrize("i", range(F.COUNT))
def test_random_regime_switching_plan(oracle, drawn, engine, i):
    c = F.finish(oracle, drawn[i])
    assert c["i"] == i
    try:
        check_case(oracle, engine, c)
    except AssertionError as err:
        raise AssertionError(f"{F.brief(c)}: {err}") from err
