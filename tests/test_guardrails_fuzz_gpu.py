"""Seeded random differential test of smmc_engine_simulate_guardrails: the cases of tests/guardrails_fuzz.py -- seeds, path
ids up to 2^62, K, R, E, sizes, laws and rules nobody wrote down by hand, drawn from a fixed numpy seed so that a failure
names a reproducible case -- each compared with the restatement by the comparison of tests/test_guardrails_gpu.py
(check_case): every output on its bits.  Every drawn case is run and compared, one test per case (a test sizes its own
case's rule on the restatement); none is skipped, and a case the header refuses fails the test."""
import pytest

import guardrails_fuzz as F
import test_guardrails_gpu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def drawn():
    return F.draw()


@pytest.fixture(scope="module")
def engine():
    import stock_market_monte_carlo_amd as S
    eng = S.Engine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("i", range(F.COUNT))
def test_random_guardrails(oracle, drawn, engine, i):
    c = F.finish(oracle, drawn[i])
    assert c["i"] == i
    if c["mode"] == "table":
        engine.set_asset_table(c["assets"])
    try:
        T.check_case(oracle, engine, c)
    except AssertionError as err:
        raise AssertionError(f"{F.brief(c)}: {err}") from err
