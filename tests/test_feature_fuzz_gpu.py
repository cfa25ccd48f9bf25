"""Seeded random differential test of the seven feature entry points: seeds, path ids, sizes, capitals, laws, tables,
buckets, divides and each feature's own arguments that nobody wrote down by hand (tests/feature_fuzz.py draws them from a
fixed numpy seed per function, so a failure names a reproducible case), each compared with the family's restatement by
the comparison of tests/test_feature_matrix_gpu.py.  Every drawn case is run and compared; none is skipped, and a case the
header refuses fails the test.

Reference work per function, measured on the CPU with the restatements run alone (tests/test_feature_fuzz_cpu.py prints
it; the sizing of the schedules included): checkpoints 40 cases < 0.1 s, cash flows 40 cases 1.6 s, sweeps 30 cases 4.3 s,
excursions 40 cases 0.8 s, blocks 40 cases 0.1 s, portfolios 30 cases 0.7 s, portfolio cash flows 30 cases 3.5 s: all far
below the 30 s a function may take.

Evidence that the fuzz bites (a tools/variant_build.py build loaded through SMMC_LIB, run once on the device):
portfolio_kernel's high id word masked to its low two bits (path_hi & 3 where the draws are made) passes all of
tests/test_portfolio_gpu.py and tests/test_feature_matrix_gpu.py and fails test_random_portfolios here, first at case 5.
The same mask in another feature kernel was not run.

Wall time per function on an MI355X, references included: checkpoints 4.8 s, cash flows 0.6 s, sweeps 1.2 s, excursions
9.9 s, blocks 5.0 s, portfolios 1.7 s, portfolio cash flows 19.0 s."""
import pytest

import feature_fuzz as F
import test_feature_matrix_gpu as G

pytestmark = pytest.mark.gpu


def _run(oracle, family, check, monkeypatch=None):
    import stock_market_monte_carlo_amd as S
    eng = S.Engine(0)
    try:
        for c in F.cases(oracle, family):
            if c["mode"] == "table":
                if "assets" in c:
                    eng.set_asset_table(c["assets"])
                else:
                    eng.set_table(c["table"])
            try:
                check(oracle, eng, c)
            except AssertionError as err:
                raise AssertionError(f"{F.brief(c)}: {err}") from err
    finally:
        eng.close()


def test_random_checkpoints(oracle):
    _run(oracle, "checkpoints_kernel", G.check_checkpoints)


def test_random_cashflows(oracle):
    _run(oracle, "cashflow_kernel", G.check_cashflow)


def test_random_cashflow_sweeps(oracle):
    _run(oracle, "cashflow_sweep_kernel", G.check_cashflow_sweep)


def test_random_excursions(oracle):
    _run(oracle, "excursions_kernel", G.check_excursions)


def test_random_blocks(oracle, monkeypatch):
    monkeypatch.delenv("SMMC_BLOCKS_READ", raising=False)  # the host's own choice of layout
    _run(oracle, "blocks_kernel", G.check_blocks)


def test_random_portfolios(oracle):
    _run(oracle, "portfolio_kernel", G.check_portfolio)


def test_random_portfolio_cashflows(oracle):
    _run(oracle, "portfolio_cashflow_kernel", G.check_portfolio_cashflow)
