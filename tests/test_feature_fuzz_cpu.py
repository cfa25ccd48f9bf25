"""The conditions against a vacuous fuzz (tests/feature_fuzz.py), asserted on the restatements alone: of each cash-flow
function's cases at most a quarter have every path or no path depleted, of the excursion cases at most a quarter have no
path ever below its lower level or none reaching its target.  The restatements' times are printed: they are what
tests/test_feature_fuzz_gpu.py's docstring quotes."""
import time

import numpy as np
import pytest

import feature_fuzz as F
import feature_matrix as M


@pytest.mark.parametrize("family", ["cashflow_kernel", "cashflow_sweep_kernel", "portfolio_cashflow_kernel"])
def test_at_most_a_quarter_of_the_cash_flow_cases_deplete_all_or_none(oracle, family):
    t0 = time.time()
    flags = [F.vacuous(M.reference(oracle, c)) for c in F.cases(oracle, family)]
    print(f"{family}: {sum(flags)} of {len(flags)} cases deplete every path or none; references {time.time() - t0:.1f} s")
    assert len(flags) == F.PLAN[family][1] and sum(flags) <= len(flags) / 4


def test_at_most_a_quarter_of_the_excursion_cases_pass_no_level(oracle):
    t0 = time.time()
    flags = []
    for c in F.cases(oracle, "excursions_kernel"):
        r = M.reference(oracle, c)
        flags.append(not (r["first_below"] > 0).any() or not (r["first_reach"] > 0).any())
    print(f"excursions_kernel: {sum(flags)} of {len(flags)} cases with a level no path passes; references {time.time() - t0:.1f} s")
    assert sum(flags) <= len(flags) / 4


@pytest.mark.parametrize("family", ["checkpoints_kernel", "blocks_kernel", "portfolio_kernel"])
def test_the_drawn_cases_cover_what_the_fuzz_is_for(oracle, family):
    """Every function's draw holds ids beyond 2^32 and beyond 2^45, both halves of seeds, the IEEE divide and both sides of
    a Philox block; the restatement of every case can be formed."""
    t0 = time.time()
    cs = list(F.cases(oracle, family))
    for c in cs:
        M.reference(oracle, c)
    print(f"{family}: references {time.time() - t0:.1f} s")
    assert any(c["first"] >= 1 << 45 for c in cs) and any(c["first"] >> 32 > 3 for c in cs) and any(c["first"] < 256 for c in cs)
    assert any(c["seed"] >> 32 for c in cs) and any(c["exact"] for c in cs) and any(not c["exact"] for c in cs)
    assert any(c["P"] > 8 for c in cs) and any(c["P"] < 4 for c in cs) and any(c["n"] > 256 for c in cs) and any(c["n"] < 64 for c in cs)
    if family in F.P_ZERO:
        assert any(c["P"] == 0 for c in cs)
