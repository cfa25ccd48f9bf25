"""The 36 seeded random cases of tests/glide_reference.py (fuzz_cases) on the device against the restatement, bit for bit:
K = 1 .. 4, both modes, tables on both sides of 2048 rows, P <= 24, n <= 3000, any R, 0 to 6 changes (weights of exactly 0
among them, changes at and beyond P), constant and per-period schedules, path ids up to 2^62.
tests/test_glide_fuzz_cpu.py shows on the restatement alone that no case is vacuous."""
import pytest

import glide_reference as G
import test_glide_gpu as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(G.FUZZ_COUNT))
def test_random_glide_paths(oracle, i):
    import stock_market_monte_carlo_amd as S
    c = G.fuzz_finish(oracle, G.fuzz_draw()[i])
    eng = S.Engine(0)
    try:
        if c["mode"] == "table":
            eng.set_asset_table(c["assets"])
        T.check_case(oracle, eng, c)
    finally:
        eng.close()
