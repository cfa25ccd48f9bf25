"""The three wave-walk features -- checkpoint statistics, cash flows, excursions -- against the bytes their kernels
wrote before they were given one skeleton: tests/golden/wave_walk_parent.json holds the sha256 of every output buffer,
the packed records as raw bytes (the double sums depend on the order of accumulation), taken on that commit by
tests/golden/make_wave_walk_golden.py, whose case list this test runs again.  Gaussian, dense table and four-draw
table; both divides; n_periods 1, one exact Philox block, 13 (no whole block, no partial block, both); n_paths 1, 63,
4099; 0 and 100 buckets; a constant and a varying schedule; both records and one; and 2 * grid_cap * group_paths + 77
paths at 5 periods, where every wave walks more than one chunk and the last chunk is ragged."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    path = os.path.join(GOLDEN, "wave_walk_parent.json")
    assert os.path.exists(path), "tests/golden/wave_walk_parent.json is missing: take it with make_wave_walk_golden.py on the commit before the skeleton"
    return json.load(open(path))


@pytest.fixture(scope="module")
def run(table):
    import stock_market_monte_carlo_amd as S
    spec = importlib.util.spec_from_file_location("make_wave_walk_golden", os.path.join(GOLDEN, "make_wave_walk_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    eng = S.Engine(0)
    geometry = list(eng.geometry())
    got = gen.digests(S, eng, table)
    eng.close()
    return geometry, got


def test_every_output_byte_is_the_parents(recorded, run):
    geometry, got = run
    assert geometry == recorded["geometry"], (
        f"the recorded digests belong to the launch geometry (grid, block, compute units) {recorded['geometry']}; this engine has "
        f"{geometry}: the partial sums are folded per workgroup, so the records' bytes differ with it")
    assert sorted(got) == sorted(recorded["cases"])
    differing = {case: sorted(k for k in bufs if bufs[k] != recorded["cases"][case].get(k))
                 for case, bufs in got.items() if bufs != recorded["cases"][case]}
    assert not differing, f"{len(differing)} of {len(got)} cases differ from the parent's bytes: {dict(list(differing.items())[:8])}"
