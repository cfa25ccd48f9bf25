"""The circular block bootstrap (smmc_engine_simulate_blocks and its _to_host form, through the C ABI) on the GPU
against the numpy restatement over the CPU oracle (tests/blocks_reference.py).

Final values, histogram, counters, min and max are compared exactly; the two double sums to the relative 1e-12 of
tests/test_gpu_parity.py (the device adds in another order); chunk means and variances to the 1e-6 / 1e-5 of tests/test_gpu_parity.py.
Seed 0x5EED0123456789AB (both halves non-zero) and first_path 2^33 + 3 throughout.

The shapes are the smallest at which the loop can go wrong: tables of 1, 2 and 7 entries (shorter than a segment of 8
periods: the base wraps by 8 mod T), 1127 (the bundled months; four shifted copies, 16-byte reads), 2048 (the largest
table drawn eight starts per Philox block; one copy, 4-byte reads), 2049 and 16384 (four starts per block); block
lengths around the segment length (7, 8, 9), longer than the run (P + 5) and longer than the table (T + 3); run lengths
0, 1, around a segment, 8 L and 8 L + 1 (4 L and 4 L + 1 above 2048 entries: the first start taken from a second
Philox block); 1, 255, 256, 257 and 1000 paths."""
import json
import os

import numpy as np
import pytest

import blocks_reference as ref

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream(table):
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check_blocks(table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (table, L, P, n_paths)
CASES = [
    ("1", 1, 9, 257), ("1", 7, 360, 255), ("1", 4, 9, 1),
    ("2", 2, 17, 256), ("2", 5, 41, 257), ("2", 12, 360, 255),
    ("7", 9, 360, 1000), ("7", 10, 80, 255), ("7", 1, 8, 1), ("7", 8, 7, 257), ("7", 365, 360, 256),
    ("bundled", 12, 360, 1000), ("bundled", 1, 360, 1000), ("bundled", 2, 16, 257), ("bundled", 7, 57, 256),
    ("bundled", 8, 64, 255), ("bundled", 9, 73, 257), ("bundled", 360, 360, 256), ("bundled", 365, 360, 257),
    ("bundled", 1130, 1140, 255), ("bundled", 12, 0, 257), ("bundled", 12, 1, 1), ("bundled", 3, 7, 256),
    ("bundled", 12, 97, 1000), ("bundled", 8, 9, 255),
    ("2048", 12, 360, 257), ("2048", 2051, 360, 255), ("2048", 8, 65, 256), ("2048", 1, 8, 1),
    ("2049", 12, 49, 257), ("2049", 7, 28, 256), ("2049", 9, 360, 1000), ("2049", 1, 9, 255), ("2049", 2052, 360, 1),
    ("16384", 12, 360, 257), ("16384", 16387, 360, 255), ("16384", 8, 33, 256), ("16384", 2, 9, 1000),
]
# the same loop through the other LDS layout: one copy and 4-byte reads where four copies would be chosen
NARROW_CASES = [("1", 7, 360, 255), ("7", 9, 360, 1000), ("bundled", 12, 360, 1000), ("bundled", 9, 73, 257),
                ("bundled", 1130, 1140, 255)]
WIDE_CASES = [("2048", 12, 360, 257), ("2049", 9, 360, 1000)]  # ... and four copies where one would be chosen


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engines():
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(key):
        if key not in made:
            made[key] = S.Engine(0)
            made[key].set_table(ref.table_of(key))
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _sim(n, P, first=ref.FIRST_PATH, exact_div=False, n_bins=ref.BINS, capital=ref.CAPITAL):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(n, P, S.MODE_TABLE, ref.SEED, first_path=first, initial_capital=capital, n_bins=n_bins,
                             hist_lo=ref.LO, hist_hi=ref.HI, below_threshold=ref.BELOW, exact_div=exact_div)


def _run(eng, sim, L, final=True, chunks=True, stats=True):
    raw = eng.simulate_blocks_raw(sim, L, want_final=final, want_chunk_stats=chunks, want_stats=stats)
    eng.sync()
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in raw.items()}
    if out["stats_raw"] is not None:
        out["stats_raw"] = out["stats_raw"].tobytes()
    return out


def _check(got, want, n, tag):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    if got["final"] is not None:
        assert np.array_equal(_bits(got["final"]), _bits(want["final"])), tag
    if got["stats_raw"] is not None:
        st, ost = stats_from_bytes(got["stats_raw"]), want["stats"]
        assert st.count == ost.count == n, tag
        assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
        assert np.array_equal(st.hist, want["hist"]), tag
        if n:
            assert st.min == ost.min and st.max == ost.max, tag
        if np.isfinite(ost.sumsq):
            assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag
        else:
            assert st.sum == ost.sum and st.sumsq == ost.sumsq, tag
    if got["chunk_mean"] is not None and n:
        assert np.allclose(got["chunk_mean"], want["chunk_mean"], rtol=1e-6, atol=0.0), tag
        assert np.allclose(got["chunk_var"], want["chunk_var"], rtol=1e-5, atol=1e-6 * float(np.max(want["chunk_var"]) + 1)), tag


@pytest.mark.parametrize("key,L,P,n", CASES)
def test_against_the_restatement(engines, oracle, key, L, P, n):
    want = ref.cached_result(oracle, key, n, P, L)
    _check(_run(engines(key), _sim(n, P), L), want, n, (key, L, P, n))


@pytest.mark.parametrize("read,cases", [("b32", NARROW_CASES), ("b128", WIDE_CASES)])
def test_the_other_lds_layout(engines, oracle, monkeypatch, read, cases):
    monkeypatch.setenv("SMMC_BLOCKS_READ", read)
    for key, L, P, n in cases:
        _check(_run(engines(key), _sim(n, P), L), ref.cached_result(oracle, key, n, P, L), n, (read, key, L, P, n))


@pytest.mark.parametrize("key,P,n", [("bundled", 360, 1000), ("7", 9, 257), ("2049", 41, 256)])
def test_block_length_one_is_simulate(engines, key, P, n):
    """L = 1 against smmc_engine_simulate in table mode on the same engine: every byte."""
    eng, sim = engines(key), _sim(n, P)
    a = _run(eng, sim, 1)
    r = eng.simulate(sim, want_final=True, want_chunk_stats=True, want_stats=True)
    eng.sync()
    assert np.array_equal(_bits(a["final"]), _bits(r.final.cpu().numpy()))
    assert a["stats_raw"] == r.stats_raw.cpu().numpy().tobytes()
    assert np.array_equal(_bits(a["chunk_mean"]), _bits(r.chunk_mean.cpu().numpy()))
    assert np.array_equal(_bits(a["chunk_var"]), _bits(r.chunk_var.cpu().numpy()))


def test_prefix_property_on_the_device(engines, oracle):
    """P = 1 .. 20 at L = 3: each run is column P of the restatement's trajectories."""
    eng, table, n = engines("bundled"), ref.table_of("bundled"), 64
    traj = np.stack([ref.trajectory(oracle, table, ref.SEED, ref.FIRST_PATH + i, 20, 3) for i in range(n)])
    for P in range(1, 21):
        got = _run(eng, _sim(n, P), 3, chunks=False, stats=False)["final"]
        assert np.array_equal(_bits(got), _bits(traj[:, P])), P


def test_divide_variants_with_the_extreme_months(engines, oracle):
    """The 1127 months with the S&P 500's best and worst month (+42.2 %, -29.7 %) cannot be proven safe for the fast
    divide over 360 periods: CHECKED, and forced EXACT gives the same bits (the bundled synthetic months alone are
    provably safe: FAST).  A +-1 % table is FAST, and its forced EXACT agrees too."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import _lib
    eng, n = engines("extremes"), 1000
    assert eng.blocks_divide_kind(_sim(n, 360), 12) == _lib.DIV_CHECKED
    assert eng.blocks_divide_kind(_sim(n, 360, exact_div=True), 12) == _lib.DIV_EXACT
    assert engines("bundled").blocks_divide_kind(_sim(n, 360), 12) == _lib.DIV_FAST
    want = ref.cached_result(oracle, "extremes", n, 360, 12)
    _check(_run(eng, _sim(n, 360), 12), want, n, "checked")
    _check(_run(eng, _sim(n, 360, exact_div=True), 12), want, n, "exact")
    calm = S.Engine(0)
    try:
        calm_table = np.where(np.arange(64) % 3 == 0, -1.0, 1.0).astype(np.float32)
        calm.set_table(calm_table)
        assert calm.blocks_divide_kind(_sim(n, 360), 12) == _lib.DIV_FAST
        want = ref.result(oracle, calm_table, n, 360, 12)
        _check(_run(calm, _sim(n, 360), 12), want, n, "fast")
        _check(_run(calm, _sim(n, 360, exact_div=True), 12), want, n, "fast table, exact")
    finally:
        calm.close()


def test_redo_of_paths_that_leave_the_checked_window(engines, oracle):
    """Five +100 % and three -50 % months, L = 4, 360 periods, 4096 paths: CHECKED with a window of about
    [2^-81, 2^111]; a third of the paths leave it and are redone with the IEEE divide, a tenth end at +inf."""
    from stock_market_monte_carlo_amd import _lib
    eng, n = engines("redo"), 4096
    sim = _sim(n, 360)
    assert eng.blocks_divide_kind(sim, 4) == _lib.DIV_CHECKED
    want = ref.cached_result(oracle, "redo", n, 360, 4)
    inf = int(np.isinf(want["final"]).sum())
    print(f"redo case: {inf} of {n} paths end at +inf")
    assert 0 < inf < n
    with np.errstate(all="ignore"):
        _check(_run(eng, sim, 4, chunks=False), want, n, "redo")
        _check(_run(eng, _sim(n, 360, exact_div=True), 4, chunks=False), want, n, "redo, exact")


def test_two_shards_equal_the_whole_run(engines):
    eng, n, cut = engines("bundled"), 1000, 300  # the cut is inside a chunk of 256
    whole = _run(eng, _sim(n, 360), 12, chunks=False, stats=False)["final"]
    a = _run(eng, _sim(cut, 360), 12, chunks=False, stats=False)["final"]
    b = _run(eng, _sim(n - cut, 360, first=ref.FIRST_PATH + cut), 12, chunks=False, stats=False)["final"]
    assert np.array_equal(_bits(np.concatenate([a, b])), _bits(whole))


def test_run_to_run_determinism(engines):
    eng, sim = engines("bundled"), _sim(1000, 360)
    a, b = _run(eng, sim, 12), _run(eng, sim, 12)
    assert np.array_equal(_bits(a["final"]), _bits(b["final"])) and a["stats_raw"] == b["stats_raw"]
    assert np.array_equal(_bits(a["chunk_var"]), _bits(b["chunk_var"]))


def test_null_outputs_in_every_combination(engines, oracle):
    eng, n = engines("bundled"), 257
    want = ref.cached_result(oracle, "bundled", n, 73, 9)
    for mask in range(8):
        got = _run(eng, _sim(n, 73), 9, final=bool(mask & 1), chunks=bool(mask & 2), stats=bool(mask & 4))
        assert (got["final"] is not None) == bool(mask & 1) and (got["stats_raw"] is not None) == bool(mask & 4)
        _check(got, want, n, mask)
    # no histogram, and no paths
    got = _run(eng, _sim(n, 73, n_bins=0), 9)
    assert np.array_equal(_bits(got["final"]), _bits(want["final"]))
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    st = stats_from_bytes(got["stats_raw"])
    assert st.count == n and st.min == want["stats"].min and st.hist.size == 0
    empty = _run(eng, _sim(0, 73), 9)
    assert stats_from_bytes(empty["stats_raw"]).count == 0 and empty["final"].size == 0


def test_to_host_against_the_device_result(oracle, monkeypatch):
    """1000 paths through chunks of 256 into a pageable buffer: the device call's values, merged records and chunks."""
    import stock_market_monte_carlo_amd as S
    monkeypatch.setenv("SMMC_HOST_CHUNK_PATHS", "256")
    eng = S.Engine(0)  # the knobs are read when an engine is created
    try:
        eng.set_table(ref.table_of("bundled"))
        n, sim = 1000, _sim(1000, 360)
        dev = _run(eng, sim, 12)
        host, st, (cm, cv) = eng.simulate_blocks_to_host(sim, 12, out=np.full(n, -1.0, dtype=np.float32), want_stats=True,
                                                          want_chunk_stats=True)
        want = ref.cached_result(oracle, "bundled", n, 360, 12)
        assert np.array_equal(_bits(host), _bits(dev["final"])) and np.array_equal(_bits(host), _bits(want["final"]))
        ost = want["stats"]
        assert (st.count, st.below, st.underflow, st.overflow) == (n, ost.below, ost.underflow, ost.overflow)
        assert st.min == ost.min and st.max == ost.max and np.array_equal(st.hist, want["hist"])
        assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12)
        # chunks of 256 paths are the chunk statistics' own groups: the same numbers as the device call's
        assert np.allclose(cm, dev["chunk_mean"], rtol=1e-6, atol=0.0) and np.allclose(cv, dev["chunk_var"], rtol=1e-5, atol=0.0)
        only_stats = eng.simulate_blocks_to_host(sim, 12, want_stats=True)[1]
        assert only_stats.count == n and np.array_equal(only_stats.hist, want["hist"])
    finally:
        eng.close()


def test_the_frozen_fixture(engines):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "blocks_v3.json")))
    assert doc["seed"] == ref.SEED and doc["first_path"] == ref.FIRST_PATH
    for case in doc["cases"]:
        n, P, L = case["n_paths"], case["n_periods"], case["block_len"]
        got = _run(engines(case["table"]), _sim(n, P), L, chunks=False, stats=False)["final"]
        assert np.array_equal(_bits(got), np.array(case["final_bits"], dtype=np.uint32)), case["table"]


def test_refusals_on_the_device(engines):
    import stock_market_monte_carlo_amd as S
    eng = engines("bundled")
    with pytest.raises(S.SmmcError, match="block_len"):
        eng.simulate_blocks(_sim(10, 5), 0)
    bad = S.Engine.make_sim(10, 5, S.MODE_GAUSSIAN, 1)
    with pytest.raises(S.SmmcError, match="SMMC_MODE_TABLE"):
        eng.simulate_blocks(bad, 3)
    v2 = S.Engine.make_sim(10, 5, S.MODE_TABLE, 1, stream=2)
    with pytest.raises(S.SmmcError, match="V2"):
        eng.simulate_blocks(v2, 3)
