"""smmc_engine_simulate_portfolio_cashflow_blocks on the device against the numpy restatement of its contract
(tests/portfolio_cashflow_blocks_reference.py), bit for bit: final values, holdings, totals paid, periods of depletion and
the depletion counts; of the record the integer counters, buckets, min and max on their bits, the two double sums to the
relative 1e-12 of tests/test_gpu_parity.py against math.fsum of the restated binary32 values and of their squares.

Tables: 37 rows with K = 1 .. 4 (eight block starts per Philox block), 2500 rows x 2 assets (four), 5 rows x 2 assets (fewer
rows than a segment) and 1 row x 1 asset; path ids from 2^32 - 100 on; 64 * 4 * 2 + 37 = 549 paths: whole chunks, a ragged one
and inactive lanes.  L in 1, 3, 8, 9, 12, 40, 64 (tails of 1 and 4, L > T = 37, L > P), P in 1, 7, 8, 9, 41, R in 0, 1, 5, 12 on
the sparse, covering product of the reference module (every (L, P) with every R, the four schedules cycling), then L = 12
and L = 5 with R = 12 and once more with a weight of exactly 0.  tests/test_portfolio_cashflow_blocks_cpu.py shows that
the reviewed edges of the row walk occur among these cases and that the schedules deplete 10 % .. 90 % of the paths.

The later walk trips run in a fresh child process with SMMC_BLOCKS_PER_CU=1 (the knob is read when an engine is made), as
tests/test_real_cashflow_gpu.py does; their sizes rest on host_wave_walk_grid capping the launch at min(chunks, grid).

On the commit before this feature every test here fails: the symbols do not exist.  A build with the row rule wrong on
purpose -- every run starts one row late, (s_b + 1) mod n_rows (tools/variant_build.py, loaded through SMMC_LIB) -- fails 28
of the 35 tests here and 36 of the 40 cases of tests/test_portfolio_cashflow_blocks_fuzz_gpu.py on the device; what passes
is the table of one row and the tests that compare the call with itself (host form, NULL outputs, repeat calls)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import portfolio_cashflow_blocks_reference as B

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("portfolio_cashflow_blocks")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, LO, HI, BELOW = B.BINS, B.LO, B.HI, B.BELOW
STATS = dict(n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
ALL = dict(want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
WANTS = {k: v for k, v in ALL.items() if k != "want_stats"}
KEYS = ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engines():
    """One engine per table, made on first use; none has a single-series table unless a test sets one."""
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(T, K):
        if (T, K) not in made:
            made[T, K] = S.Engine(0)
            made[T, K].set_asset_table(B.asset_table(T, K))
        return made[T, K]

    yield get
    for e in made.values():
        e.close()


def _sim(n, P, first=0, **kw):
    import stock_market_monte_carlo_amd as S
    return S.Engine.make_sim(n, P, S.MODE_TABLE, B.SEED, first_path=B.FIRST_PATH + first, initial_capital=B.CAPITAL, **kw)


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
    for T, K in B.TABLES:
        yield T, K, B.WEIGHTS[K]
    yield B.ZERO_WEIGHT + (B.WEIGHTS_WITH_ZERO[B.ZERO_WEIGHT[1]],)


# 1
@pytest.mark.parametrize("T,K,weights", list(_cases()))
def test_outputs_bit_for_bit(oracle, engines, T, K, weights):
    """Every L and P with every R, the schedules cycling; then the rebalance on and inside a block's boundary."""
    eng = engines(T, K)
    for L, P, R, name in B.device_cases(T):
        want = B.reference(oracle, T, K, weights, R, name, P, L)
        kw = B.cut(B.schedules(oracle, T, K, weights, L)[name], P)
        r = eng.simulate_portfolio_cashflow_blocks(_sim(B.N, P), weights, L, R, **kw, **WANTS)
        _check_outputs(r, want, (T, K, weights, L, P, R, name))


# 2
@pytest.mark.parametrize("T", [37, 2500])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_every_instantiation_and_both_divides(oracle, engines, T, K):
    """(dense | four-draw table) x K x (constant | varying schedule) x (IEEE | reciprocal-multiply divide): a request whose
    rule says FAST, the same with SMMC_FLAG_EXACT_DIV, and the reference, equal bits; L = 12 and 9, R = 5, P = 41."""
    from stock_market_monte_carlo_amd import _lib
    eng, w, P, R = engines(T, K), B.WEIGHTS[K], B.LONGEST, 5
    for L in (12, 9):
        for form, kw in B.fast_schedules(oracle, T, K, w, L).items():
            fast, exact = _sim(B.N, P), _sim(B.N, P, exact_div=True)
            assert eng.portfolio_cashflow_blocks_divide_kind(fast, w, L, R, **kw) == _lib.DIV_FAST, (form, L)
            assert eng.portfolio_cashflow_blocks_divide_kind(exact, w, L, R, **kw) == _lib.DIV_EXACT, (form, L)
            assert eng.portfolio_cashflow_divide_kind(fast, w, R, **kw) == _lib.DIV_FAST
            want = B.pcref.simulate(B.multipliers(oracle, T, K, L), w, R, **kw)
            if form == "constant":
                assert 0.10 <= 1.0 - want["depleted_at"][0] / B.N <= 0.90, (T, K, L)
            for sim in (fast, exact):
                _check_outputs(eng.simulate_portfolio_cashflow_blocks(sim, w, L, R, **kw, **WANTS), want, (T, K, L, form))
        # unproven requests take the IEEE divide: the varying and the fraction schedules of test 1
        assert eng.portfolio_cashflow_blocks_divide_kind(_sim(B.N, P), w, L, R, fraction=0.004) == _lib.DIV_EXACT
    if T == 2500 and K != 2:  # the four-draw table with K = 1, 3, 4 runs nowhere else: one varying and one fraction schedule
        for name in ("varying", "fraction"):
            want = B.reference(oracle, T, K, w, R, name, P, 9)
            r = eng.simulate_portfolio_cashflow_blocks(_sim(B.N, P), w, 9, R, **B.schedules(oracle, T, K, w, 9)[name], **WANTS)
            _check_outputs(r, want, (T, K, name))


# 3
@pytest.mark.parametrize("T,K,name,L", [(37, 3, "amount", 12), (2500, 2, "varying", 9), (5, 2, "floor", 40)])
def test_the_record_of_the_final_values(oracle, engines, T, K, name, L):
    eng, P = engines(T, K), B.LONGEST
    want = B.reference(oracle, T, K, B.WEIGHTS[K], 12, name, P, L)
    r = eng.simulate_portfolio_cashflow_blocks(_sim(B.N, P, **STATS), B.WEIGHTS[K], L, 12, want_final=False, want_stats=True,
                                               **B.schedules(oracle, T, K, B.WEIGHTS[K], L)[name])
    assert r.final is None and r.holdings is None and r.paid is None
    _check_record(oracle, r.stats, want["final"], (T, K, name, L))
    assert np.array_equal(r.depleted_at, want["depleted_at"])
    assert r.survival()[-1] == pytest.approx(want["depleted_at"][0] / B.N)


# 4: identity 1
@pytest.mark.parametrize("T,K", [(37, 1), (37, 4), (2500, 2), (5, 2), (1, 1)])
def test_block_length_one_is_simulate_portfolio_cashflow(oracle, engines, T, K):
    eng, w = engines(T, K), B.WEIGHTS[K]
    for name, R, P in (("amount", 5, B.LONGEST), ("varying", 12, B.LONGEST), ("floor", 1, 9), ("fraction", 0, 7)):
        kw = B.cut(B.schedules(oracle, T, K, w, 1)[name], P)
        sim = _sim(B.N, P, **STATS)
        want = eng.simulate_portfolio_cashflow_raw(sim, w, R, **kw, **ALL)
        got = eng.simulate_portfolio_cashflow_blocks_raw(sim, w, 1, R, **kw, **ALL)
        eng.sync()
        for key in ("final", "holdings", "paid", "ruin_period", "depleted_at"):
            assert got[key].cpu().numpy().tobytes() == want[key].cpu().numpy().tobytes(), (T, K, name, key)
        import stock_market_monte_carlo_amd as S
        a, b = (S.engine.stats_from_bytes(x["stats_raw"].cpu().numpy().tobytes()) for x in (got, want))
        assert (a.count, a.below, a.underflow, a.overflow, a.min, a.max) == (b.count, b.below, b.underflow, b.overflow, b.min, b.max)
        assert np.array_equal(a.hist, b.hist)
        assert a.sum == pytest.approx(b.sum, rel=1e-12) and a.sumsq == pytest.approx(b.sumsq, rel=1e-12)


# 5: identity 2
@pytest.mark.parametrize("T", [37, 2500, 5])
def test_one_asset_without_flows_is_simulate_blocks_on_that_column(T):
    import stock_market_monte_carlo_amd as S
    column = B.asset_table(T, 1)
    eng = S.Engine(0)
    try:
        eng.set_table(column[:, 0])
        eng.set_asset_table(column)
        for L in (1, 3, 9, 12, 40, 64):
            for P in (9, B.LONGEST):
                for exact in (False, True):  # whatever divide either call takes
                    sim = _sim(B.N, P, exact_div=exact)
                    want = eng.simulate_blocks(sim, L).final.cpu().numpy()
                    assert np.isfinite(want).all() and (want > 0).all()
                    got = eng.simulate_portfolio_cashflow_blocks(sim, (1.0,), L, 0, **WANTS)
                    assert got.final.cpu().numpy().tobytes() == want.tobytes(), (T, L, P, exact)
                    assert got.holdings.cpu().numpy().tobytes() == want.tobytes() and got.depleted_at[0] == B.N
                    assert not got.paid.cpu().numpy().any() and not got.ruin_period.cpu().numpy().any()
    finally:
        eng.close()


# 6
@pytest.mark.parametrize("T,K,name,L", [(37, 3, "varying", 9), (5, 2, "amount", 12)])
def test_two_shards_split_at_an_odd_path_are_the_whole_request(oracle, engines, T, K, name, L):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes
    eng, P, cut, w = engines(T, K), 24, 333, B.WEIGHTS[K]
    kw = B.cut(B.schedules(oracle, T, K, w, L)[name], P)

    def run(first, count):
        raw = eng.simulate_portfolio_cashflow_blocks_raw(_sim(count, P, first=first, **STATS), w, L, 5, **ALL, **kw)
        eng.sync()
        return {k: raw[k].cpu().numpy() for k in KEYS}

    whole, lo, hi = run(0, B.N), run(0, cut), run(cut, B.N - cut)
    for key in ("final", "paid", "ruin_period"):
        assert np.concatenate([lo[key], hi[key]]).tobytes() == whole[key].tobytes(), key
    assert np.concatenate([lo["holdings"], hi["holdings"]], axis=1).tobytes() == whole["holdings"].tobytes()
    assert np.array_equal(lo["depleted_at"] + hi["depleted_at"], whole["depleted_at"])
    merged = S.engine.stats_from_bytes(merge_stats_bytes([lo["stats_raw"].tobytes(), hi["stats_raw"].tobytes()]))
    want = S.engine.stats_from_bytes(whole["stats_raw"].tobytes())
    assert (merged.count, merged.below, merged.underflow, merged.overflow) == (want.count, want.below, want.underflow, want.overflow)
    assert merged.min == want.min and merged.max == want.max and np.array_equal(merged.hist, want.hist)
    assert merged.sum == pytest.approx(want.sum, rel=1e-12) and merged.sumsq == pytest.approx(want.sumsq, rel=1e-12)
    assert np.array_equal(_bits(whole["final"]), _bits(B.reference(oracle, T, K, w, 5, name, P, L)["final"]))


# 7
@pytest.mark.parametrize("T,K,name,L", [(37, 4, "varying", 12), (2500, 2, "fraction", 3)])
def test_the_host_form_is_the_device_form_and_no_paths_is_empty(oracle, engines, T, K, name, L):
    eng, P, w = engines(T, K), 24, B.WEIGHTS[K]
    kw = B.cut(B.schedules(oracle, T, K, w, L)[name], P)
    sim = _sim(B.N, P, **STATS)
    raw = eng.simulate_portfolio_cashflow_blocks_raw(sim, w, L, 12, **ALL, **kw)
    eng.sync()
    host = eng.simulate_portfolio_cashflow_blocks_to_host(sim, w, L, 12, **ALL, **kw)
    for key in KEYS:
        h = host[key] if isinstance(host[key], bytes) else host[key].tobytes()
        assert h == raw[key].cpu().numpy().tobytes(), key
    empty = eng.simulate_portfolio_cashflow_blocks_to_host(_sim(0, P, **STATS), w, L, 12, **ALL, **kw)
    assert not empty["depleted_at"].any() and empty["final"].size == 0 and empty["holdings"].shape == (K, 0)
    assert not np.frombuffer(empty["stats_raw"], dtype=np.uint64)[:4].any()  # count, below, underflow, overflow
    none = eng.simulate_portfolio_cashflow_blocks(_sim(0, P, **STATS), w, L, 12, **ALL, **kw)
    assert none.final.numel() == 0 and not none.depleted_at.any() and none.stats.count == 0


# 8
def test_null_outputs_singly_and_all_together(oracle, engines):
    T, K, L, P, R, name = 37, 3, 9, 24, 5, "varying"
    eng, w = engines(T, K), B.WEIGHTS[K]
    kw = B.cut(B.schedules(oracle, T, K, w, L)[name], P)
    sim = _sim(B.N, P, **STATS)
    full = eng.simulate_portfolio_cashflow_blocks_raw(sim, w, L, R, **ALL, **kw)
    eng.sync()
    full = {k: full[k].cpu().numpy().tobytes() for k in KEYS}
    wants = dict(want_final=True, **ALL)
    for left_out in list(wants) + [None]:
        asked = {k: left_out is not None and k != left_out for k in wants}  # None: every output NULL
        raw = eng.simulate_portfolio_cashflow_blocks_raw(sim, w, L, R, **asked, **kw)
        eng.sync()
        for key in KEYS:
            want_key = "want_" + ("stats" if key == "stats_raw" else key)
            if asked[want_key]:
                assert raw[key].cpu().numpy().tobytes() == full[key], (left_out, key)
            else:
                assert raw[key] is None, (left_out, key)


# 9
@pytest.mark.parametrize("T,K,name,L", [(37, 2, "varying", 9), (5, 2, "amount", 40)])
def test_determinism_and_the_accumulators_are_left_zero(oracle, engines, T, K, name, L):
    import stock_market_monte_carlo_amd as S
    eng, P, w = engines(T, K), 24, B.WEIGHTS[K]
    kw = B.cut(B.schedules(oracle, T, K, w, L)[name], P)
    runs = []
    for _ in range(2):
        raw = eng.simulate_portfolio_cashflow_blocks_raw(_sim(B.N, P, **STATS), w, L, 5, **ALL, **kw)
        eng.sync()
        runs.append({k: raw[k].cpu().numpy().tobytes() for k in KEYS})
    assert runs[0] == runs[1]
    assert int(np.frombuffer(runs[0]["depleted_at"], dtype=np.uint64).sum()) == B.N
    # a plain simulate with buckets straight afterwards: its record is its own
    plain = S.Engine.make_sim(1000, 36, S.MODE_GAUSSIAN, 99, **STATS)
    st = eng.read_stats(eng.simulate(plain, want_final=False, want_stats=True).stats_raw)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 36, 1000, 99, **STATS))
    assert np.array_equal(st.hist, o["hist"]) and st.below == o["stats"].below and st.count == 1000
    # and a run of fewer periods straight after that: its depletion counts are its own
    short = eng.simulate_portfolio_cashflow_blocks(_sim(B.N, 7), w, L, 5, **B.cut(kw, 7))
    assert np.array_equal(short.depleted_at, B.reference(oracle, T, K, w, 5, name, 7, L)["depleted_at"])


# 10
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import portfolio_cashflow_blocks_reference as B
import stock_market_monte_carlo_amd as S
out, T, K, R, L = sys.argv[3], 37, 3, 5, 9
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
eng.set_asset_table(B.asset_table(T, K))
res = {"grid": grid}
kw = B.schedules(O, T, K, B.WEIGHTS[K], L)["varying"]
for n in (2 * 256 * grid + 37, 3 * 256 * grid - 1):
    sim = S.Engine.make_sim(n, B.LONGEST, S.MODE_TABLE, B.SEED, first_path=B.FIRST_PATH, initial_capital=B.CAPITAL, n_bins=B.BINS,
                            hist_lo=B.LO, hist_hi=B.HI, below_threshold=B.BELOW)
    raw = eng.simulate_portfolio_cashflow_blocks_raw(sim, B.WEIGHTS[K], L, R, want_holdings=True, want_paid=True, want_ruin_period=True,
                                                     want_stats=True, **kw)
    eng.sync()
    for key in ("final", "holdings", "paid", "ruin_period", "stats_raw", "depleted_at"):
        res[f"{n}:{key}"] = raw[key].cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 3, L = 9, R = 5, the varying schedule: every wave makes a second and a third trip, the lanes' records persist
    across them, and the starts, the period count and the schedule begin again with every path."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid, T, K, R, L, P = int(got["grid"]), 37, 3, 5, 9, B.LONGEST
    sizes = (2 * 256 * grid + 37, 3 * 256 * grid - 1)
    a = B.multipliers_of(oracle, B.asset_table(T, K), max(sizes), P, L)
    want = B.pcref.simulate(a, B.WEIGHTS[K], R, **B.schedules(oracle, T, K, B.WEIGHTS[K], L)["varying"])
    for n in sizes:
        assert np.array_equal(_bits(got[f"{n}:final"]), _bits(want["final"][:n])), n
        assert np.array_equal(_bits(got[f"{n}:holdings"]), _bits(want["holdings"][:, :n])), n
        assert np.array_equal(_bits(got[f"{n}:paid"]), _bits(want["paid"][:n])), n
        assert np.array_equal(got[f"{n}:ruin_period"].view(np.uint32), want["ruin_period"][:n]), n
        assert np.array_equal(got[f"{n}:depleted_at"].view(np.uint64), np.bincount(want["ruin_period"][:n], minlength=P + 1)), n
        _check_record(oracle, S.engine.stats_from_bytes(got[f"{n}:stats_raw"].tobytes()), want["final"][:n], n)
